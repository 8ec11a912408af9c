// In-order TCP delivery into socket rings (fs_deliver_flows_batch): behind the launches of the
// flow-aware coalesce (framesum_flows.hip), whose per-slot scratch of the same call these kernels
// read -- the sort keys (slot k's frame), the slot records (payload start, length, flags byte, the
// flow heads), the key records and the flow numbers -- admit each listed socket's data segments in
// order and copy their bytes from the frames into the socket's ring.
//
// The launches on the caller's stream, none of which waits on another workgroup or wave of its own
// launch, every loop bounded by a count known at its start:
//   (memset)  the per-slot ring positions and the per-socket first slots to "none", `delivered` to 0.
//   match     flow_match (framesum_match_dev.h) over the staged socket table: the flow's socket, the
//             socket's first slot.
//   mark      one lane per slot of a matched flow: Seq and Ack from the frame at L4 = 14 + 4 IHL, and
//             the bits of the rule that do not depend on the frames before: considered, window and
//             ACK check, SYN | RST, FIN (framesum_deliver.h mark_word).
//   walk      one wave per socket, the sequential part: the flow's slots in chunks of 64, the loads
//             of four chunks in flight together (the next four's while these are walked); a wave
//             scan over the lengths gives every lane the state it meets if the lanes before it are
//             admitted, a ballot finds the first lane that is not, and the walk restarts behind it
//             (at most the flow's frames); per slot the ring position or "none" and `delivered`,
//             per socket the out record.
//   copy      sixteen lanes per slot, as the gather's copy: copy_payload once per contiguous piece,
//             two pieces at the wrap; the sources are the frames.
#include <hip/hip_runtime.h>

#include <rocprim/warp/warp_scan.hpp>

#include "../../include/framesum_deliver.h"
#include "framesum_coalesce.h"
#include "framesum_coalesce_dev.h"
#include "framesum_deliver.h"
#include "framesum_flows.h"
#include "framesum_internal.h"
#include "framesum_match_dev.h"

namespace framesum {

namespace {

using namespace codev;
namespace dl = deliver;

// (the match's record in front: the owners are the listed sockets)
struct DlArgs : FlowMatch<fs_rx_sock> {
    const uint8_t* frames;
    const uint64_t* offsets;
    const fs_rx_flow_totals* totals;
    // this call's own scratch
    uint2* mk;        // per slot of a matched flow: Seq, mark_word
    uint32_t* dwpos;  // per slot: where in its socket's ring the payload goes, or none
    uint8_t* rings;
    fs_rx_sock_out* socks_out;
    uint8_t* delivered;
};

__device__ __forceinline__ uint32_t be32_at(const uint8_t* p) { return __builtin_bswap32(load_at<uint32_t>(p)); }

__global__ void __launch_bounds__(kThreads) deliver_mark(const DlArgs a) {
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t k = blk * kScanBlock + threadIdx.x;
        if (k >= a.n) continue;
        const uint2 r = a.rec[k];
        if (!(r.y & kAccepted)) continue;
        const uint32_t s = a.flow_owner[a.flowidx[k]];
        if (s >= a.n_owners) continue;
        // an accepted TCP frame holds its whole TCP header (the verdict's gates)
        const uint8_t* __restrict__ p = a.frames + a.offsets[slot_frame(a, k)];
        const uint32_t l4 = 14u + 4u * (p[14] & 15u);
        const uint32_t seq = be32_at(p + l4 + 4u), ack = be32_at(p + l4 + 8u);
        a.mk[k] = make_uint2(seq, dl::mark_word(rec_len(r.x), rec_flags(r.x), ack, a.recs[s].rcv_wnd, a.recs[s].snd_nxt));
    }
}

// What a lane holds of its slot of a chunk: in the flow or not, Seq, the mark word, the slot's frame.
// The three loads do not wait for each other (a slot outside the flow reads scratch it does not use).
struct Held {
    uint32_t in, seq, word, frame;
};
__device__ __forceinline__ Held hold(const DlArgs& a, uint32_t first, uint32_t k, uint32_t n_acc) {
    Held h{0u, 0u, 0u, 0u};
    if (k < n_acc) {
        const uint32_t y = a.rec[k].y;
        const uint2 m = a.mk[k];
        h.frame = slot_frame(a, k);
        h.in = (k == first || !(y & flows::kFlowHead)) ? 1u : 0u;
        h.seq = m.x, h.word = m.y;
    }
    return h;
}

// The inclusive sum over the lanes up to and including this one (rocPRIM's wave scan).
using WaveScan = rocprim::warp_scan<uint32_t, 64>;
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, WaveScan::storage_type& storage) {
    uint32_t out;
    WaveScan().inclusive_scan(v, out, storage);
    return out;
}
__device__ __forceinline__ unsigned long long lanes_below(uint32_t l) { return l >= 64u ? ~0ull : (1ull << l) - 1ull; }

// One chunk of a socket's walk: the 64 slots from `base` on, of which lane l holds slot base + l in
// `cur`. Advances the state `st` and the out record `o`; returns true when the walk has ended (its
// `stop` is set then). Every value that steers the loop is the same in all lanes.
__device__ __forceinline__ bool walk_chunk(const DlArgs& a, uint32_t ring_size, uint32_t base, uint32_t lane, const Held& cur,
                                           dl::State& st, fs_rx_sock_out& o, WaveScan::storage_type& storage) {
    const unsigned long long out_of_flow = __ballot(cur.in == 0u);
    const uint32_t cnt = out_of_flow ? (uint32_t)__builtin_ctzll(out_of_flow) : 64u;
    uint32_t my_pos = dl::kNone, my_del = 0u;
    bool done = false;
    // A candidate passes everything that does not depend on the frames before. If every candidate
    // from lane `at` on is admitted, lane l meets the state advanced by the candidates in [at, l):
    // one scan per chunk gives that state to every lane at once, and the first lane that does not
    // pass under it is decided exactly, since the lanes before it do pass. The walk restarts behind
    // such a lane: at most once per lane.
    const bool in = lane < cnt;
    const bool stop = in && (cur.word & dl::kMkStop) != 0;
    const bool cons = in && !stop && (cur.word & dl::kMkConsidered) != 0;
    const bool cand = cons && (cur.word & dl::kMkFixedOk) != 0;
    const uint32_t len = cur.word & 0xFFFFu, fin = (cur.word & dl::kMkFin) ? 1u : 0u;
    // Seq advances by len + fin: the lengths by one scan, the FINs by counting a ballot's bits
    const uint32_t c_len = cand ? len : 0u;
    const uint32_t i_len = wave_scan(c_len, storage), e_len = i_len - c_len;  // (64 x 65,536 < 2^32)
    const unsigned long long fins = __ballot(cand && fin != 0u), stops = __ballot(stop);
    const uint32_t e_fin = (uint32_t)__popcll(fins & lanes_below(lane));
    for (uint32_t at = 0; at < cnt;) {
        const uint32_t b_len = lane_value(e_len, at), b_fin = (uint32_t)__popcll(fins & lanes_below(at));
        const uint32_t p_len = e_len - b_len, p_seq = p_len + (e_fin - b_fin);
        const bool live = in && lane >= at;
        const bool ok = cand && dl::in_order_and_fits(dl::State{st.nxt + p_seq, 0u, st.free - p_len}, cur.seq, len);
        const unsigned long long bad_mask = __ballot(live && (stop || (cons && !ok)));
        const unsigned long long fin_mask = __ballot(live && ok && fin != 0u);
        const uint32_t bad = bad_mask ? (uint32_t)__builtin_ctzll(bad_mask) : cnt;
        const uint32_t fin_at = fin_mask ? (uint32_t)__builtin_ctzll(fin_mask) : 64u;
        const bool ends = fin_at < bad;  // an admitted FIN ends the walk
        const uint32_t upto = ends ? fin_at + 1u : bad;
        const bool mine = live && lane < upto && cand;  // admitted
        if (mine) {
            const uint32_t pos = st.wpos + p_len;  // (below 2^31 + 2^22)
            my_pos = pos >= ring_size ? pos - ring_size : pos;
            my_del = 1u;
        }
        if (upto > at) {
            const uint32_t t_len = lane_value(i_len, upto - 1u) - b_len;
            const uint32_t t_seq = t_len + ((uint32_t)__popcll(fins & lanes_below(upto)) - b_fin);
            const uint32_t pos = st.wpos + t_len;  // (t_len <= free <= ring_size)
            st.nxt += t_seq;
            st.free -= t_len;
            st.wpos = pos >= ring_size ? pos - ring_size : pos;
            o.bytes += t_len;
            o.n_delivered += (uint32_t)__popcll(__ballot(mine));
        }
        if (ends) {
            o.stop = base + upto;
            done = true;
            break;
        }
        if (bad >= cnt) break;
        if ((stops >> bad) & 1ull) {  // SYN or RST: this frame and the later ones are the host's
            o.stop = base + bad;
            done = true;
            break;
        }
        if (lane == bad) my_del = 2u;
        o.n_dropped += 1u;
        at = bad + 1u;
    }
    if (my_del == 1u) a.dwpos[base + lane] = my_pos;
    if (my_del != 0u && a.delivered) a.delivered[cur.frame] = (uint8_t)my_del;
    if (!done && cnt < 64u) {  // the flow ends inside this chunk
        o.stop = base + cnt;
        done = true;
    }
    return done;
}

// Chunks whose loads are in flight together: the walk's time is the latency of one round of loads per
// kAhead chunks, not per chunk.
constexpr uint32_t kAhead = 4;

__global__ void __launch_bounds__(kThreads) deliver_walk(const DlArgs a) {
    __shared__ WaveScan::storage_type s_scan[kWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t s = blockIdx.x * kWaves + wave; s < a.n_owners; s += gridDim.x * kWaves) {
        const fs_rx_sock sk = a.recs[s];
        fs_rx_sock_out o = dl::untouched(sk);
        const uint32_t first = a.owner_first[s];
        if (first < a.n) {
            const uint32_t n_acc = a.totals->n_accepted < a.n ? a.totals->n_accepted : a.n;
            dl::State st{sk.rcv_nxt, sk.ring_wpos, sk.ring_free};
            bool done = false;
            o.flow = a.flowidx[first];
            Held cur[kAhead], next[kAhead];
#pragma unroll
            for (uint32_t c = 0; c < kAhead; ++c) cur[c] = hold(a, first, first + 64u * c + lane, n_acc);
            // (at most the accepted slots from `first` on: ceil((n_acc - first) / 256) rounds)
            for (uint32_t base = first; base < n_acc && !done; base += 64u * kAhead) {
#pragma unroll
                for (uint32_t c = 0; c < kAhead; ++c) next[c] = hold(a, first, base + 64u * (kAhead + c) + lane, n_acc);
#pragma unroll
                for (uint32_t c = 0; c < kAhead; ++c)
                    if (!done && base + 64u * c < n_acc) done = walk_chunk(a, sk.ring_size, base + 64u * c, lane, cur[c], st, o, s_scan[wave]);
#pragma unroll
                for (uint32_t c = 0; c < kAhead; ++c) cur[c] = next[c];
            }
            if (!done) o.stop = n_acc;  // the flow ends with the last accepted slot
            o.rcv_nxt = st.nxt, o.ring_wpos = st.wpos, o.ring_free = st.free;
        }
        if (lane == 0) a.socks_out[s] = o;
    }
}

__global__ void __launch_bounds__(kThreads) deliver_copy(const DlArgs a) {
    const uint32_t sub = threadIdx.x & (kGroup - 1u), grp = threadIdx.x / kGroup;
    const uint32_t n_tiles = (a.n + kTileFrames - 1u) / kTileFrames;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t k = tile * kTileFrames + grp;
        if (k >= a.n) continue;
        const uint32_t pos = a.dwpos[k];
        if (pos == dl::kNone) continue;
        const uint32_t x = a.rec[k].x, len = rec_len(x);
        const uint32_t s = a.flow_owner[a.flowidx[k]];
        if (len == 0 || s >= a.n_owners) continue;  // (an admitted FIN without data)
        const uint64_t ring_off = a.recs[s].ring_off;
        const uint32_t size = a.recs[s].ring_size;
        if (pos >= size || len > size) continue;  // (the walk rules this out)
        const uint8_t* src = a.frames + a.offsets[slot_frame(a, k)] + rec_start(x);
        uint8_t* ring = a.rings + ring_off;
        const dl::Split sp = dl::split_at_wrap(pos, len, size);
        copy_payload(ring + pos, src, sp.first, sub);
        if (sp.second != 0) copy_payload(ring, src + sp.first, sp.second, sub);
    }
}

}  // namespace

DeliverScratch deliver_scratch(uint32_t n, uint32_t n_socks) {
    DeliverScratch s;
    uint64_t at = 0;
    s.mk = at, at += 8ull * n;
    s.dwpos = at, at += 4ull * n;  // dwpos and sock_first lie together: one memset covers both
    s.sock_first = at, at += 4ull * n_socks;
    s.flow_sock = at, at += 4ull * n;
    s.bytes = at;
    return s;
}

hipError_t launch_deliver(const RxBatch& b, const RxResults& r, const RxLeft& left, const uint8_t* d_block, uint32_t n_socks,
                          const RxLaunch& how) {
    uint8_t* const scratch = left.deliver_scratch;
    const DeliverScratch& s = left.ds;
    const uint32_t n = b.n;
    const hipStream_t stream = how.stream;
    const ScanGrid g = scan_grid(n, how);
    DlArgs a;
    fill_match(a, flow_view(left, n), d_block, dl::block_of(n_socks).table, reinterpret_cast<uint32_t*>(scratch + s.flow_sock),
               reinterpret_cast<uint32_t*>(scratch + s.sock_first), n, n_socks, how);
    a.frames = b.frames;
    a.offsets = b.offsets;
    a.totals = static_cast<const fs_rx_flow_totals*>(r.totals());
    a.mk = reinterpret_cast<uint2*>(scratch + s.mk);
    a.dwpos = reinterpret_cast<uint32_t*>(scratch + s.dwpos);
    a.rings = r.rings;
    a.socks_out = r.socks_out();
    a.delivered = r.delivered();
    const uint32_t n_tiles = (uint32_t)(((uint64_t)n + kTileFrames - 1) / kTileFrames);
    const uint32_t walk_blocks = (n_socks + kWaves - 1u) / kWaves;
    hipError_t e = hipMemsetAsync(scratch + s.dwpos, 0xFF, 4ull * n + 4ull * n_socks, stream);
    if (e != hipSuccess) return e;
    if (n != 0) {
        hipLaunchKernelGGL(flow_match<fs_rx_sock>, dim3(g.scan), dim3(kThreads), 0, stream, a);
        hipLaunchKernelGGL(deliver_mark, dim3(g.scan), dim3(kThreads), 0, stream, a);
    }
    hipLaunchKernelGGL(deliver_walk, dim3(g.capped(walk_blocks)), dim3(kThreads), 0, stream, a);
    if (n != 0) hipLaunchKernelGGL(deliver_copy, dim3(g.capped(n_tiles)), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace framesum
