// The active open of the connect call (fs_connect_flows_batch): behind the launches of the close call
// (framesum_close.hip), these kernels read what the flow launches left of the same call -- the sort keys
// (slot k's frame), the slot records (payload length, the flow heads), the key records, the flow numbers
// -- walk every opener's flow under the rule of framesum_connect.h and build the control frame each
// opener owes.
//
// The launches on the caller's stream, none of which waits on another workgroup or wave of its own
// launch, every loop bounded by a count known at its start:
//   (memset)  the openers' first slots to "none".
//   mark      one lane per slot that opens a flow: the probe of the staged opener table (at most every
//             table slot once); the flow's opener, the opener's first slot.
//   gather    one lane per slot of an opener's flow: Seq, Ack, the dword at L4 + 12 and the payload length
//             into per-slot scratch, so that the walk's loads are contiguous. (The input of the MSS option
//             walk, up to 40 bytes, is read from the one frame that needs it, by the walk itself.)
//   walk      one wave per opener: the flow's slots in chunks of 64, the next chunk's loads in flight
//             while this one is decided. The state is fixed until the walk ends, so one decision per chunk
//             suffices: all lanes run code_of, the first lane whose frame ends the walk (an event) is found
//             by ballot, the lanes below it are committed (their codes; the counts are popcounts), and
//             the event is applied wave-uniformly. Then the out record and, for an opener that owes a
//             frame, its record for the frame body.
//   reply     one wave per opener, the control-frame body (framesum_ctlframe_dev.h): the 54 header bytes,
//             both checksums, the FCS, the digest and the verdict.
#include <hip/hip_runtime.h>

#include "../../include/framesum_connect.h"
#include "framesum_coalesce.h"
#include "framesum_coalesce_dev.h"
#include "framesum_connect.h"
#include "framesum_ctlframe_dev.h"
#include "framesum_flows.h"
#include "framesum_internal.h"

namespace framesum {

namespace {

using namespace codev;
namespace cn = connect;

struct CnArgs : FlowView {  // (the flow launches' scratch of this call)
    const uint8_t* frames;
    const uint64_t* offsets;
    const fs_rx_flow_totals* totals;
    // the staged block
    const fs_cn_sock* openers;
    const uint32_t* table;
    // this call's own scratch
    uint32_t* flow_opener;     // per flow: its opener, or none
    uint32_t* opener_first;    // per opener: its flow's first slot, or none
    uint4* sq;                 // per slot of an opener's flow: Seq, Ack, the dword at L4 + 12, the payload length
    segment::SendRec* reprec;  // per opener with a reply: the reply as the frame body takes a record
    // the results
    fs_cn_out* openers_out;
    uint8_t* ctl_code;
    uint32_t n, n_blocks, n_openers, tmask, hash_mask;
};

__global__ void __launch_bounds__(kThreads) connect_mark(const CnArgs a) {
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t k = blk * kScanBlock + threadIdx.x;
        if (k >= a.n) continue;
        const uint32_t y = a.rec[k].y;
        if (!(y & kAccepted) || !(y & flows::kFlowHead)) continue;
        const uint32_t f = a.flowidx[k];
        if (f >= a.n) continue;  // (the flow launches rule this out)
        const uint4 v = a.keys[slot_frame(a, k)];
        const flows::Key key{{v.x, v.y, v.z, v.w}};
        uint32_t c = cn::kNone;
        if (flows::key_byte(key, 0) == 6u) c = cn::lookup_opener(key, a.openers, a.table, a.tmask, a.hash_mask);
        a.flow_opener[f] = c;
        if (c < a.n_openers) a.opener_first[c] = k;  // (distinct keys on both sides: one flow per opener)
    }
}

__global__ void __launch_bounds__(kThreads) connect_gather(const CnArgs a) {
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t k = blk * kScanBlock + threadIdx.x;
        if (k >= a.n) continue;
        const uint2 r = a.rec[k];
        if (!(r.y & kAccepted)) continue;
        const uint32_t f = a.flowidx[k];
        if (f >= a.n || a.flow_opener[f] >= a.n_openers) continue;
        // an accepted TCP frame holds its whole TCP header (the verdict's gates)
        const uint8_t* __restrict__ p = a.frames + a.offsets[slot_frame(a, k)];
        const uint32_t l4 = 14u + 4u * (p[14] & 15u);
        a.sq[k] = make_uint4(__builtin_bswap32(load_at<uint32_t>(p + l4 + 4u)), __builtin_bswap32(load_at<uint32_t>(p + l4 + 8u)),
                             load_at<uint32_t>(p + l4 + 12u), rec_len(r.x));
    }
}

// What a lane holds of its slot of a chunk: in the flow or not, the frame as the rule reads it, the
// slot's frame and its data offset. The loads do not wait for each other (a slot outside the flow reads
// scratch it does not use).
struct Held {
    uint32_t in, frame, doff;
    cn::Seg f;
};
__device__ __forceinline__ Held hold(const CnArgs& a, uint32_t first, uint32_t k, uint32_t n_acc) {
    Held h{0u, 0u, 0u, cn::Seg{0u, 0u, 0u, 0u, 0u}};
    if (k < n_acc) {
        const uint32_t y = a.rec[k].y;
        const uint4 q = a.sq[k];
        h.frame = slot_frame(a, k);
        h.in = (k == first || !(y & flows::kFlowHead)) ? 1u : 0u;
        h.doff = (q.z >> 4) & 15u;
        h.f = cn::Seg{q.x, q.y, recv::window_of(q.z), recv::flags9_of(q.z), q.w};
    }
    return h;
}

// The peer's MSS from the options of frame `frame` (the same frame in every lane), whose data offset is
// `doff`: accept::peer_mss over the 4 doff - 20 option bytes, which an accepted frame holds.
__device__ __forceinline__ uint32_t frame_mss(const CnArgs& a, uint32_t frame, uint32_t doff) {
    if (frame >= a.n || doff <= 5u) return 0u;
    const uint8_t* __restrict__ p = a.frames + a.offsets[frame];
    const uint32_t l4 = 14u + 4u * (p[14] & 15u);
    return accept::peer_mss(p + l4 + 20u, 4u * (doff - 5u));
}

__global__ void __launch_bounds__(kThreads) connect_walk(const CnArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = blockIdx.x * kWaves + wave; i < a.n_openers; i += gridDim.x * kWaves) {
        const fs_cn_sock sk = a.openers[i];
        fs_cn_out o = cn::untouched(sk);
        const uint32_t first = a.opener_first[i];
        if (first < a.n) {
            const uint32_t n_acc = a.totals->n_accepted < a.n ? a.totals->n_accepted : a.n;
            uint32_t n_rejected = 0, n_keepalive = 0;
            o.stop = first;
            uint32_t base = first;
            Held cur = hold(a, first, base + lane, n_acc);
            bool done = false;
            // (at most the accepted slots from `first` on: ceil((n_acc - first) / 64) rounds; every value that
            // steers the loop is the same in all lanes)
            for (; base < n_acc && !done; base += 64u) {
                const Held next = hold(a, first, base + 64u + lane, n_acc);
                const unsigned long long out_of_flow = __ballot(cur.in == 0u);
                const uint32_t cnt = out_of_flow ? (uint32_t)__builtin_ctzll(out_of_flow) : 64u;
                const bool active = lane < cnt;
                const uint32_t code = active ? cn::code_of(sk.iss, sk.rcv_wnd, cur.f) : 0u;
                const unsigned long long events = __ballot(active && cn::is_event(code));
                const uint32_t e = events ? (uint32_t)__builtin_ctzll(events) : cnt;  // the first event's lane, or none
                const bool mine = lane < e;  // (e <= cnt) the frames in front of the event
                n_rejected += (uint32_t)__popcll(__ballot(mine && cn::counts_rejected(code)));
                n_keepalive += (uint32_t)__popcll(__ballot(mine && code == recv::kKeepalive));
                if (mine && a.ctl_code && cur.frame < a.n) a.ctl_code[cur.frame] = (uint8_t)code;
                if (e < cnt) {  // the event, applied in all lanes alike; it ends the walk
                    const uint32_t ecode = lane_value(code, e), eframe = lane_value(cur.frame, e);
                    const cn::Seg ef{lane_value(cur.f.seq, e), lane_value(cur.f.ack, e), lane_value(cur.f.window, e),
                                     lane_value(cur.f.flags9, e), lane_value(cur.f.len, e)};
                    const uint32_t mss = ecode == recv::kTaken ? frame_mss(a, eframe, lane_value(cur.doff, e)) : 0u;
                    o = cn::apply(o, sk, ecode, ef, base + e, eframe, mss);
                    if (lane == e && (ecode == recv::kTaken || ecode == cn::kCodeBadAck) && a.ctl_code && cur.frame < a.n)
                        a.ctl_code[cur.frame] = (uint8_t)ecode;
                    done = true;
                } else {
                    o.stop = base + cnt;
                    done = cnt < 64u;
                }
                cur = next;
            }
            o.n_rejected = n_rejected, o.n_keepalive = n_keepalive;
        }
        o = cn::with_syn(o, sk);
        if (lane == 0) {
            a.openers_out[i] = o;
            if (o.reply != FS_CN_REPLY_NONE) {
                segment::SendRec rec;
                cn::reply_template(sk, o, rec.hdr);
                ctlframe::finish_rec(rec, i);
                a.reprec[i] = rec;
            }
        }
    }
}

// ---- The replies: the control-frame body over the openers whose record names a reply.
__global__ void __launch_bounds__(txdev::kThreads) connect_reply(const ctlframe::Args a, const fs_cn_out* openers_out) {
    ctlframe::build(a, reinterpret_cast<const uint8_t*>(openers_out) + offsetof(fs_cn_out, reply), sizeof(fs_cn_out));
}

}  // namespace

ConnectScratch connect_scratch(uint32_t n, uint32_t n_openers) {
    ConnectScratch s;
    uint64_t at = 0;
    s.sq = at, at += 16ull * n;
    s.reprec = at, at += (uint64_t)sizeof(segment::SendRec) * n_openers;
    s.flow_opener = at, at += 4ull * n;
    s.opener_first = at, at += 4ull * n_openers;
    s.bytes = at;
    return s;
}

hipError_t launch_connect(const RxBatch& b, const RxResults& r, const RxConnect& z, const RxLeft& left, const uint8_t* d_block,
                          const SegTables* tables, int tx_workgroups, const RxLaunch& how) {
    uint8_t* const scratch = left.connect_scratch;
    const ConnectScratch& s = left.cns;
    const uint32_t n = b.n;
    const hipStream_t stream = how.stream;
    CnArgs a;
    if (n != 0)
        static_cast<FlowView&>(a) = flow_view(left, n);
    else
        static_cast<FlowView&>(a) = FlowView{nullptr, nullptr, nullptr, nullptr, 0u};
    a.frames = b.frames;
    a.offsets = b.offsets;
    a.totals = static_cast<const fs_rx_flow_totals*>(r.totals());
    a.openers = reinterpret_cast<const fs_cn_sock*>(d_block);
    a.table = reinterpret_cast<const uint32_t*>(d_block + connect::block_of(z.n_openers).table);
    a.flow_opener = reinterpret_cast<uint32_t*>(scratch + s.flow_opener);
    a.opener_first = reinterpret_cast<uint32_t*>(scratch + s.opener_first);
    a.sq = reinterpret_cast<uint4*>(scratch + s.sq);
    a.reprec = reinterpret_cast<segment::SendRec*>(scratch + s.reprec);
    a.openers_out = z.openers_out;
    a.ctl_code = z.ctl_code;
    a.n = n;
    a.n_blocks = (uint32_t)(((uint64_t)n + kScanBlock - 1) / kScanBlock);
    a.n_openers = z.n_openers;
    a.tmask = flows::table_slots(z.n_openers) - 1u;
    a.hash_mask = how.hash_mask;
    const uint32_t cap = (uint32_t)(how.max_workgroups > 0 ? how.max_workgroups : 1);
    const uint32_t scan_grid = a.n_blocks < cap ? a.n_blocks : cap;
    const uint32_t walk_blocks = (z.n_openers + kWaves - 1u) / kWaves;
    const hipError_t e = hipMemsetAsync(a.opener_first, 0xFF, 4ull * z.n_openers, stream);
    if (e != hipSuccess) return e;
    if (n != 0) {
        hipLaunchKernelGGL(connect_mark, dim3(scan_grid), dim3(kThreads), 0, stream, a);
        hipLaunchKernelGGL(connect_gather, dim3(scan_grid), dim3(kThreads), 0, stream, a);
    }
    hipLaunchKernelGGL(connect_walk, dim3(walk_blocks < cap ? walk_blocks : cap), dim3(kThreads), 0, stream, a);
    const ctlframe::Args ra =
        ctlframe::args_of(a.reprec, z.n_openers, z.replies, z.reply_out, z.reply_status, tables, b.mtu, z.reply_flags);
    hipLaunchKernelGGL(connect_reply, dim3(ctlframe::grid_of(z.n_openers, tx_workgroups)), dim3(txdev::kThreads), 0, stream, ra,
                       z.openers_out);
    return hipGetLastError();
}

}  // namespace framesum
