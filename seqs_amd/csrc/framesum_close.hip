// The closing states and the RST of the close call (fs_close_flows_batch): behind the launches of the
// accept call (framesum_accept.hip), these kernels read what the flow launches left of the same call --
// the sort keys (slot k's frame), the slot records (payload length, the flow heads), the key records,
// the flow numbers -- and, when sockets are listed, what the delivery and the receive launches left: per
// socket its flow's first slot (`sock_first`), per slot of a listed socket's flow Seq and the payload
// length (`mk`), Ack and the dword at L4 + 12 (`aw`), and the two out records socks_out and snd_out.
// They walk every closer's flow, and every listed socket's flow from the receive call's `stop` on, under
// the rule of framesum_close.h.
//
// The launches on the caller's stream, none of which waits on another workgroup or wave of its own
// launch, every loop bounded by a count known at its start:
//   (memset)  `ctl_code` to 0, the closers' first slots to "none".
//   match     flow_match (framesum_match_dev.h) over the staged closer table: the flow's closer, the
//             closer's first slot.
//   gather    flow_gather_sq, which the connect call launches too: one lane per slot of a closer's flow:
//             Seq, Ack, the dword at L4 + 12 and the payload length into per-slot scratch, so that the
//             walk's loads are contiguous. (The slots of a listed
//             socket's flow need none: the delivery's mark and the receive call's gather have left all
//             four values for every slot of such a flow, also behind `stop`.)
//   walk      one wave per closer and one per listed socket: the flow's slots in chunks of 64, the next
//             chunk's loads in flight while this one is decided. Under a fixed (state, rcv.NXT) no
//             frame's code depends on another frame, so all lanes decide at once; the first lane whose
//             frame changes the state or rcv.NXT (an event) is found by ballot, the lanes up to it are
//             committed -- the counts are popcounts, snd.UNA and snd.WND come from the highest committed
//             lane that sets them -- the event is applied wave-uniformly, and the lanes behind it decide
//             again. Every pass retires at least one lane: at most 64 passes per chunk.
#include <hip/hip_runtime.h>

#include "../../include/framesum_close.h"
#include "framesum_close.h"
#include "framesum_coalesce.h"
#include "framesum_coalesce_dev.h"
#include "framesum_flows.h"
#include "framesum_internal.h"
#include "framesum_match_dev.h"

namespace framesum {

namespace {

using namespace codev;
namespace cl = closing;

// (the match's record in front: the owners are the closers)
struct ClArgs : FlowMatch<fs_cl_sock> {
    const uint8_t* frames;
    const uint64_t* offsets;
    const fs_rx_flow_totals* totals;
    // the delivery's and the receive launches' scratch and results of this call; null without sockets
    const uint2* mk;
    const uint2* aw;
    const uint32_t* sock_first;
    const fs_rx_sock_out* socks_out;
    const fs_rx_snd_out* snd_out;
    // the staged block, behind the closers and their table
    const cl::Fixed* socks;  // per listed socket
    // this call's own scratch
    const uint4* sq;  // per slot of a closer's flow: Seq, Ack, the dword at L4 + 12, the payload length
    // the results
    fs_cl_out* closers_out;
    fs_cl_out* socks_close;
    uint8_t* ctl_code;
    uint32_t n_socks;
};

// The gather of the close and of the connect call: one lane per slot of an owner's flow.
struct SqArgs : FlowView {
    const uint8_t* frames;
    const uint64_t* offsets;
    const uint32_t* flow_owner;
    uint4* sq;
    uint32_t n, n_blocks, n_owners;
};
__global__ void __launch_bounds__(kThreads) flow_gather_sq(const SqArgs a) {
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t k = blk * kScanBlock + threadIdx.x;
        if (k >= a.n) continue;
        const uint2 r = a.rec[k];
        if (!(r.y & kAccepted)) continue;
        const uint32_t f = a.flowidx[k];
        if (f >= a.n || a.flow_owner[f] >= a.n_owners) continue;
        // an accepted TCP frame holds its whole TCP header (the verdict's gates)
        const uint8_t* __restrict__ p = a.frames + a.offsets[slot_frame(a, k)];
        const uint32_t l4 = 14u + 4u * (p[14] & 15u);
        a.sq[k] = make_uint4(__builtin_bswap32(load_at<uint32_t>(p + l4 + 4u)), __builtin_bswap32(load_at<uint32_t>(p + l4 + 8u)),
                             load_at<uint32_t>(p + l4 + 12u), rec_len(r.x));
    }
}

// What a lane holds of its slot of a chunk: in the flow's walked part or not, the frame as the rule reads
// it, the slot's frame. The loads do not wait for each other (a slot outside the flow reads scratch it
// does not use). `from_sock`: the slot's values lie in the delivery's and the receive call's scratch.
struct Held {
    uint32_t in, frame;
    cl::Seg f;
};
__device__ __forceinline__ Held hold(const ClArgs& a, bool from_sock, uint32_t first, uint32_t k, uint32_t n_acc) {
    Held h{0u, 0u, cl::Seg{0u, 0u, 0u, 0u, 0u}};
    if (k < n_acc) {
        const uint32_t y = a.rec[k].y;
        uint4 q;
        if (from_sock) {
            const uint2 m = a.mk[k], w = a.aw[k];
            q = make_uint4(m.x, w.x, w.y, m.y & 0xFFFFu);
        } else {
            q = a.sq[k];
        }
        h.frame = slot_frame(a, k);
        h.in = (k == first || !(y & flows::kFlowHead)) ? 1u : 0u;
        h.f = seg_of(q);
    }
    return h;
}

__device__ __forceinline__ unsigned long long lanes_from_to(uint32_t lo, uint32_t hi) {  // lanes [lo, hi), hi <= 64
    const unsigned long long below_hi = hi >= 64u ? ~0ull : (1ull << hi) - 1ull;
    const unsigned long long below_lo = lo >= 64u ? ~0ull : (1ull << lo) - 1ull;
    return below_hi & ~below_lo;
}

// The walk's state between chunks, the same in all lanes.
struct Walk {
    cl::Ctl c;
    uint32_t n_taken, n_rejected, stop;
};

// One chunk of a walk: lane l holds slot base + l in `cur`. Returns true when the walk has ended (the flow's end
// lies in this chunk, or rule 2). Every value that steers the loop is the same in all lanes.
__device__ __forceinline__ bool walk_chunk(const ClArgs& a, const cl::Fixed& x, uint32_t base, uint32_t lane,
                                           const Held& cur, Walk& w) {
    const unsigned long long out_of_flow = __ballot(cur.in == 0u);
    const uint32_t cnt = out_of_flow ? (uint32_t)__builtin_ctzll(out_of_flow) : 64u;
    uint32_t done = 0;  // the lanes below `done` are retired
    bool ended = false;
    // every pass retires at least one lane
    for (uint32_t pass = 0; pass < 64u && done < cnt; ++pass) {
        const bool active = lane >= done && lane < cnt;
        const uint32_t code = active ? cl::code_of(w.c.state, w.c.nxt, x, cur.f) : 0u;
        const unsigned long long events = __ballot(active && cl::is_event(w.c.state, code, x, cur.f));
        const uint32_t e = events ? (uint32_t)__builtin_ctzll(events) : cnt;  // the first event's lane, or none
        // the lanes [done, e) change neither the state nor rcv.NXT
        const unsigned long long plain = lanes_from_to(done, e);
        const bool mine = ((plain >> lane) & 1ull) != 0ull;
        const unsigned long long taken = __ballot(mine && code == recv::kTaken);
        const unsigned long long acked = __ballot(mine && code == recv::kTaken && (cur.f.flags9 & cl::kAck) != 0u);
        w.n_taken += (uint32_t)__popcll(taken);
        w.n_rejected += (uint32_t)__popcll(__ballot(mine && cl::counts_rejected(code)));
        if (taken != 0ull) w.c.wnd = lane_value(cur.f.window, 63u - (uint32_t)__builtin_clzll(taken));
        if (acked != 0ull) w.c.una = lane_value(cur.f.ack, 63u - (uint32_t)__builtin_clzll(acked));
        if (mine && a.ctl_code && cur.frame < a.n) a.ctl_code[cur.frame] = (uint8_t)code;
        if (e >= cnt) {
            done = cnt;
            break;
        }
        // the event, applied in all lanes alike
        const uint32_t ecode = lane_value(code, e);
        if (ecode == cl::kEnds) {  // rule 2: the walk ends in front of this frame
            w.stop = base + e;
            ended = true;
            break;
        }
        const cl::Seg ef = lane_seg(cur.f, e);
        w.c = cl::step(w.c, ecode, x, ef);
        if (ecode == recv::kTaken) ++w.n_taken;
        if (lane == e && a.ctl_code && cur.frame < a.n) a.ctl_code[cur.frame] = (uint8_t)ecode;
        done = e + 1u;
    }
    if (!ended) {
        w.stop = base + done;
        ended = cnt < 64u;
    }
    return ended;
}

// The walk over the slots [begin, the flow's end) of the flow whose first slot is `first`.
__device__ __forceinline__ void walk_flow(const ClArgs& a, const cl::Fixed& x, bool from_sock, uint32_t first, uint32_t begin,
                                          uint32_t lane, Walk& w) {
    const uint32_t n_acc = a.totals->n_accepted < a.n ? a.totals->n_accepted : a.n;
    w.stop = begin;
    uint32_t base = begin;
    Held cur = hold(a, from_sock, first, base + lane, n_acc);
    bool done = false;
    // (at most the accepted slots from `base` on: ceil((n_acc - base) / 64) rounds)
    for (; base < n_acc && !done; base += 64u) {
        const Held next = hold(a, from_sock, first, base + 64u + lane, n_acc);
        done = walk_chunk(a, x, base, lane, cur, w);
        cur = next;
    }
}

__global__ void __launch_bounds__(kThreads) close_walk(const ClArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_walks = a.n_owners + a.n_socks;
    for (uint32_t i = blockIdx.x * kWaves + wave; i < n_walks; i += gridDim.x * kWaves) {
        if (i < a.n_owners) {
            const fs_cl_sock sk = a.recs[i];
            fs_cl_out o = cl::untouched_closer(sk);
            const uint32_t first = a.owner_first[i];
            if (first < a.n) {
                Walk w{cl::ctl_of(sk), 0u, 0u, first};
                walk_flow(a, cl::Fixed{sk.snd_nxt, sk.rcv_wnd}, false, first, first, lane, w);
                o = cl::out_of(w.c, w.n_taken, w.n_rejected, w.stop);
            }
            if (lane == 0) a.closers_out[i] = o;
            continue;
        }
        // an Established socket: where the receive call's walk ended
        const uint32_t s = i - a.n_owners;
        const cl::Fixed x = a.socks[s];
        const fs_rx_sock_out so = a.socks_out[s];
        const fs_rx_snd_out sn = a.snd_out[s];
        fs_cl_out o = cl::untouched_sock(so.rcv_nxt, sn.snd_una, sn.snd_wnd, so.stop);
        const uint32_t first = a.sock_first[s];
        if (first < a.n) {
            const uint32_t n_acc = a.totals->n_accepted < a.n ? a.totals->n_accepted : a.n;
            const uint32_t stop = so.stop;  // (first <= stop <= the accepted slots)
            Walk w{cl::Ctl{cl::kEstablished, so.rcv_nxt, sn.snd_una, sn.snd_wnd, 0u}, 0u, 0u, stop};
            if (stop < first || stop > n_acc) {
                // (the delivery rules this out)
            } else if (sn.flags & FS_RECV_FIN) {
                w.c.state = cl::kCloseWait;
                walk_flow(a, x, true, first, stop, lane, w);
                o = cl::out_of(w.c, w.n_taken, w.n_rejected, w.stop);
            } else if (stop < n_acc && (stop == first || !(a.rec[stop].y & flows::kFlowHead))) {  // the slot lies in the flow
                const Held h = hold(a, true, first, stop, n_acc);  // (the same slot in every lane)
                if ((h.f.flags9 & cl::kRst) && !(h.f.flags9 & cl::kSyn)) {
                    const uint32_t code = cl::code_of(cl::kEstablished, w.c.nxt, x, h.f);
                    if (lane == 0 && a.ctl_code && h.frame < a.n) a.ctl_code[h.frame] = (uint8_t)code;
                    w.stop = stop + 1u;
                    if (code == cl::kCodeRst) {
                        w.c = cl::step(w.c, code, x, h.f);
                        walk_flow(a, x, true, first, stop + 1u, lane, w);
                    } else {
                        w.n_rejected = 1u;
                    }
                    o = cl::out_of(w.c, w.n_taken, w.n_rejected, w.stop);
                }
            }
        }
        if (lane == 0) a.socks_close[s] = o;
    }
}

}  // namespace

OwnerScratch owner_scratch(uint32_t n, uint32_t n_owners) {
    OwnerScratch s;
    uint64_t at = 0;
    s.sq = at, at += 16ull * n;
    s.flow_owner = at, at += 4ull * n;
    s.owner_first = at, at += 4ull * n_owners;
    s.bytes = at;
    return s;
}

void launch_flow_gather_sq(const RxBatch& b, const RxLeft& left, uint8_t* scratch, const OwnerScratch& s, uint32_t n_owners,
                           const RxLaunch& how) {
    const ScanGrid g = scan_grid(b.n, how);
    SqArgs a;
    static_cast<FlowView&>(a) = flow_view(left, b.n);
    a.frames = b.frames;
    a.offsets = b.offsets;
    a.flow_owner = reinterpret_cast<const uint32_t*>(scratch + s.flow_owner);
    a.sq = reinterpret_cast<uint4*>(scratch + s.sq);
    a.n = b.n;
    a.n_blocks = g.blocks;
    a.n_owners = n_owners;
    hipLaunchKernelGGL(flow_gather_sq, dim3(g.scan), dim3(kThreads), 0, how.stream, a);
}

hipError_t launch_close(const RxBatch& b, const RxResults& r, const RxClose& y, const RxLeft& left, const uint8_t* d_block,
                        const RxLaunch& how) {
    uint8_t* const scratch = left.close_scratch;
    const OwnerScratch& s = left.cs;
    const uint32_t n = b.n;
    const hipStream_t stream = how.stream;
    const bool socks = y.n_socks != 0;
    const ScanGrid g = scan_grid(n, how);
    const closing::Block blk = closing::block_of(y.n_closers, y.n_socks);
    ClArgs a;
    fill_match(a, flow_view(left, n), d_block, blk.table, reinterpret_cast<uint32_t*>(scratch + s.flow_owner),
               reinterpret_cast<uint32_t*>(scratch + s.owner_first), n, y.n_closers, how);
    a.frames = b.frames;
    a.offsets = b.offsets;
    a.totals = static_cast<const fs_rx_flow_totals*>(r.totals());
    a.mk = socks ? reinterpret_cast<const uint2*>(left.deliver_scratch + left.ds.mk) : nullptr;
    a.aw = socks ? reinterpret_cast<const uint2*>(left.recv_scratch + left.rs.aw) : nullptr;
    a.sock_first = socks ? reinterpret_cast<const uint32_t*>(left.deliver_scratch + left.ds.sock_first) : nullptr;
    a.socks_out = r.socks_out();
    a.snd_out = r.snd_out();
    a.socks = reinterpret_cast<const cl::Fixed*>(d_block + blk.socks);
    a.sq = reinterpret_cast<const uint4*>(scratch + s.sq);
    a.closers_out = y.closers_out;
    a.socks_close = y.socks_close;
    a.ctl_code = y.ctl_code;
    a.n_socks = y.n_socks;
    const uint32_t walk_blocks = (y.n_closers + y.n_socks + kWaves - 1u) / kWaves;
    if (y.n_closers != 0) {
        const hipError_t e = hipMemsetAsync(a.owner_first, 0xFF, 4ull * y.n_closers, stream);
        if (e != hipSuccess) return e;
        if (n != 0) {
            hipLaunchKernelGGL(flow_match<fs_cl_sock>, dim3(g.scan), dim3(kThreads), 0, stream, a);
            launch_flow_gather_sq(b, left, scratch, s, y.n_closers, how);
        }
    }
    hipLaunchKernelGGL(close_walk, dim3(g.capped(walk_blocks)), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace framesum
