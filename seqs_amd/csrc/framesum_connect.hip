// The active open of the connect call (fs_connect_flows_batch): behind the launches of the close call
// (framesum_close.hip), these kernels read what the flow launches left of the same call -- the sort keys
// (slot k's frame), the slot records (payload length, the flow heads), the key records, the flow numbers
// -- walk every opener's flow under the rule of framesum_connect.h and build the control frame each
// opener owes.
//
// The launches on the caller's stream, none of which waits on another workgroup or wave of its own
// launch, every loop bounded by a count known at its start:
//   (memset)  the openers' first slots to "none".
//   match     flow_match (framesum_match_dev.h) over the staged opener table: the flow's opener, the
//             opener's first slot.
//   gather    the close call's flow_gather_sq (framesum_close.hip) over the openers' flows: Seq, Ack, the
//             dword at L4 + 12 and the payload length per slot. (The input of the MSS option
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
#include "framesum_match_dev.h"

namespace framesum {

namespace {

using namespace codev;
namespace cn = connect;

// (the match's record in front: the owners are the openers)
struct CnArgs : FlowMatch<fs_cn_sock> {
    const uint8_t* frames;
    const uint64_t* offsets;
    const fs_rx_flow_totals* totals;
    // this call's own scratch
    const uint4* sq;           // per slot of an opener's flow: Seq, Ack, the dword at L4 + 12, the payload length
    segment::SendRec* reprec;  // per opener with a reply: the reply as the frame body takes a record
    // the results
    fs_cn_out* openers_out;
    uint8_t* ctl_code;
};

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
        h.f = seg_of(q);
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
    for (uint32_t i = blockIdx.x * kWaves + wave; i < a.n_owners; i += gridDim.x * kWaves) {
        const fs_cn_sock sk = a.recs[i];
        fs_cn_out o = cn::untouched(sk);
        const uint32_t first = a.owner_first[i];
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
                    const cn::Seg ef = lane_seg(cur.f, e);
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
    static_cast<OwnerScratch&>(s) = owner_scratch(n, n_openers);
    s.reprec = (s.bytes + 7u) & ~7ull;
    s.bytes = s.reprec + (uint64_t)sizeof(segment::SendRec) * n_openers;
    return s;
}

hipError_t launch_connect(const RxBatch& b, const RxResults& r, const RxConnect& z, const RxLeft& left, const uint8_t* d_block,
                          const SegTables* tables, int tx_workgroups, const RxLaunch& how) {
    uint8_t* const scratch = left.connect_scratch;
    const ConnectScratch& s = left.cns;
    const uint32_t n = b.n;
    const hipStream_t stream = how.stream;
    const ScanGrid g = scan_grid(n, how);
    CnArgs a;
    fill_match(a, n != 0 ? flow_view(left, n) : FlowView{nullptr, nullptr, nullptr, nullptr, 0u}, d_block,
               connect::block_of(z.n_openers).table, reinterpret_cast<uint32_t*>(scratch + s.flow_owner),
               reinterpret_cast<uint32_t*>(scratch + s.owner_first), n, z.n_openers, how);
    a.frames = b.frames;
    a.offsets = b.offsets;
    a.totals = static_cast<const fs_rx_flow_totals*>(r.totals());
    a.sq = reinterpret_cast<const uint4*>(scratch + s.sq);
    a.reprec = reinterpret_cast<segment::SendRec*>(scratch + s.reprec);
    a.openers_out = z.openers_out;
    a.ctl_code = z.ctl_code;
    const uint32_t walk_blocks = (z.n_openers + kWaves - 1u) / kWaves;
    const hipError_t e = hipMemsetAsync(a.owner_first, 0xFF, 4ull * z.n_openers, stream);
    if (e != hipSuccess) return e;
    if (n != 0) {
        hipLaunchKernelGGL(flow_match<fs_cn_sock>, dim3(g.scan), dim3(kThreads), 0, stream, a);
        launch_flow_gather_sq(b, left, scratch, s, z.n_openers, how);
    }
    hipLaunchKernelGGL(connect_walk, dim3(g.capped(walk_blocks)), dim3(kThreads), 0, stream, a);
    const ctlframe::Args ra =
        ctlframe::args_of(a.reprec, z.n_openers, z.replies, z.reply_out, z.reply_status, tables, b.mtu, z.reply_flags);
    hipLaunchKernelGGL(connect_reply, dim3(ctlframe::grid_of(z.n_openers, tx_workgroups)), dim3(txdev::kThreads), 0, stream, ra,
                       z.openers_out);
    return hipGetLastError();
}

}  // namespace framesum
