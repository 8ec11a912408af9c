// The passive open of the accept call (fs_accept_flows_batch): behind the launches of the receive call
// (framesum_recv.hip), whose scratch of the same call these kernels read -- the sort keys (slot k's
// frame), the slot records (payload length, the flow heads), the key records, the flow numbers and,
// when sockets are listed, per flow its socket (`flow_sock`) -- give every first SYN to a listener one of
// the listener's free connections, in ascending order of flow number, and build its SYN-ACK
// (framesum_accept.h).
//
// The launches on the caller's stream, none of which waits on another workgroup or wave of its own
// launch, every loop bounded by a count known at its start:
//   (memset)  `conns` and `listeners_out` to 0, `accept_of` and the rank keys to all ones.
//   mark      one lane per slot that opens a flow: the candidate test on the flow's first frame, the
//             probe of the staged listener table (at most every table slot once); a candidate's rank
//             key listener << b | flow and its frame.
//   sort      rocprim::radix_sort_keys over the low b + index_bits(n_listeners) bits: every listener's
//             candidates lie together, in ascending flow order, in front of the all-ones entries.
//   assign    one lane per sorted position: a binary search for the listener's first position (at most
//             32 steps) gives the candidate's rank r with no atomic; r < n_slots fills slots[slot_first
//             + r] (the connection record, the SYN-ACK's record for the frame body), else FULL; the
//             listener's last candidate writes the listener's counts.
//   synack    one wave per slot, the control-frame body (framesum_ctlframe_dev.h: the TX frame build's body
//             over a piece source without payload): the 54 header bytes, both checksums, the FCS, the
//             digest and the verdict.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/framesum_accept.h"
#include "framesum_accept.h"
#include "framesum_coalesce.h"
#include "framesum_coalesce_dev.h"
#include "framesum_ctlframe_dev.h"
#include "framesum_flows.h"
#include "framesum_internal.h"
#include "framesum_segment.h"
#include "framesum_tx_dev.h"

namespace framesum {

namespace {

using namespace codev;
namespace ac = accept;

struct AcArgs : FlowView {  // (the flow launches' scratch of this call)
    const uint8_t* frames;
    const uint64_t* offsets;
    const uint32_t* flow_sock;  // the delivery launches' scratch of this call; null without sockets
    // the staged block
    const fs_listener* listeners;
    const uint32_t* table;
    const fs_accept_slot* slots;
    // this call's own scratch
    uint64_t* rank_in;          // per flow: the rank key, or all ones
    const uint64_t* rank_sorted;
    uint32_t* cand_frame;       // per candidate flow: its first frame
    segment::SendRec* synrec;   // per filled slot: the SYN-ACK as the frame body takes a record
    // the results
    fs_accept_conn* conns;
    fs_listener_out* listeners_out;
    uint32_t* accept_of;
    uint32_t n, n_blocks, n_socks, n_listeners, n_slots, tmask, hash_mask, lb;
};

__global__ void __launch_bounds__(kThreads) accept_mark(const AcArgs a) {
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t k = blk * kScanBlock + threadIdx.x;
        if (k >= a.n) continue;
        const uint2 r = a.rec[k];
        if (!(r.y & kAccepted) || !(r.y & flows::kFlowHead)) continue;
        const uint32_t f = a.flowidx[k];
        if (f >= a.n) continue;  // (the flow launches rule this out)
        if (a.flow_sock && a.flow_sock[f] < a.n_socks) continue;  // a listed socket has the flow
        const uint32_t frame = slot_frame(a, k);
        const uint4 v = a.keys[frame];
        const flows::Key key{{v.x, v.y, v.z, v.w}};
        if (flows::key_byte(key, 0) != 6u) continue;
        // an accepted TCP frame holds its whole TCP header (the verdict's gates)
        const uint8_t* __restrict__ p = a.frames + a.offsets[frame];
        const uint32_t l4 = 14u + 4u * (p[14] & 15u);
        if (!ac::first_syn(6u, ac::syn_of(p + l4), rec_len(r.x))) continue;
        const uint32_t l = ac::lookup_listener(ac::local_of_key(key), a.listeners, a.table, a.tmask, a.hash_mask);
        if (l >= a.n_listeners) continue;
        a.rank_in[f] = ac::rank_key(l, f, a.b);
        a.cand_frame[f] = frame;
    }
}

__global__ void __launch_bounds__(kThreads) accept_assign(const AcArgs a) {
    const uint64_t mask = ((uint64_t)1 << (a.b + a.lb)) - 1u;
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t pos = blk * kScanBlock + threadIdx.x;
        if (pos >= a.n) continue;
        const uint64_t rk = a.rank_sorted[pos];
        if (rk == ac::kNoCandidate) continue;
        const uint32_t l = (uint32_t)(rk >> a.b), f = ac::rank_flow(rk, a.b);
        if (l >= a.n_listeners || f >= a.n) continue;  // (mark writes no such key)
        const fs_listener lis = a.listeners[l];
        const uint32_t rank = pos - ac::lower_bound(a.rank_sorted, a.n, (uint64_t)l << a.b, mask);
        const uint64_t after = pos + 1u < a.n ? a.rank_sorted[pos + 1u] : ac::kNoCandidate;
        if (after == ac::kNoCandidate || (uint32_t)(after >> a.b) != l) {  // the listener's last candidate
            fs_listener_out o;
            o.n_syn = rank + 1u;
            o.n_accepted = o.n_syn < lis.n_slots ? o.n_syn : lis.n_slots;
            o.n_full = o.n_syn - o.n_accepted;
            o.reserved = 0;
            a.listeners_out[l] = o;
        }
        if (rank >= lis.n_slots) {
            if (a.accept_of) a.accept_of[f] = ac::kFull;
            continue;
        }
        const uint32_t slot = lis.slot_first + rank;
        if (slot >= a.n_slots) continue;  // (the host's checks rule this out)
        const uint32_t frame = a.cand_frame[f];
        if (frame >= a.n) continue;
        const uint4 v = a.keys[frame];
        const flows::Key key{{v.x, v.y, v.z, v.w}};
        const uint8_t* __restrict__ p = a.frames + a.offsets[frame];
        const uint32_t l4 = 14u + 4u * (p[14] & 15u);
        const ac::Syn syn = ac::syn_of(p + l4);
        // the options lie inside the frame: an accepted frame holds its whole TCP header
        const uint32_t n_opt = syn.doff > 5u ? 4u * (syn.doff - 5u) : 0u;
        const fs_accept_slot sl = a.slots[slot];
        const fs_accept_conn c = ac::conn_of(sl, key, p + 6, syn, ac::peer_mss(p + l4 + 20u, n_opt), frame, f);
        a.conns[slot] = c;
        segment::SendRec rec;
        ac::synack_template(lis, sl, c, rec.hdr);
        ctlframe::finish_rec(rec, slot);
        a.synrec[slot] = rec;
        if (a.accept_of) a.accept_of[f] = slot;
    }
}

// ---- The SYN-ACKs: the control-frame body (framesum_ctlframe_dev.h) over the filled slots.
__global__ void __launch_bounds__(txdev::kThreads) accept_synack(const ctlframe::Args a, const fs_accept_conn* conns) {
    ctlframe::build(a, reinterpret_cast<const uint8_t*>(conns) + offsetof(fs_accept_conn, used), sizeof(fs_accept_conn));
}

hipError_t sort_keys(void* temp, size_t& temp_bytes, uint64_t* in, uint64_t* out, uint32_t n, uint32_t bits,
                     hipStream_t stream) {
    return rocprim::radix_sort_keys(temp, temp_bytes, in, out, n, 0u, bits, stream);
}

}  // namespace

AcceptScratch accept_scratch(uint32_t n, uint32_t n_listeners, uint32_t n_slots) {
    AcceptScratch s;
    size_t sort_bytes = 0;
    // (a null pointer: the sort only reports what it needs)
    if (n != 0 && sort_keys(nullptr, sort_bytes, nullptr, nullptr, n, ac::rank_bits(flows::index_bits(n), n_listeners),
                            nullptr) != hipSuccess)
        sort_bytes = 0;
    uint64_t at = 0;
    s.rank_in = at, at += 8ull * n;
    s.rank_sorted = at, at += 8ull * n;
    s.synrec = at, at += (uint64_t)sizeof(segment::SendRec) * n_slots;
    s.cand_frame = at, at += 4ull * n;
    at = (at + 255u) & ~255ull;
    s.sort_temp = at, at += sort_bytes;
    s.sort_bytes = sort_bytes;
    s.bytes = at;
    return s;
}

hipError_t launch_accept(const RxBatch& b, const RxAccept& x, const RxLeft& left, const uint8_t* d_block,
                         const SegTables* tables, int tx_workgroups, const RxLaunch& how) {
    uint8_t* const scratch = left.accept_scratch;
    const AcceptScratch& s = left.acs;
    const uint32_t n = b.n;
    const hipStream_t stream = how.stream;
    const ac::Block blk = ac::block_of(x.n_listeners, x.n_slots);
    AcArgs a;
    static_cast<FlowView&>(a) = flow_view(left, n);
    a.frames = b.frames;
    a.offsets = b.offsets;
    a.flow_sock = left.deliver_scratch ? reinterpret_cast<const uint32_t*>(left.deliver_scratch + left.ds.flow_sock) : nullptr;
    a.listeners = reinterpret_cast<const fs_listener*>(d_block);
    a.table = reinterpret_cast<const uint32_t*>(d_block + blk.table);
    a.slots = reinterpret_cast<const fs_accept_slot*>(d_block + blk.slots);
    a.rank_in = reinterpret_cast<uint64_t*>(scratch + s.rank_in);
    a.rank_sorted = reinterpret_cast<const uint64_t*>(scratch + s.rank_sorted);
    a.cand_frame = reinterpret_cast<uint32_t*>(scratch + s.cand_frame);
    a.synrec = reinterpret_cast<segment::SendRec*>(scratch + s.synrec);
    a.conns = x.conns;
    a.listeners_out = x.listeners_out;
    a.accept_of = x.accept_of;
    a.n = n;
    const ScanGrid g = scan_grid(n, how);
    a.n_blocks = g.blocks;
    a.n_socks = x.n_socks;
    a.n_listeners = x.n_listeners;
    a.n_slots = x.n_slots;
    a.tmask = flows::table_slots(x.n_listeners) - 1u;
    a.hash_mask = how.hash_mask;
    a.lb = flows::index_bits(x.n_listeners);
    hipError_t e = hipMemsetAsync(a.rank_in, 0xFF, 8ull * n, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(accept_mark, dim3(g.scan), dim3(kThreads), 0, stream, a);
    size_t sort_bytes = s.sort_bytes;
    e = sort_keys(scratch + s.sort_temp, sort_bytes, a.rank_in, reinterpret_cast<uint64_t*>(scratch + s.rank_sorted), n,
                  ac::rank_bits(a.b, x.n_listeners), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(accept_assign, dim3(g.scan), dim3(kThreads), 0, stream, a);
    if (x.n_slots != 0) {
        const ctlframe::Args sa = ctlframe::args_of(a.synrec, x.n_slots, x.synacks, x.synack_out, x.synack_status, tables,
                                                    b.mtu, x.synack_flags);
        hipLaunchKernelGGL(accept_synack, dim3(ctlframe::grid_of(x.n_slots, tx_workgroups)), dim3(txdev::kThreads), 0, stream,
                           sa, x.conns);
    }
    return hipGetLastError();
}

}  // namespace framesum
