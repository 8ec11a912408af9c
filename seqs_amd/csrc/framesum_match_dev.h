// Device code the kernels behind the flow launches share for their connection lists (framesum_deliver.hip:
// the listed sockets; framesum_close.hip: the closers; framesum_connect.hip: the openers): the match of
// every flow's head against a list's staged keyed table (framesum_flows.h), written once over the record
// type; and what the close and the connect call share beyond it -- the scratch the match and the gather
// (flow_gather_sq, framesum_close.hip) fill, and how a walk reads an entry of it. HIP only.
#pragma once
#include <hip/hip_runtime.h>

#include "framesum_close.h"
#include "framesum_coalesce_dev.h"
#include "framesum_flows.h"
#include "framesum_internal.h"

namespace framesum {
namespace codev {

// What the match reads and writes, the flow launches' scratch of this call in front. A record of the
// list is an "owner": a flow has at most one, and (distinct keys on both sides) an owner at most one
// flow. The argument structs of the three calls' kernels derive from it.
template <class Rec>
struct FlowMatch : FlowView {
    // the staged block
    const Rec* recs;
    const uint32_t* table;
    // the call's own scratch
    uint32_t* flow_owner;   // per flow: its owner, or none
    uint32_t* owner_first;  // per owner: its flow's first slot, or none
    uint32_t n, n_blocks, n_owners, tmask, hash_mask;
};
// `d_block`: the staged block, the records at its start and their table at `table_at`.
template <class Rec>
void fill_match(FlowMatch<Rec>& m, const FlowView& v, const uint8_t* d_block, uint64_t table_at, uint32_t* flow_owner,
                uint32_t* owner_first, uint32_t n, uint32_t n_owners, const RxLaunch& how) {
    static_cast<FlowView&>(m) = v;
    m.recs = reinterpret_cast<const Rec*>(d_block);
    m.table = reinterpret_cast<const uint32_t*>(d_block + table_at);
    m.flow_owner = flow_owner;
    m.owner_first = owner_first;
    m.n = n;
    m.n_blocks = scan_grid(n, how).blocks;
    m.n_owners = n_owners;
    m.tmask = flows::table_slots(n_owners) - 1u;
    m.hash_mask = how.hash_mask;
}

// One lane per slot that opens a flow: the probe of the staged table with the key record of the slot's
// frame (at most every table slot once); the flow's owner, the owner's first slot.
template <class Rec>
__global__ void __launch_bounds__(kThreads) flow_match(const FlowMatch<Rec> m) {
    for (uint32_t blk = blockIdx.x; blk < m.n_blocks; blk += gridDim.x) {
        const uint32_t k = blk * kScanBlock + threadIdx.x;
        if (k >= m.n) continue;
        const uint32_t y = m.rec[k].y;
        if (!(y & kAccepted) || !(y & flows::kFlowHead)) continue;
        const uint32_t f = m.flowidx[k];
        if (f >= m.n) continue;  // (the flow launches rule this out)
        const uint4 v = m.keys[slot_frame(m, k)];
        const flows::Key key{{v.x, v.y, v.z, v.w}};
        uint32_t o = flows::kEmpty;
        if (flows::key_byte(key, 0) == 6u) o = flows::lookup(key, m.recs, m.table, m.tmask, m.hash_mask);
        m.flow_owner[f] = o;
        if (o < m.n_owners) m.owner_first[o] = k;
    }
}

// ---- The walks of the close and the connect call. An entry of `sq` (OwnerScratch, framesum_internal.h:
// Seq, Ack, the dword at L4 + 12, the payload length) as the rules read a frame (flags9_of and window_of:
// framesum_recv.h).
__device__ __forceinline__ closing::Seg seg_of(const uint4& q) {
    return closing::Seg{q.x, q.y, recv::window_of(q.z), recv::flags9_of(q.z), q.w};
}
// Lane `l`'s frame, l the same in all lanes.
__device__ __forceinline__ closing::Seg lane_seg(const closing::Seg& f, uint32_t l) {
    return closing::Seg{lane_value(f.seq, l), lane_value(f.ack, l), lane_value(f.window, l), lane_value(f.flags9, l),
                        lane_value(f.len, l)};
}

}  // namespace codev
}  // namespace framesum
