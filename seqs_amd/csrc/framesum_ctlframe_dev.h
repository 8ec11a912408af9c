// The 54-byte control frames of the RX calls -- the accept call's SYN-ACKs (framesum_accept.hip) and the
// connect call's replies (framesum_connect.hip) -- as one kernel body: the TX frame build's body
// (framesum_tx_dev.h) over a record without payload (mss 0: one frame of all its bytes, of which there
// are none). A kernel of either call is this body and nothing else. Included by those two files only.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/framesum_accept.h"
#include "framesum_segment.h"
#include "framesum_tx_dev.h"

namespace framesum {
namespace ctlframe {
namespace {

using Args = txdev::Args<segment::SendRec>;
struct NoPayload {
    using Rec = segment::SendRec;
    static constexpr bool kMayUdp = false, kMssZero = true;
    static __device__ __forceinline__ uint32_t total(const Rec*) { return 0u; }
    __device__ __forceinline__ NoPayload(const Args&, const Rec*, uint32_t, uint32_t) {}
    __device__ __forceinline__ void load(int, uint32_t d[4]) const { d[0] = d[1] = d[2] = d[3] = 0u; }
};

static_assert(!NoPayload::kMayUdp, "a control frame is TCP: the body has no protocol branch");

// One wave per slot s of [0, a.n_frames) whose byte used[s * stride] is not 0: the frame of a.recs[s] (its
// template's bytes 18, 19 carry the ID seed) at the record's frame_base, the digest and the verdict at
// entry s. A workgroup none of whose slots is used builds no tables (a batch without such a frame: all of
// them).
__device__ __forceinline__ void build(const Args& a, const uint8_t* used, uint32_t stride) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int mine = 0;
    for (uint32_t slot = blockIdx.x * txdev::kWaves + wave; slot < a.n_frames; slot += gridDim.x * txdev::kWaves)
        mine |= used[(uint64_t)slot * stride];
    if (!__syncthreads_or(mine)) return;
    txdev::load_tables(a.tables);
    // (a.n_frames: the slots; a used slot's frame is the slot's)
    for (uint32_t slot = blockIdx.x * txdev::kWaves + wave; slot < a.n_frames; slot += gridDim.x * txdev::kWaves) {
        if (__builtin_amdgcn_readfirstlane((uint32_t)used[(uint64_t)slot * stride]) == 0u) continue;
        const segment::SendRec* rec = a.recs + slot;
        const uint32_t seed = __builtin_amdgcn_readfirstlane(((uint32_t)rec->hdr[18] << 8) | rec->hdr[19]);
        txdev::build_frame<false, NoPayload>(a, rec, 0u, txdev::prand16(seed), slot, lane);
    }
}

// The launch arguments of such a kernel over n_slots records: frames at `frames` + the records'
// frame_base, `out` and `status` nullable.
inline Args args_of(const segment::SendRec* recs, uint32_t n_slots, uint8_t* frames, fs_digest* out, uint8_t* status,
                    const SegTables* tables, uint32_t mtu, uint32_t flags) {
    Args sa;
    sa.recs = recs;
    sa.prefix = nullptr;
    sa.ids = nullptr;
    sa.src = nullptr;
    sa.frames = frames;
    sa.offsets = nullptr;
    sa.lengths = nullptr;
    sa.out = reinterpret_cast<uint2*>(out);
    sa.status = status;
    sa.tables = tables;
    sa.n_recs = n_slots;
    sa.n_frames = n_slots;
    sa.tile = 1;
    sa.mtu = mtu;
    sa.flags = flags;
    sa.align = 1;
    return sa;
}
// The record of slot `slot` around a filled template: no payload, one frame at slot * FS_ACCEPT_STRIDE.
__host__ __device__ inline void finish_rec(segment::SendRec& rec, uint32_t slot) {
    rec.mss = 0;
    rec.payload_off = 0;
    rec.payload_len = 0;
    rec.frames = 1;
    rec.frame_base = (uint64_t)slot * FS_ACCEPT_STRIDE;
    rec.id_at = 0;
    rec.pad = 0;
}
inline uint32_t grid_of(uint32_t n_slots, int tx_workgroups) {
    const uint32_t want = (n_slots + txdev::kWaves - 1u) / txdev::kWaves;
    const uint32_t tx_cap = (uint32_t)(tx_workgroups > 0 ? tx_workgroups : 1);
    return want < tx_cap ? want : tx_cap;
}

}  // namespace
}  // namespace ctlframe
}  // namespace framesum
