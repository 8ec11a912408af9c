// Device code the two RX coalesce kernel files share (framesum_coalesce.hip: fs_coalesce_batch;
// framesum_flows.hip: fs_coalesce_flows_batch): the workgroup scan, loads and stores at any
// alignment, a frame's header load and classification, the payload copy by 16 lanes, and the four
// gather steps -- classify, the scan of the partials, apply, copy -- written once over a mode that
// each file supplies, with the launch arguments and the scratch layout the two families have in
// common; and what the kernels behind the flow launches share (framesum_deliver.hip,
// framesum_recv.hip): their view of those launches' scratch. (framesum_tx_dev.h takes Piece, load_at
// and store_at from here.) HIP only; the
// arithmetic these call is in framesum_coalesce.h, which compiles without HIP.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/framesum.h"
#include "framesum_coalesce.h"
#include "framesum_flows.h"
#include "framesum_internal.h"

namespace framesum {
namespace codev {

using namespace coalesce;

constexpr int kThreads = (int)kScanBlock;  // one frame per lane in the scan kernels
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kGroup = 16;                       // lanes per frame in the copy kernel
constexpr uint32_t kTileFrames = kThreads / kGroup;   // frames a workgroup copies at a time

// The workgroup's scan of one P per lane: `incl` through the lane itself, `excl` without it,
// `total` the workgroup's. `lds`: kWaves Ps, free again when the call returns. P{} is the scan's
// zero; combine(P, P) and shfl_up_part(P, int) are found beside P.
template <typename P>
__device__ __forceinline__ void block_scan(P v, P* lds, P& incl, P& excl, P& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const P u = shfl_up_part(v, d);
        if (lane >= (uint32_t)d) v = combine(u, v);
    }
    P before = shfl_up_part(v, 1);
    if (lane == 0) before = P{};
    if (lane == 63) lds[wave] = v;
    __syncthreads();
    P pre = P{}, all = P{};
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const P p = lds[w];
        if ((uint32_t)w < wave) pre = combine(pre, p);
        all = combine(all, p);
    }
    __syncthreads();
    incl = combine(pre, v);
    excl = combine(pre, before);
    total = all;
}

struct __attribute__((packed)) Piece {  // 16 bytes at any alignment
    uint32_t d[4];
};
template <typename T>
__device__ __forceinline__ T load_at(const uint8_t* p) {  // any alignment
    T v;
    __builtin_memcpy(&v, p, sizeof v);
    return v;
}
template <typename T>
__device__ __forceinline__ void store_at(uint8_t* p, T v) {
    __builtin_memcpy(p, &v, sizeof v);
}

// Frame i's header and what the classify step keeps of it. A frame that is not accepted is not read.
// A: the kernel's arguments, of which this reads frames, offsets, lengths, status, n and fcs.
template <typename A>
__device__ __forceinline__ Info classify_frame(const A& a, uint32_t i, Hdr& h) {
#pragma unroll
    for (uint32_t k = 0; k < kHdrWords; ++k) h.w[k] = 0;
    if (i >= a.n || a.status[i] != FS_OK) return rejected();
    const uint8_t* __restrict__ p = a.frames + a.offsets[i];
    const uint32_t len = a.lengths[i];
    const uint32_t avail = len >= a.fcs ? len - a.fcs : 0u;
    if (avail >= kHdr) {
        const Piece p0 = *reinterpret_cast<const Piece*>(p), p1 = *reinterpret_cast<const Piece*>(p + 16),
                    p2 = *reinterpret_cast<const Piece*>(p + 32);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            h.w[k] = p0.d[k];
            h.w[4 + k] = p1.d[k];
            h.w[8 + k] = p2.d[k];
        }
        h.w[12] = load_at<uint32_t>(p + 48);
        h.w[13] = load_at<uint16_t>(p + 52);
    } else {
        h = load_hdr_bytes(p, avail);
    }
    uint32_t doff = byte_of(h, 46), flags = byte_of(h, 47);
    if (is_tcp(h) && ihl_of(h) != 5u) {  // IP options: the TCP header lies further on
        const uint32_t at = tcp_bytes_at(h);
        if (at + 1u >= avail) return rejected();  // (FS_OK rules this out)
        doff = p[at];
        flags = p[at + 1];
    }
    const Info f = payload_range(h, doff, flags);
    if (f.start > avail || f.len > avail - f.start) return rejected();  // (FS_OK rules this out too)
    return f;
}

// `len` bytes from src to dst by the 16 lanes of a group (sub = 0..15), any two alignments.
__device__ __forceinline__ void copy_payload(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t len,
                                             uint32_t sub) {
    const CopyPlan c = copy_plan((uint64_t)reinterpret_cast<uintptr_t>(dst), len);
    // the body: piece p is [head + 16 p, head + 16 p + 16), four pieces in flight per lane
    const uint8_t* __restrict__ bs = src + c.head;
    uint8_t* __restrict__ bd = dst + c.head;
    for (uint32_t p = sub; p < c.body; p += 4 * kGroup) {
        const bool b1 = p + kGroup < c.body, b2 = p + 2 * kGroup < c.body, b3 = p + 3 * kGroup < c.body;
        const size_t o0 = (size_t)p * 16u, o1 = o0 + 16u * kGroup, o2 = o0 + 32u * kGroup, o3 = o0 + 48u * kGroup;
        Piece v0, v1, v2, v3;
        v0 = *reinterpret_cast<const Piece*>(bs + o0);
        if (b1) v1 = *reinterpret_cast<const Piece*>(bs + o1);
        if (b2) v2 = *reinterpret_cast<const Piece*>(bs + o2);
        if (b3) v3 = *reinterpret_cast<const Piece*>(bs + o3);
        *reinterpret_cast<Piece*>(bd + o0) = v0;
        if (b1) *reinterpret_cast<Piece*>(bd + o1) = v1;
        if (b2) *reinterpret_cast<Piece*>(bd + o2) = v2;
        if (b3) *reinterpret_cast<Piece*>(bd + o3) = v3;
    }
    // the head: 1, 2, 4 and 8 bytes in this order (the set bits of head), lanes 0..3
    if (sub == 0 && (c.head & 1u)) dst[0] = src[0];
    if (sub == 1 && (c.head & 2u)) store_at<uint16_t>(dst + (c.head & 1u), load_at<uint16_t>(src + (c.head & 1u)));
    if (sub == 2 && (c.head & 4u)) store_at<uint32_t>(dst + (c.head & 3u), load_at<uint32_t>(src + (c.head & 3u)));
    if (sub == 3 && (c.head & 8u)) store_at<uint64_t>(dst + (c.head & 7u), load_at<uint64_t>(src + (c.head & 7u)));
    // the tail: 8, 4, 2 and 1 bytes in this order, lanes 4..7
    const size_t t0 = (size_t)c.head + (size_t)c.body * 16u;
    if (sub == 4 && (c.tail & 8u)) store_at<uint64_t>(dst + t0, load_at<uint64_t>(src + t0));
    if (sub == 5 && (c.tail & 4u)) store_at<uint32_t>(dst + t0 + (c.tail & 8u), load_at<uint32_t>(src + t0 + (c.tail & 8u)));
    if (sub == 6 && (c.tail & 2u)) store_at<uint16_t>(dst + t0 + (c.tail & 12u), load_at<uint16_t>(src + t0 + (c.tail & 12u)));
    if (sub == 7 && (c.tail & 1u)) dst[t0 + (c.tail & 14u)] = src[t0 + (c.tail & 14u)];
}

// ---- The gather steps. Slot k of the scans and the copy stands for one frame; a run is a row of
// slots whose frames continue each other. A mode M says which frame, and what else is kept:
//   M::Part               the record the scans carry: sum (payload bytes), heads and hidx1 (run heads
//                         and the last one's slot + 1; 0: none yet), and what the mode adds; P{} is
//                         the zero, combine() and shfl_up_part() stand beside it
//   M::part(len, head, fhead, acc, k)   slot k's
//   M::Key, M::key(a, k), M::shfl_up_key(key)   what a slot knows beside its number: slot k's, read
//                         from memory (k < a.n), and the lane before's; Key{} where there is no slot
//   M::frame(a, k, key)   the frame slot k < a.n stands for
//   M::write_totals(a, carry)           the call's totals from the scan's grand total
//   M::kFlowBit           the bit of the slot record's y that says the slot opens a flow, and so a
//                         run; 0: the mode has no flows and none of the following
//   M::flow_head(a, k, acc, pacc, key, pkey)    does slot k open a flow?
//   M::apply_extra(a, k, i, in, acc)    what apply writes per slot beside payoff, runidx, hidx, run_of
//   M::flow_record(a, k, ny, off, len)  copy: lane 9 of slot k, ny = the next slot's y (0: none)
// A: the kernel's arguments (fill_gather_args below names the fields these read).

// One lane per slot: the slot record and the workgroup's partial.
template <typename M, typename A>
__device__ __forceinline__ void gather_classify(const A& a) {
    using P = typename M::Part;
    __shared__ P s_part[kWaves];
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t k = blk * kScanBlock + threadIdx.x;
        const typename M::Key key = k < a.n ? M::key(a, k) : typename M::Key{};
        const uint32_t i = k < a.n ? M::frame(a, k, key) : a.n;
        Hdr h, ph;
        const Info f = classify_frame(a, i, h);
        // the slot before: from the lane before, which has just classified it
        Info pf;
#pragma unroll
        for (uint32_t w = 0; w < kHdrWords; ++w) ph.w[w] = __shfl_up(h.w[w], 1, 64);
        const uint32_t packed = pack_info(f), bits = (f.accepted ? 1u : 0u) | (f.plain_tcp ? 2u : 0u);
        const uint32_t ppacked = __shfl_up(packed, 1, 64), pbits = __shfl_up(bits, 1, 64);
        typename M::Key pkey = M::shfl_up_key(key);
        pf.start = rec_start(ppacked);
        pf.len = rec_len(ppacked);
        pf.tcp_flags = rec_flags(ppacked);
        pf.accepted = (pbits & 1u) != 0;
        pf.plain_tcp = (pbits & 2u) != 0;
        if (lane == 0) {  // ... except for a wave's first lane, which reads it itself
            if (k > 0 && k < a.n) {
                pkey = M::key(a, k - 1u);
                pf = classify_frame(a, M::frame(a, k - 1u, pkey), ph);
            } else {
                pf = rejected();
            }
        }
        bool fhead = false;
        if constexpr (M::kFlowBit != 0) fhead = M::flow_head(a, k, f.accepted, pf.accepted, key, pkey);
        const bool head = f.accepted && (fhead || !joins(ph, pf, h, f));
        if (k < a.n)
            a.rec[k] = make_uint2(packed, (f.accepted ? kAccepted : 0u) | (head ? kHead : 0u) | (fhead ? M::kFlowBit : 0u));
        P incl, excl, total;
        block_scan(M::part(f.accepted ? (uint64_t)f.len : 0ull, head, fhead, f.accepted, k), s_part, incl, excl, total);
        if (threadIdx.x == 0) a.partial[blk] = total;
    }
}

// One workgroup: prefix[b] = the partials of the workgroups before b; the totals.
template <typename M, typename A>
__device__ __forceinline__ void gather_scan_partials(const A& a) {
    using P = typename M::Part;
    __shared__ P s_part[kWaves];
    P carry = P{};
    for (uint32_t base = 0; base < a.n_blocks; base += kScanBlock) {
        const uint32_t b = base + threadIdx.x;
        P incl, excl, total;
        block_scan(b < a.n_blocks ? a.partial[b] : P{}, s_part, incl, excl, total);
        if (b < a.n_blocks) a.prefix[b] = combine(carry, excl);
        carry = combine(carry, total);
    }
    if (threadIdx.x == 0) {
        M::write_totals(a, carry);
        *a.copied = carry.sum <= a.cap ? carry.sum : 0ull;
    }
}

// The same workgroups as classify scan their records from their prefix: per slot its packed
// position (64-bit), its run's index and its run's head (a max-scan of head slots).
template <typename M, typename A>
__device__ __forceinline__ void gather_apply(const A& a) {
    using P = typename M::Part;
    __shared__ P s_part[kWaves];
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t k = blk * kScanBlock + threadIdx.x;
        const uint2 r = k < a.n ? a.rec[k] : make_uint2(0u, 0u);
        const bool acc = (r.y & kAccepted) != 0, head = (r.y & kHead) != 0, fhead = (r.y & M::kFlowBit) != 0;
        const uint32_t len = acc ? rec_len(r.x) : 0u;
        P incl, excl, total;
        block_scan(M::part((uint64_t)len, head, fhead, acc, k), s_part, incl, excl, total);
        const P base = a.prefix[blk];
        const P in = combine(base, incl);
        const uint64_t off = base.sum + excl.sum;
        if (k < a.n) {
            const uint32_t i = M::frame(a, k, M::key(a, k));
            const uint32_t run = acc ? in.heads - 1u : kNoRun;
            a.payoff[k] = off;
            a.runidx[k] = run;
            a.hidx[k] = acc ? in.hidx1 - 1u : kNoRun;
            if constexpr (M::kFlowBit != 0) M::apply_extra(a, k, i, in, acc);
            if (a.run_of && i < a.n) a.run_of[i] = run;
        }
        // how far the packed buffer gets written when payload_cap cuts it short (the scan of the
        // partials has set `copied` to the total when everything fits, else to 0): the end of the
        // last frame below the cap. Only then do the waves meet at this one address.
        if (a.totals->payload_bytes > a.cap) {
            unsigned long long end = (acc && off + len <= a.cap) ? off + len : 0ull;
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) {
                const uint32_t lo = __shfl_xor((uint32_t)end, m, 64), hi = __shfl_xor((uint32_t)(end >> 32), m, 64);
                const unsigned long long o = ((unsigned long long)hi << 32) | lo;
                end = o > end ? o : end;
            }
            if ((threadIdx.x & 63u) == 0 && end != 0ull) atomicMax(a.copied, end);
        }
    }
}

// The hot path: 16 lanes per slot. The destination advances with the slots; the source is wherever
// the slot's frame lies. The last slot of a run writes the run's record, behind its copy.
template <typename M, typename A>
__device__ __forceinline__ void gather_copy(const A& a) {
    const uint32_t sub = threadIdx.x & (kGroup - 1u), grp = threadIdx.x / kGroup;
    const uint32_t n_tiles = (a.n + kTileFrames - 1u) / kTileFrames;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t k = tile * kTileFrames + grp;
        if (k >= a.n) continue;
        const uint2 r = a.rec[k];  // (loads that do not wait for the verdict: one latency, not two)
        const uint64_t off = a.payoff[k];
        const uint64_t at = a.offsets[M::frame(a, k, M::key(a, k))];
        if (!(r.y & kAccepted)) continue;
        const uint32_t len = rec_len(r.x);
        if (len != 0 && off + len <= a.cap) copy_payload(a.payload + off, a.frames + at + rec_start(r.x), len, sub);
        if (sub == 8 || (M::kFlowBit != 0 && sub == 9)) {
            const uint32_t ny = k + 1u == a.n ? 0u : a.rec[k + 1u].y;
            // a run ends where the next slot does not continue it (a continuing slot is accepted and
            // no head of a run or a flow); its last slot writes the record
            if (sub == 8 && ny != kAccepted) {
                const uint32_t hd = a.hidx[k];
                const uint64_t hoff = a.payoff[hd];
                fs_rx_run run;
                run.payload_off = hoff;
                run.payload_len = (uint32_t)(off + len - hoff);
                run.first_frame = hd;
                run.n_frames = k - hd + 1u;
                run.tcp_flags = (uint8_t)run_flags(rec_flags(a.rec[hd].x), rec_flags(r.x));
                run.reserved[0] = run.reserved[1] = run.reserved[2] = 0;
                a.runs[a.runidx[k]] = run;
            }
            if constexpr (M::kFlowBit != 0)
                if (sub == 9) M::flow_record(a, k, ny, off, len);
        }
    }
}

// ---- The host side both families share. The fields of the kernel arguments the gather steps read
// (`totals` and what a mode adds are the caller's), and the grids: `scan` for the kernels with one
// lane per frame, `copy` for the copy, neither above max_workgroups.
struct GatherGrids {
    uint32_t scan, copy;
};
// The same for any launch of a call over n slots: `blocks` blocks of kScanBlock slots (a kernel's
// n_blocks) run by `scan` workgroups; capped(want) for a kernel that wants another count.
struct ScanGrid {
    uint32_t blocks, scan, cap;
    uint32_t capped(uint32_t want) const { return want < cap ? want : cap; }
};
inline ScanGrid scan_grid(uint32_t n, const RxLaunch& how) {
    const uint32_t blocks = (uint32_t)(((uint64_t)n + kScanBlock - 1) / kScanBlock);
    const uint32_t cap = (uint32_t)(how.max_workgroups > 0 ? how.max_workgroups : 1);
    return ScanGrid{blocks, blocks < cap ? blocks : cap, cap};
}
template <typename A, typename S>
GatherGrids fill_gather_args(A& a, const RxBatch& b, const RxResults& r, uint8_t* scratch, const S& s, int max_workgroups) {
    const uint32_t n = b.n;
    a.frames = b.frames;
    a.offsets = b.offsets;
    a.lengths = b.lengths;
    a.status = r.status;
    a.rec = reinterpret_cast<uint2*>(scratch + s.rec);
    a.payoff = reinterpret_cast<uint64_t*>(scratch + s.payoff);
    a.partial = reinterpret_cast<decltype(a.partial)>(scratch + s.partial);
    a.prefix = reinterpret_cast<decltype(a.prefix)>(scratch + s.prefix);
    a.copied = reinterpret_cast<unsigned long long*>(scratch + s.copied);
    a.runidx = reinterpret_cast<uint32_t*>(scratch + s.runidx);
    a.hidx = reinterpret_cast<uint32_t*>(scratch + s.hidx);
    a.payload = r.payload;
    a.cap = r.payload_cap;
    a.runs = r.runs();
    a.run_of = r.run_of();
    a.n = n;
    a.n_blocks = (uint32_t)(((uint64_t)n + kScanBlock - 1) / kScanBlock);
    a.fcs = (b.flags & FS_RX_FCS) ? 4u : 0u;
    const uint32_t cap = (uint32_t)(max_workgroups > 0 ? max_workgroups : 1);
    const uint32_t n_tiles = (uint32_t)(((uint64_t)n + kTileFrames - 1) / kTileFrames);
    return GatherGrids{a.n_blocks < cap ? a.n_blocks : cap, n_tiles < cap ? n_tiles : cap};
}

// The scratch of the gather steps from offset `at` on, in two rows (the flow family keeps its table
// between them): the records, positions, partials of `part_bytes` each and `copied`; the run words.
// Each returns the offset behind its row.
template <typename S>
uint64_t lay_scan_arrays(S& s, uint64_t at, uint64_t n, uint64_t part_bytes) {
    const uint64_t nb = (n + kScanBlock - 1) / kScanBlock;
    s.rec = at, at += 8ull * n;
    s.payoff = at, at += 8ull * n;
    s.partial = at, at += part_bytes * nb;
    s.prefix = at, at += part_bytes * nb;
    s.copied = at, at += 8;
    return at;
}
template <typename S>
uint64_t lay_run_arrays(S& s, uint64_t at, uint64_t n) {
    s.runidx = at, at += 4ull * n;
    s.hidx = at, at += 4ull * n;
    return at;
}

// ---- What the kernels behind the flow launches share (framesum_deliver.hip, framesum_recv.hip): the
// view of what those launches left in their scratch of the same call. Their argument structs derive
// from it.
struct FlowView {
    const uint64_t* sorted;   // per slot: the sort key, whose low b bits are the frame
    const uint2* rec;         // per slot
    const uint4* keys;        // per frame
    const uint32_t* flowidx;  // per slot
    uint32_t b;
};
inline FlowView flow_view(const RxLeft& left, uint32_t n) {
    return FlowView{reinterpret_cast<const uint64_t*>(left.flow_scratch + left.fs.sorted),
                    reinterpret_cast<const uint2*>(left.flow_scratch + left.fs.rec),
                    reinterpret_cast<const uint4*>(left.flow_scratch + left.fs.keys),
                    reinterpret_cast<const uint32_t*>(left.flow_scratch + left.fs.flowidx), flows::index_bits(n)};
}
__device__ __forceinline__ uint32_t slot_frame(const FlowView& v, uint32_t k) { return flows::sort_index(v.sorted[k], v.b); }
// Lane `l`'s value, l the same in all lanes.
__device__ __forceinline__ uint32_t lane_value(uint32_t v, uint32_t l) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane((int)l));
}

}  // namespace codev
}  // namespace framesum
