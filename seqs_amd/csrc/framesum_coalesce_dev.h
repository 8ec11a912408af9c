// Device code the two RX coalesce kernels files share (framesum_coalesce.hip: fs_coalesce_batch;
// framesum_flows.hip: fs_coalesce_flows_batch): the workgroup scan, loads and stores at any
// alignment, a frame's header load and classification, and the payload copy by 16 lanes. HIP only;
// the arithmetic these call is in framesum_coalesce.h, which compiles without HIP.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/framesum.h"
#include "framesum_coalesce.h"

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

}  // namespace codev
}  // namespace framesum
