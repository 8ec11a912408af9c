// RX coalesce (fs_coalesce_batch): behind the digest launch, gather the payload of every accepted
// frame into one packed buffer and report the runs of TCP segments that continue each other.
//
// Four launches on the caller's stream, none of which waits on another workgroup of its own launch:
//   classify  one lane per frame: the verdict, the frame's first 54 bytes (at any alignment), the
//             payload range and the join flag against the frame before it (the lanes of a wave pass
//             their header to the next lane; a wave's first lane reads frame i - 1 itself). Leaves an
//             8-byte record per frame and, per workgroup of kScanBlock frames, the partial (payload
//             bytes of its accepted frames, its run heads, its last head's index).
//   partials  one workgroup scans the partials into exclusive prefixes and writes the totals.
//   apply     the same workgroups as classify scan their records from their prefix: per frame its
//             packed position (64-bit), its run index and its run's head (a max-scan of head indices).
//   copy      the hot path: 16 lanes per frame. The last frame of a run writes the run's record from
//             its head's position; every accepted frame's payload moves to its packed position as
//             16-byte pieces stored at 16-byte boundaries of the destination and loaded at whatever
//             alignment the source has (gfx950 serves global accesses at any byte address), the 0..15
//             bytes in front of the first boundary and behind the last as one 1-, 2-, 4- and 8-byte
//             access each. Exactly the payload's bytes are read and exactly its destination written.
#include <hip/hip_runtime.h>

#include "../../include/framesum.h"
#include "framesum_coalesce.h"
#include "framesum_coalesce_dev.h"
#include "framesum_internal.h"

namespace framesum {

namespace {

using namespace codev;  // the scan, the header load and the copy shared with framesum_flows.hip

static_assert(sizeof(fs_rx_run) == 24 && sizeof(fs_rx_totals) == 16, "fs_rx_run / fs_rx_totals layout");

// What the scans carry: payload bytes, run heads, and the last head's frame index + 1 (0: none yet).
struct Part {
    uint64_t sum;
    uint32_t heads;
    uint32_t hidx1;
};
static_assert(sizeof(Part) == 16, "Part layout");

struct CoArgs {
    const uint8_t* frames;
    const uint64_t* offsets;
    const uint32_t* lengths;
    const uint8_t* status;
    uint2* rec;
    uint64_t* payoff;
    Part* partial;
    Part* prefix;
    unsigned long long* copied;
    uint32_t* runidx;
    uint32_t* hidx;
    uint8_t* payload;
    uint64_t cap;
    fs_rx_run* runs;
    uint32_t* run_of;
    fs_rx_totals* totals;
    uint32_t n, n_blocks, fcs;
};

__device__ __forceinline__ Part zero_part() { return Part{0ull, 0u, 0u}; }
__device__ __forceinline__ Part combine(const Part& a, const Part& b) {
    return Part{a.sum + b.sum, a.heads + b.heads, a.hidx1 > b.hidx1 ? a.hidx1 : b.hidx1};
}
__device__ __forceinline__ Part shfl_up_part(const Part& v, int d) {
    Part u;
    const uint32_t lo = __shfl_up((uint32_t)v.sum, d, 64), hi = __shfl_up((uint32_t)(v.sum >> 32), d, 64);
    u.sum = ((uint64_t)hi << 32) | lo;
    u.heads = __shfl_up(v.heads, d, 64);
    u.hidx1 = __shfl_up(v.hidx1, d, 64);
    return u;
}

__global__ void __launch_bounds__(kThreads) coalesce_classify(const CoArgs a) {
    __shared__ Part s_part[kWaves];
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t i = blk * kScanBlock + threadIdx.x;
        Hdr h, ph;
        const Info f = classify_frame(a, i, h);
        // the frame before: from the lane before, which has just classified it
        Info pf;
#pragma unroll
        for (uint32_t k = 0; k < kHdrWords; ++k) ph.w[k] = __shfl_up(h.w[k], 1, 64);
        const uint32_t packed = pack_info(f), bits = (f.accepted ? 1u : 0u) | (f.plain_tcp ? 2u : 0u);
        const uint32_t ppacked = __shfl_up(packed, 1, 64), pbits = __shfl_up(bits, 1, 64);
        pf.start = rec_start(ppacked);
        pf.len = rec_len(ppacked);
        pf.tcp_flags = rec_flags(ppacked);
        pf.accepted = (pbits & 1u) != 0;
        pf.plain_tcp = (pbits & 2u) != 0;
        if (lane == 0) {  // ... except for a wave's first lane, which reads it itself
            if (i > 0 && i < a.n) pf = classify_frame(a, i - 1, ph);
            else pf = rejected();
        }
        const bool head = f.accepted && !joins(ph, pf, h, f);
        if (i < a.n) a.rec[i] = make_uint2(packed, (f.accepted ? kAccepted : 0u) | (head ? kHead : 0u));
        Part incl, excl, total;
        block_scan(Part{f.accepted ? (uint64_t)f.len : 0ull, head ? 1u : 0u, head ? i + 1u : 0u}, s_part, incl, excl, total);
        if (threadIdx.x == 0) a.partial[blk] = total;
    }
}

// One workgroup: prefix[b] = the partials of the workgroups before b; the totals.
__global__ void __launch_bounds__(kThreads) coalesce_scan_partials(const CoArgs a) {
    __shared__ Part s_part[kWaves];
    Part carry = zero_part();
    for (uint32_t base = 0; base < a.n_blocks; base += kScanBlock) {
        const uint32_t b = base + threadIdx.x;
        Part incl, excl, total;
        block_scan(b < a.n_blocks ? a.partial[b] : zero_part(), s_part, incl, excl, total);
        if (b < a.n_blocks) a.prefix[b] = combine(carry, excl);
        carry = combine(carry, total);
    }
    if (threadIdx.x == 0) {
        fs_rx_totals t;
        t.payload_bytes = carry.sum;
        t.n_runs = carry.heads;
        t.reserved = 0;
        *a.totals = t;
        *a.copied = carry.sum <= a.cap ? carry.sum : 0ull;
    }
}

__global__ void __launch_bounds__(kThreads) coalesce_apply(const CoArgs a) {
    __shared__ Part s_part[kWaves];
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t i = blk * kScanBlock + threadIdx.x;
        const uint2 r = i < a.n ? a.rec[i] : make_uint2(0u, 0u);
        const bool acc = (r.y & kAccepted) != 0, head = (r.y & kHead) != 0;
        const uint32_t len = acc ? rec_len(r.x) : 0u;
        Part incl, excl, total;
        block_scan(Part{(uint64_t)len, head ? 1u : 0u, head ? i + 1u : 0u}, s_part, incl, excl, total);
        const Part base = a.prefix[blk];
        const Part in = combine(base, incl);
        const uint64_t off = base.sum + excl.sum;
        if (i < a.n) {
            const uint32_t run = acc ? in.heads - 1u : kNoRun;
            a.payoff[i] = off;
            a.runidx[i] = run;
            a.hidx[i] = acc ? in.hidx1 - 1u : kNoRun;
            if (a.run_of) a.run_of[i] = run;
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

__global__ void __launch_bounds__(kThreads) coalesce_copy(const CoArgs a) {
    const uint32_t sub = threadIdx.x & (kGroup - 1u), grp = threadIdx.x / kGroup;
    const uint32_t n_tiles = (a.n + kTileFrames - 1u) / kTileFrames;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t i = tile * kTileFrames + grp;
        if (i >= a.n) continue;
        const uint2 r = a.rec[i];  // (three independent loads: one latency)
        const uint64_t off = a.payoff[i];
        const uint64_t at = a.offsets[i];
        if (!(r.y & kAccepted)) continue;
        const uint32_t len = rec_len(r.x);
        if (len != 0 && off + len <= a.cap) copy_payload(a.payload + off, a.frames + at + rec_start(r.x), len, sub);
        if (sub == 8) {
            // a run ends where the next frame does not continue it (a continuing frame is accepted
            // and no head); its last frame writes the record, behind its copy's loads and stores
            const bool last = i + 1u == a.n || a.rec[i + 1u].y != kAccepted;
            if (last) {
                const uint32_t hd = a.hidx[i];
                const uint64_t hoff = a.payoff[hd];
                fs_rx_run run;
                run.payload_off = hoff;
                run.payload_len = (uint32_t)(off + len - hoff);
                run.first_frame = hd;
                run.n_frames = i - hd + 1u;
                run.tcp_flags = (uint8_t)run_flags(rec_flags(a.rec[hd].x), rec_flags(r.x));
                run.reserved[0] = run.reserved[1] = run.reserved[2] = 0;
                a.runs[a.runidx[i]] = run;
            }
        }
    }
}

}  // namespace

CoScratch coalesce_scratch(uint32_t n) {
    CoScratch s;
    const uint64_t nb = ((uint64_t)n + kScanBlock - 1) / kScanBlock;
    uint64_t at = 0;
    s.rec = at, at += 8ull * n;
    s.payoff = at, at += 8ull * n;
    s.partial = at, at += 16ull * nb;
    s.prefix = at, at += 16ull * nb;
    s.copied = at, at += 8;
    s.runidx = at, at += 4ull * n;
    s.hidx = at, at += 4ull * n;
    s.bytes = at;
    return s;
}

hipError_t launch_coalesce(const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths, uint32_t n,
                           uint32_t flags, const uint8_t* status, uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs,
                           uint32_t* run_of, fs_rx_totals* totals, uint8_t* scratch, int max_workgroups,
                           hipStream_t stream) {
    const CoScratch s = coalesce_scratch(n);
    CoArgs a;
    a.frames = frames;
    a.offsets = offsets;
    a.lengths = lengths;
    a.status = status;
    a.rec = reinterpret_cast<uint2*>(scratch + s.rec);
    a.payoff = reinterpret_cast<uint64_t*>(scratch + s.payoff);
    a.partial = reinterpret_cast<Part*>(scratch + s.partial);
    a.prefix = reinterpret_cast<Part*>(scratch + s.prefix);
    a.copied = reinterpret_cast<unsigned long long*>(scratch + s.copied);
    a.runidx = reinterpret_cast<uint32_t*>(scratch + s.runidx);
    a.hidx = reinterpret_cast<uint32_t*>(scratch + s.hidx);
    a.payload = payload;
    a.cap = payload_cap;
    a.runs = runs;
    a.run_of = run_of;
    a.totals = totals;
    a.n = n;
    a.n_blocks = (uint32_t)(((uint64_t)n + kScanBlock - 1) / kScanBlock);
    a.fcs = (flags & FS_RX_FCS) ? 4u : 0u;
    const uint32_t cap = (uint32_t)(max_workgroups > 0 ? max_workgroups : 1);
    const uint32_t n_tiles = (uint32_t)(((uint64_t)n + kTileFrames - 1) / kTileFrames);
    const uint32_t g_scan = a.n_blocks < cap ? a.n_blocks : cap, g_copy = n_tiles < cap ? n_tiles : cap;
    hipLaunchKernelGGL(coalesce_classify, dim3(g_scan), dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL(coalesce_scan_partials, dim3(1), dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL(coalesce_apply, dim3(g_scan), dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL(coalesce_copy, dim3(g_copy), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace framesum
