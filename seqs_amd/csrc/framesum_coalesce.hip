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
// The four steps are the gather steps of framesum_coalesce_dev.h, which fs_coalesce_flows_batch runs
// too; here are the mode that makes them this call's (Plain: slot k of the scans is frame k, no
// flows), the kernels by the names the traces know, and the launch.
#include <hip/hip_runtime.h>

#include "../../include/framesum.h"
#include "framesum_coalesce.h"
#include "framesum_coalesce_dev.h"
#include "framesum_internal.h"

namespace framesum {

namespace {

using namespace codev;  // the scan, the header load, the copy and the gather steps shared with framesum_flows.hip

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

// The mode of the gather steps (framesum_coalesce_dev.h): slot k is frame k, and there are no flows.
struct Plain {
    using Part = framesum::Part;
    struct Key {};
    static constexpr uint32_t kFlowBit = 0;
    static __device__ __forceinline__ Key key(const CoArgs&, uint32_t) { return Key{}; }
    static __device__ __forceinline__ Key shfl_up_key(Key) { return Key{}; }
    static __device__ __forceinline__ uint32_t frame(const CoArgs&, uint32_t k, Key) { return k; }
    static __device__ __forceinline__ Part part(uint64_t len, bool head, bool, bool, uint32_t k) {
        return Part{len, head ? 1u : 0u, head ? k + 1u : 0u};
    }
    static __device__ __forceinline__ void write_totals(const CoArgs& a, const Part& carry) {
        fs_rx_totals t;
        t.payload_bytes = carry.sum;
        t.n_runs = carry.heads;
        t.reserved = 0;
        *a.totals = t;
    }
};

__global__ void __launch_bounds__(kThreads) coalesce_classify(const CoArgs a) { gather_classify<Plain>(a); }
__global__ void __launch_bounds__(kThreads) coalesce_scan_partials(const CoArgs a) { gather_scan_partials<Plain>(a); }
__global__ void __launch_bounds__(kThreads) coalesce_apply(const CoArgs a) { gather_apply<Plain>(a); }
__global__ void __launch_bounds__(kThreads) coalesce_copy(const CoArgs a) { gather_copy<Plain>(a); }

}  // namespace

CoScratch coalesce_scratch(uint32_t n) {
    CoScratch s;
    s.bytes = lay_run_arrays(s, lay_scan_arrays(s, 0, n, sizeof(Part)), n);
    return s;
}

hipError_t launch_coalesce(const RxBatch& b, const RxResults& r, uint8_t* scratch, const RxLaunch& how) {
    CoArgs a;
    const GatherGrids g = fill_gather_args(a, b, r, scratch, coalesce_scratch(b.n), how.max_workgroups);
    const hipStream_t stream = how.stream;
    a.totals = static_cast<fs_rx_totals*>(r.totals());
    hipLaunchKernelGGL(coalesce_classify, dim3(g.scan), dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL(coalesce_scan_partials, dim3(1), dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL(coalesce_apply, dim3(g.scan), dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL(coalesce_copy, dim3(g.copy), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace framesum
