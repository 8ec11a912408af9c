// Flow-aware RX coalesce (fs_coalesce_flows_batch): behind the digest launch, put the accepted
// frames into delivery order -- flow by flow, flows by their first frame, a flow's frames in batch
// order -- gather their payload in that order and report the runs inside each flow.
//
// The launches on the caller's stream, none of which waits on another workgroup of its own launch:
//   keys      one lane per frame: the 16-byte key record (classify_frame's header load).
//   (memset)  the flow table and the per-slot first-frame words to 0xFFFFFFFF.
//   insert    one lane per accepted frame. The frames of a workgroup that share a key meet in a table
//             in LDS first; the first of them goes to the flow table for all: claim a slot with
//             atomicCAS or find the slot whose claimant has an equal key (the keys are the previous
//             launch's, so nothing waits for another lane's store), probing linearly; then atomicMin
//             the slot's first frame. Which frame claims a slot depends on timing; a slot's first
//             frame and the set of frames that share a slot do not.
//   sortkeys  one lane per frame: first frame of its flow << b | own index (framesum_flows.h).
//   sort      rocprim::radix_sort_keys over the low 2 b + 1 bits: sorted[k] & mask is the frame at
//             delivery slot k; the frames that are not accepted follow the accepted ones.
//   classify, partials, apply, copy
//             the gather steps of framesum_coalesce.hip (their one body is in framesum_coalesce_dev.h)
//             in the mode ByFlow below: slot k stands for frame sorted[k], so a wave's lanes hold
//             consecutive slots and pass their header to the next lane; a change of flow opens a run;
//             the scans also carry the flow heads, the last flow head's slot and the accepted count;
//             the copy's destination advances sequentially while its source is wherever the slot's
//             frame lies, and the last slot of a flow writes the flow's record as the last slot of a
//             run writes the run's, each behind its copy.
// Here are the three kernels of the delivery order, that mode, the gather kernels by the names the
// traces know, and the launch.
#include <hip/hip_runtime.h>

#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/framesum.h"
#include "framesum_coalesce.h"
#include "framesum_coalesce_dev.h"
#include "framesum_flows.h"
#include "framesum_internal.h"

namespace framesum {

namespace {

using namespace codev;
using flows::Key;

static_assert(sizeof(fs_rx_flow) == 32 && sizeof(fs_rx_flow_totals) == 24, "fs_rx_flow / fs_rx_flow_totals layout");
static_assert(sizeof(Key) == 16, "Key layout");

// What the scans carry: payload bytes, run heads and the last one's slot + 1 (0: none yet), flow
// heads and the last one's slot + 1, accepted frames.
struct FlowPart {
    uint64_t sum;
    uint32_t heads, hidx1;
    uint32_t fheads, fidx1;
    uint32_t acc, pad;
};
static_assert(sizeof(FlowPart) == 32, "FlowPart layout");

struct FlArgs {
    const uint8_t* frames;
    const uint64_t* offsets;
    const uint32_t* lengths;
    const uint8_t* status;
    uint4* keys;        // per frame
    uint32_t* table;    // tmask + 1 slots: the claiming frame
    uint32_t* rep;      // tmask + 1 slots: the flow's first frame
    uint32_t* slot_of;  // per frame
    uint64_t* sk_in;    // per frame
    uint64_t* sorted;   // per slot
    uint2* rec;         // per slot from here on
    uint64_t* payoff;
    uint32_t* runidx;
    uint32_t* hidx;
    uint32_t* flowidx;
    uint32_t* fhidx;
    FlowPart* partial;
    FlowPart* prefix;
    unsigned long long* copied;
    uint8_t* payload;
    uint64_t cap;
    fs_rx_run* runs;
    fs_rx_flow* flows;
    uint32_t* order;
    uint32_t* run_of;
    fs_rx_flow_totals* totals;
    uint32_t n, n_blocks, fcs, tmask, hash_mask, b;
};

__device__ __forceinline__ FlowPart combine(const FlowPart& a, const FlowPart& b) {
    return FlowPart{a.sum + b.sum, a.heads + b.heads, a.hidx1 > b.hidx1 ? a.hidx1 : b.hidx1,
                    a.fheads + b.fheads, a.fidx1 > b.fidx1 ? a.fidx1 : b.fidx1, a.acc + b.acc, 0u};
}
__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d, 64), hi = __shfl_up((uint32_t)(v >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ FlowPart shfl_up_part(const FlowPart& v, int d) {
    FlowPart u;
    u.sum = shfl_up_u64(v.sum, d);
    u.heads = __shfl_up(v.heads, d, 64);
    u.hidx1 = __shfl_up(v.hidx1, d, 64);
    u.fheads = __shfl_up(v.fheads, d, 64);
    u.fidx1 = __shfl_up(v.fidx1, d, 64);
    u.acc = __shfl_up(v.acc, d, 64);
    u.pad = 0;
    return u;
}

__device__ __forceinline__ Key load_key(const uint4* keys, uint32_t i) {
    const uint4 v = keys[i];
    return Key{{v.x, v.y, v.z, v.w}};
}

__global__ void __launch_bounds__(kThreads) flows_keys(const FlArgs a) {
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t i = blk * kScanBlock + threadIdx.x;
        if (i >= a.n) continue;
        Hdr h;
        const Info f = classify_frame(a, i, h);
        Key key = flows::no_key();
        if (f.accepted) {
            const uint32_t len = a.lengths[i];
            key = flows::key_of(h, a.frames + a.offsets[i], len >= a.fcs ? len - a.fcs : 0u);
        }
        a.keys[i] = make_uint4(key.w[0], key.w[1], key.w[2], key.w[3]);
    }
}

// The workgroup's own table, in LDS: its frames that share a key meet there first, and only the
// first of them goes to the flow table. Twice the frames of a workgroup, so it is at most half full.
constexpr uint32_t kLocalSlots = 2u * kScanBlock;

__global__ void __launch_bounds__(kThreads) flows_insert(const FlArgs a) {
    __shared__ uint4 s_key[kThreads];
    __shared__ uint32_t s_tab[kLocalSlots], s_min[kLocalSlots], s_slot[kLocalSlots];
    const uint32_t t = threadIdx.x;
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t i = blk * kScanBlock + t;
        const Key key = i < a.n ? load_key(a.keys, i) : flows::no_key();
        const bool acc = flows::key_accepted(key);
        s_key[t] = make_uint4(key.w[0], key.w[1], key.w[2], key.w[3]);
#pragma unroll
        for (uint32_t k = t; k < kLocalSlots; k += kThreads) s_tab[k] = s_min[k] = flows::kEmpty;
        __syncthreads();
        // in the workgroup: the same claim-or-compare as below, on LDS; s_min is the key's first lane
        const uint32_t hash = flows::key_hash(key) & a.hash_mask;
        uint32_t ls = flows::kEmpty;
        if (acc) {
            uint32_t s = hash & (kLocalSlots - 1u);
            for (uint32_t probe = 0; probe < kLocalSlots; ++probe) {
                uint32_t owner = atomicCAS(&s_tab[s], flows::kEmpty, t);
                if (owner == flows::kEmpty) owner = t;
                if (owner == t) {
                    ls = s;
                    break;
                }
                const uint4 o = s_key[owner & (kThreads - 1u)];
                if (flows::same_key(key, Key{{o.x, o.y, o.z, o.w}})) {
                    ls = s;
                    break;
                }
                s = (s + 1u) & (kLocalSlots - 1u);
            }
            if (ls != flows::kEmpty) atomicMin(&s_min[ls], t);
        }
        __syncthreads();
        // in the flow table: the key's first frame of this workgroup, for all of them
        if (acc && ls != flows::kEmpty && s_min[ls] == t) {
            uint32_t s = hash & a.tmask;
            uint32_t found = flows::kEmpty;
            // at most every slot once: the table is at most half full, so an empty slot turns up
            for (uint32_t probe = 0; probe <= a.tmask; ++probe) {
                // a slot never changes once claimed, so a plain look spares the contended atomic
                uint32_t owner = __hip_atomic_load(&a.table[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (owner == flows::kEmpty) {
                    owner = atomicCAS(&a.table[s], flows::kEmpty, i);
                    if (owner == flows::kEmpty) owner = i;
                }
                if (owner == i || (owner < a.n && flows::same_key(key, load_key(a.keys, owner)))) {
                    found = s;
                    break;
                }
                s = (s + 1u) & a.tmask;
            }
            // the slot's first frame only ever falls: a frame above what it sees has nothing to add
            if (found != flows::kEmpty &&
                __hip_atomic_load(&a.rep[found], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > i)
                atomicMin(&a.rep[found], i);
            s_slot[ls] = found;
        }
        __syncthreads();
        if (acc) a.slot_of[i] = ls != flows::kEmpty ? s_slot[ls] : flows::kEmpty;
        // (the next round rewrites s_key, s_tab and s_min, which nobody reads past the barrier above,
        // and s_slot only behind two more barriers)
    }
}

__global__ void __launch_bounds__(kThreads) flows_sortkeys(const FlArgs a) {
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t i = blk * kScanBlock + threadIdx.x;
        if (i >= a.n) continue;
        uint64_t k = flows::sort_key_rejected(i, a.b);
        if (a.keys[i].w & flows::kKeyAccepted) {
            const uint32_t s = a.slot_of[i];
            const uint32_t rep = s <= a.tmask ? a.rep[s] : i;
            k = flows::sort_key(rep <= i ? rep : i, i, a.b);
        }
        a.sk_in[i] = k;
    }
}

// The mode of the gather steps (framesum_coalesce_dev.h): slot k is the frame the k-th sort key
// names, a change of the keys' flow opens a flow, and the flows are recorded beside the runs.
struct ByFlow {
    using Part = FlowPart;
    using Key = uint64_t;  // the slot's sort key
    static constexpr uint32_t kFlowBit = flows::kFlowHead;
    static __device__ __forceinline__ Key key(const FlArgs& a, uint32_t k) { return a.sorted[k]; }
    static __device__ __forceinline__ Key shfl_up_key(Key sk) { return shfl_up_u64(sk, 1); }
    static __device__ __forceinline__ uint32_t frame(const FlArgs& a, uint32_t, Key sk) { return flows::sort_index(sk, a.b); }
    // the accepted frames come first, so an accepted slot behind slot 0 follows an accepted one
    static __device__ __forceinline__ bool flow_head(const FlArgs& a, uint32_t k, bool acc, bool pacc, Key sk, Key psk) {
        return acc && (k == 0 || !pacc || flows::sort_rep(psk, a.b) != flows::sort_rep(sk, a.b));
    }
    static __device__ __forceinline__ Part part(uint64_t len, bool head, bool fhead, bool acc, uint32_t k) {
        return Part{len, head ? 1u : 0u, head ? k + 1u : 0u, fhead ? 1u : 0u, fhead ? k + 1u : 0u, acc ? 1u : 0u, 0u};
    }
    static __device__ __forceinline__ void write_totals(const FlArgs& a, const Part& carry) {
        fs_rx_flow_totals t;
        t.payload_bytes = carry.sum;
        t.n_runs = carry.heads;
        t.n_flows = carry.fheads;
        t.n_accepted = carry.acc;
        t.reserved = 0;
        *a.totals = t;
    }
    static __device__ __forceinline__ void apply_extra(const FlArgs& a, uint32_t k, uint32_t i, const Part& in, bool acc) {
        a.flowidx[k] = acc ? in.fheads - 1u : kNoRun;
        a.fhidx[k] = acc ? in.fidx1 - 1u : kNoRun;
        if (acc) a.order[k] = i;  // (slot k of an accepted frame is below n_accepted)
    }
    // the flow ends where the next slot opens another, or holds no accepted frame: its last slot
    // writes the record, behind its copy
    static __device__ __forceinline__ void flow_record(const FlArgs& a, uint32_t k, uint32_t ny, uint64_t off, uint32_t len) {
        if (!a.flows || ((ny & kAccepted) && !(ny & flows::kFlowHead))) return;
        const uint32_t fh = a.fhidx[k];
        const uint64_t foff = a.payoff[fh];
        const uint32_t r0 = a.runidx[fh];
        fs_rx_flow fl;
        fl.payload_off = foff;
        fl.payload_len = off + len - foff;
        fl.first_run = r0;
        fl.n_runs = a.runidx[k] - r0 + 1u;
        fl.first_frame = fh;
        fl.n_frames = k - fh + 1u;
        a.flows[a.flowidx[k]] = fl;
    }
};

__global__ void __launch_bounds__(kThreads) flows_classify(const FlArgs a) { gather_classify<ByFlow>(a); }
__global__ void __launch_bounds__(kThreads) flows_scan_partials(const FlArgs a) { gather_scan_partials<ByFlow>(a); }
__global__ void __launch_bounds__(kThreads) flows_apply(const FlArgs a) { gather_apply<ByFlow>(a); }
__global__ void __launch_bounds__(kThreads) flows_copy(const FlArgs a) { gather_copy<ByFlow>(a); }

hipError_t sort_keys(void* temp, size_t& temp_bytes, uint64_t* in, uint64_t* out, uint32_t n, uint32_t bits,
                     hipStream_t stream) {
    return rocprim::radix_sort_keys(temp, temp_bytes, in, out, n, 0u, bits, stream);
}

}  // namespace

FlowScratch flows_scratch(uint32_t n) {
    FlowScratch s;
    const uint64_t slots = flows::table_slots(n);
    size_t sort_bytes = 0;
    // (a null pointer: the sort only reports what it needs)
    if (sort_keys(nullptr, sort_bytes, nullptr, nullptr, n, flows::sort_bits(flows::index_bits(n)), nullptr) != hipSuccess)
        sort_bytes = 0;
    uint64_t at = 0;
    s.keys = at, at += 16ull * n;
    s.sk_in = at, at += 8ull * n;
    s.sorted = at, at += 8ull * n;
    at = lay_scan_arrays(s, at, n, sizeof(FlowPart));
    s.table = at, at += 4ull * slots;  // table and rep lie together: one memset covers both
    s.rep = at, at += 4ull * slots;
    s.slot_of = at, at += 4ull * n;
    at = lay_run_arrays(s, at, n);
    s.flowidx = at, at += 4ull * n;
    s.fhidx = at, at += 4ull * n;
    at = (at + 255u) & ~255ull;
    s.sort_temp = at, at += sort_bytes;
    s.sort_bytes = sort_bytes;
    s.bytes = at;
    return s;
}

hipError_t launch_coalesce_flows(const RxBatch& b, const RxResults& r, const RxLeft& left, const RxLaunch& how) {
    uint8_t* const scratch = left.flow_scratch;
    const FlowScratch& s = left.fs;
    const uint32_t n = b.n, steps = how.steps;
    const hipStream_t stream = how.stream;
    FlArgs a;
    const GatherGrids g = fill_gather_args(a, b, r, scratch, s, how.max_workgroups);
    a.keys = reinterpret_cast<uint4*>(scratch + s.keys);
    a.table = reinterpret_cast<uint32_t*>(scratch + s.table);
    a.rep = reinterpret_cast<uint32_t*>(scratch + s.rep);
    a.slot_of = reinterpret_cast<uint32_t*>(scratch + s.slot_of);
    a.sk_in = reinterpret_cast<uint64_t*>(scratch + s.sk_in);
    a.sorted = reinterpret_cast<uint64_t*>(scratch + s.sorted);
    a.flowidx = reinterpret_cast<uint32_t*>(scratch + s.flowidx);
    a.fhidx = reinterpret_cast<uint32_t*>(scratch + s.fhidx);
    a.flows = r.flows();
    a.order = r.order();
    a.totals = static_cast<fs_rx_flow_totals*>(r.totals());
    a.tmask = flows::table_slots(n) - 1u;
    a.hash_mask = how.hash_mask;
    a.b = flows::index_bits(n);
    hipError_t e = hipSuccess;
    if (steps & kFlowStepOrder) {
        hipLaunchKernelGGL(flows_keys, dim3(g.scan), dim3(kThreads), 0, stream, a);
        e = hipMemsetAsync(scratch + s.table, 0xFF, 8ull * ((uint64_t)a.tmask + 1u), stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(flows_insert, dim3(g.scan), dim3(kThreads), 0, stream, a);
        hipLaunchKernelGGL(flows_sortkeys, dim3(g.scan), dim3(kThreads), 0, stream, a);
    }
    if (steps & kFlowStepSort) {
        size_t sort_bytes = s.sort_bytes;
        e = sort_keys(scratch + s.sort_temp, sort_bytes, a.sk_in, a.sorted, n, flows::sort_bits(a.b), stream);
        if (e != hipSuccess) return e;
    }
    if (steps & kFlowStepGather) {
        hipLaunchKernelGGL(flows_classify, dim3(g.scan), dim3(kThreads), 0, stream, a);
        hipLaunchKernelGGL(flows_scan_partials, dim3(1), dim3(kThreads), 0, stream, a);
        hipLaunchKernelGGL(flows_apply, dim3(g.scan), dim3(kThreads), 0, stream, a);
        hipLaunchKernelGGL(flows_copy, dim3(g.copy), dim3(kThreads), 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace framesum
