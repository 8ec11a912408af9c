// TX frame build (fs_segment_batch): TCP segmentation and UDP frame build in one fused pass.
//
// The frame body, the tables and the walk over the frames are framesum_tx_dev.h's (its header comment
// has the derivations); this file supplies the CRC tables' basis, the linear piece source and the
// kernel.
#include <hip/hip_runtime.h>

#include "framesum_internal.h"
#include "framesum_segment.h"
#include "framesum_tx_dev.h"

namespace framesum {

// Z_k[b][1 << j] for k = 1, 2, 4, ... 32768 (tables 0..15) and k = 12 (table 16), by stepping the 32
// one-bit registers through 32768 zero bytes.
void build_segment_tables(SegTables* t) {
    uint32_t byte_step[256];
    for (uint32_t v = 0; v < 256; ++v) {
        uint32_t r = v;
        for (int i = 0; i < 8; ++i) r = (r >> 1) ^ ((r & 1u) ? 0xEDB88320u : 0u);
        byte_step[v] = r;
    }
    uint32_t reg[32];
    for (int i = 0; i < 32; ++i) reg[i] = 1u << i;
    int next = 0;
    for (uint32_t k = 1; k <= 32768; ++k) {
        for (int i = 0; i < 32; ++i) reg[i] = (reg[i] >> 8) ^ byte_step[reg[i] & 255u];
        const bool pow2 = (k & (k - 1)) == 0;
        if (pow2 || k == 12) {
            const int tab = pow2 ? next++ : (int)kSegTableZ12;
            for (int i = 0; i < 32; ++i) t->basis[tab][i >> 3][i & 7] = reg[i];
        }
    }
}

namespace {

using segment::SendRec;
using SegArgs = txdev::Args<SendRec>;

// A chunk of a send's payload range: linear bytes. A send may be UDP, and one frame of all its bytes
// (mss == 0).
struct LinearSrc {
    using Rec = SendRec;
    static constexpr bool kMayUdp = true, kMssZero = true;
    static __device__ __forceinline__ uint32_t total(const SendRec* rec) { return rec->payload_len; }
    const uint8_t* __restrict__ src;
    __device__ __forceinline__ LinearSrc(const SegArgs& a, const SendRec* rec, uint32_t c0, uint32_t)
        : src(a.src + rec->payload_off + c0) {}
    __device__ __forceinline__ void load(int e, uint32_t d[4]) const { txdev::load_linear(src, e, d); }
};

__global__ void __launch_bounds__(txdev::kThreads) segment_kernel(const SegArgs a) { txdev::build_frames<LinearSrc>(a); }

}  // namespace

hipError_t launch_segment(const uint8_t* d_block, const segment::Block& b, uint32_t n_sends, uint32_t n_frames,
                          const uint8_t* payload, uint8_t* frames, uint64_t* offsets, uint32_t* lengths, void* out,
                          uint8_t* status, uint32_t mtu, uint32_t flags, uint32_t align, const SegTables* tables,
                          int workgroups, hipStream_t stream) {
    SegArgs a;
    const uint32_t grid = txdev::fill_args(a, d_block, b, n_sends, n_frames, payload, frames, offsets, lengths, out, status,
                                           mtu, flags, align, tables, workgroups);
    hipLaunchKernelGGL(segment_kernel, dim3(grid), dim3(txdev::kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace framesum
