// Ring send (fs_send_rings_batch): TCP segments built straight from socket TX rings.
//
// The frame body, the tables and the walk over the frames are the TX frame build's (framesum_tx_dev.h,
// whose header comment has the derivations): one wave builds one frame at a time, its 64 lanes stream
// the frame's chunk in 16-byte pieces counted back from the chunk's END, piece p = chunk[C - 16(p+1),
// C - 16p), lane l takes pieces l, l + 64, ... This file supplies the ring piece source and the kernel.
//
// What differs is where a piece comes from. The chunk of frame k starts at ring position
// p0 = (ring_rpos + k mss) mod ring_size and has w = ring_size - p0 bytes before the ring's end.
// chunk <= data <= ring_buffered <= ring_size, so a chunk crosses the end at most once:
//   a piece that ends at or before w is one 16-byte load at ring + p0 + e - 16 (the chunk's head of
//   1..15 bytes: one 8-, 4-, 2- and 1-byte load each), at whatever alignment that has;
//   a piece that starts at or behind w is the same load at ring + e - 16 - w;
//   the one piece with lo < w < e (lo = max(e - 16, 0)) is put together byte by byte, bytes [lo, w)
//   from the ring's last bytes and [w, e) from its first. One lane of one frame per socket and call
//   does that, and every load stays inside the chunk's own ring bytes.
// Nothing is loaded outside the sent range, so a ring may end at the last byte of `rings`.
#include <hip/hip_runtime.h>

#include "framesum_internal.h"
#include "framesum_send.h"
#include "framesum_tx_dev.h"

namespace framesum {
namespace {

using send::RingRec;
using SendArgs = txdev::Args<RingRec>;

// A chunk of a socket's sent bytes: TCP only, mss > 0. `w`: the chunk's bytes before the ring's end
// (INT_MAX: it does not wrap); chunk byte j lies at src + j before the end and at past + j behind it.
struct RingSrc {
    using Rec = RingRec;
    static constexpr bool kMayUdp = false, kMssZero = false;
    static __device__ __forceinline__ uint32_t total(const RingRec* rec) { return rec->data; }
    const uint8_t* __restrict__ src;
    const uint8_t* __restrict__ past;
    int w;
    __device__ __forceinline__ RingSrc(const SendArgs& a, const RingRec* rec, uint32_t c0, uint32_t C) {
        // the chunk's first byte in the ring (ring_rpos + c0 < 2 ring_size <= 2^32), and its bytes before the end
        const uint32_t size = rec->ring_size;
        uint32_t p0 = rec->ring_rpos + c0;
        p0 = p0 >= size ? p0 - size : p0;
        const uint32_t before = size - p0;
        w = before >= C ? 0x7FFFFFFF : (int)before;
        src = a.src + rec->ring_off + p0;
        past = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(src) - size);
    }
    __device__ __forceinline__ void load(int e, uint32_t d[4]) const { txdev::load_ring(src, past, w, e, d); }
};

// (76 VGPRs: 6 waves per SIMD, the two workgroups per CU. A second copy of load_linear for the bytes
// behind the ring's end, or an unrolled straddling path, took 86 and 112: one workgroup per CU.)
__global__ void __launch_bounds__(txdev::kThreads) send_rings_kernel(const SendArgs a) { txdev::build_frames<RingSrc>(a); }

}  // namespace

hipError_t launch_send_rings(const uint8_t* d_block, const segment::Block& b, uint32_t n_recs, uint32_t n_frames,
                             const uint8_t* rings, uint8_t* frames, uint64_t* offsets, uint32_t* lengths, void* out,
                             uint8_t* status, uint32_t mtu, uint32_t flags, uint32_t align, const SegTables* tables,
                             int workgroups, hipStream_t stream) {
    SendArgs a;
    const uint32_t grid = txdev::fill_args(a, d_block, b, n_recs, n_frames, rings, frames, offsets, lengths, out, status, mtu,
                                           flags, align, tables, workgroups);
    hipLaunchKernelGGL(send_rings_kernel, dim3(grid), dim3(txdev::kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace framesum
