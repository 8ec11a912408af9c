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
#include "framesum_send_dev.h"

namespace framesum {
namespace {

using senddev::RingSrc;  // the ring piece source (framesum_send_dev.h: the resident send's kernel takes it too)
using senddev::SendArgs;

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
