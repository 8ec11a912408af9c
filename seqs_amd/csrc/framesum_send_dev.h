// The ring piece source of the two ring-send kernel files (framesum_send.hip: fs_send_rings_batch;
// framesum_send_resident.hip: fs_send_rings_resident), written once. HIP only; framesum_send.hip's
// header comment says where a piece of a chunk comes from.
#pragma once
#include <hip/hip_runtime.h>

#include "framesum_send.h"
#include "framesum_tx_dev.h"

namespace framesum {
namespace senddev {
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

}  // namespace
}  // namespace senddev
}  // namespace framesum
