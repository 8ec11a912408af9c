// Resident ring send (fs_send_rings_resident): the ring send with its socket table in device memory.
//
// Four launches on the call's stream, each behind the one before it. The arithmetic of the first three
// is framesum_send_resident.h's (and through it framesum_send.h's checks, rule, records and block),
// one lane per socket; this file adds the scans between the lanes. Sockets are cut into chunks of 256,
// one workgroup pass each:
//   plan_sums   per chunk, the sums of what its sockets add to the scans (frames, slot bytes, ring bytes,
//               records, ID powers, idle and invalid sockets): hand-off, checks and rule per lane, then a
//               workgroup reduction.
//   plan_cut    one workgroup: the exclusive prefix of the at most 256 chunk sums; the first chunk whose
//               inclusive sums exceed frames_cap or frames_bytes holds the first socket that does not
//               fit, so its 256 sockets are planned once more and scanned to find it (the cut). Writes
//               the chunk bases, the head (cut, built counts, the block's layout, the frame kernel's
//               tile), the totals and the prefix's last entry.
//   plan_write  per chunk, the in-chunk exclusive scan on top of the chunk's base, then everything a
//               socket's lane writes: socks_out, its record, prefix entry and ID powers in the block
//               (send::stage's block, compacted: sockets before the cut that make a frame), and with
//               FS_TX_WRITEBACK its state in the table.
// The sums count every valid socket as if nothing were deferred; since the built sockets are exactly
// those with frames before the cut, the exclusive sums in front of a built socket are sums over built
// sockets only, which is why one scan serves the capacity rule, the layout and the compaction.
//   send_resident_kernel  txdev::build_frames over the ring piece source, the frame body of
//               fs_send_rings_batch, with n_recs, n_frames, the tile and the block's layout read from the
//               head. Its grid is sized from frames_cap, since the host knows no count; a workgroup with
//               no tile leaves before it builds the tables.
#include <hip/hip_runtime.h>

#include "framesum_internal.h"
#include "framesum_send_dev.h"
#include "framesum_send_resident.h"

namespace framesum {
namespace {

using resident::Call;
using resident::Head;
using resident::kChunk;
using resident::SockPlan;
using resident::Sums;
using senddev::RingSrc;
using senddev::SendArgs;

constexpr uint32_t kPlanWaves = kChunk / 64;

// Exclusive scan of one value over the workgroup's 256 lanes, and the workgroup's total: an inclusive
// scan per wave by lane shifts, then the four wave totals through LDS.
template <class T>
__device__ __forceinline__ T block_excl(T v, T& total) {
    __shared__ T wave_sum[kPlanWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(inc, d, 64);
        if (lane >= (uint32_t)d) inc += o;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    T base = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kPlanWaves; ++w) {
        const T x = wave_sum[w];
        base += w < wave ? x : (T)0;
        total += x;
    }
    __syncthreads();  // (the next scan reuses wave_sum)
    return base + inc - v;
}
__device__ __forceinline__ Sums block_excl_sums(const Sums& v, Sums& total) {
    Sums e;
    e.frames = block_excl<uint64_t>(v.frames, total.frames);
    e.bytes = block_excl<uint64_t>(v.bytes, total.bytes);
    e.data = block_excl<uint64_t>(v.data, total.data);
    e.ids = block_excl<uint64_t>(v.ids, total.ids);
    e.recs = block_excl<uint32_t>(v.recs, total.recs);
    e.idle = block_excl<uint32_t>(v.idle, total.idle);
    e.invalid = block_excl<uint32_t>(v.invalid, total.invalid);
    return e;
}

__global__ void __launch_bounds__(kChunk) plan_sums_kernel(const Call c, Sums* __restrict__ chunk_sums) {
    const uint32_t chunks = (c.n_socks + kChunk - 1) / kChunk;
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const uint32_t i = chunk * kChunk + threadIdx.x;
        Sums mine, total;
        if (i < c.n_socks) mine = resident::sums_of(resident::plan_sock(c, i));
        block_excl_sums(mine, total);
        if (threadIdx.x == 0) chunk_sums[chunk] = total;
    }
}

__global__ void __launch_bounds__(kChunk) plan_cut_kernel(const Call c, const Sums* __restrict__ chunk_sums,
                                                           Sums* __restrict__ chunk_base, Head* __restrict__ head,
                                                           uint8_t* __restrict__ block) {
    __shared__ uint32_t cut_chunk, cut;
    __shared__ uint64_t cut_base_words[sizeof(Sums) / 8];  // a Sums (its initialisers keep it from being __shared__)
    Sums& cut_base = *reinterpret_cast<Sums*>(cut_base_words);
    const uint32_t chunks = (c.n_socks + kChunk - 1) / kChunk, t = threadIdx.x;  // chunks <= kMaxChunks == kChunk
    if (t == 0) {
        cut_chunk = 0xFFFFFFFFu;
        cut = c.n_socks;
    }
    Sums mine, all;
    if (t < chunks) mine = chunk_sums[t];
    const Sums base = block_excl_sums(mine, all);  // (its barriers order the two initial stores too)
    if (t < chunks) {
        chunk_base[t] = base;
        if (!resident::fits(c, resident::add(base, mine))) atomicMin(&cut_chunk, t);
    }
    __syncthreads();
    const uint32_t cc = cut_chunk;
    if (cc == 0xFFFFFFFFu) {  // everything fits
        if (t == 0) {
            const Head h = resident::head_of(c, c.n_socks, all);
            *head = h;
            *c.totals = resident::totals_of(all, all);
            resident::write_prefix_end(h, block);
        }
        return;
    }
    if (t == cc) cut_base = base;
    // the cut chunk's sockets once more: the first one with frames whose inclusive sums do not fit
    const uint32_t i = cc * kChunk + t;
    Sums s, chunk_total;
    if (i < c.n_socks) s = resident::sums_of(resident::plan_sock(c, i));
    const Sums before = block_excl_sums(s, chunk_total);  // (its barriers order cut_base's store)
    const Sums excl = resident::add(cut_base, before);
    if (s.recs && !resident::fits(c, resident::add(excl, s))) atomicMin(&cut, i);
    __syncthreads();
    if (i == cut) {  // `excl`: the sums over the sockets before the cut, the built ones among them
        const Head h = resident::head_of(c, i, excl);
        *head = h;
        *c.totals = resident::totals_of(excl, all);
        resident::write_prefix_end(h, block);
    }
}

__global__ void __launch_bounds__(kChunk) plan_write_kernel(const Call c, const Sums* __restrict__ chunk_base,
                                                             const Head* __restrict__ head, uint8_t* __restrict__ block) {
    const uint32_t chunks = (c.n_socks + kChunk - 1) / kChunk;
    const Head h = *head;
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const uint32_t i = chunk * kChunk + threadIdx.x;
        SockPlan q;
        Sums mine, total;
        if (i < c.n_socks) {
            q = resident::plan_sock(c, i);
            mine = resident::sums_of(q);
        }
        const Sums before = block_excl_sums(mine, total);
        if (i < c.n_socks) resident::write_sock(c, h, block, i, q, resident::add(chunk_base[chunk], before));
    }
}

// The frame body of send_rings_kernel (framesum_send.hip), its counts, tile and block layout from the head.
__global__ void __launch_bounds__(txdev::kThreads) send_resident_kernel(const SendArgs a0, const Head* __restrict__ head,
                                                                          const uint8_t* __restrict__ block) {
    SendArgs a = a0;
    a.n_recs = head->n_recs;
    a.n_frames = head->n_frames;
    a.tile = head->tile;
    const uint32_t n_tiles = (a.n_frames + a.tile - 1) / a.tile;
    if (blockIdx.x * txdev::kWaves >= n_tiles) return;  // (the whole workgroup: the grid is sized from frames_cap)
    a.recs = reinterpret_cast<const send::RingRec*>(block + head->recs_at);
    a.prefix = reinterpret_cast<const uint32_t*>(block + head->prefix_at);
    a.ids = reinterpret_cast<const uint16_t*>(block + head->ids_at);
    txdev::build_frames<RingSrc>(a);
}

}  // namespace

hipError_t launch_send_resident(resident::Call c, uint8_t* scratch, const resident::Scratch& sl, const uint8_t* rings,
                                uint8_t* frames, uint64_t* offsets, uint32_t* lengths, void* out, uint8_t* status,
                                uint32_t mtu, const SegTables* tables, int plan_workgroups, int tx_workgroups,
                                hipStream_t stream) {
    const uint32_t chunks = (c.n_socks + kChunk - 1) / kChunk;
    const uint32_t plan_grid = chunks < (uint32_t)plan_workgroups ? chunks : (uint32_t)plan_workgroups;
    // the frame kernel's grid: no more workgroups than frames_cap frames can give a tile each
    const uint64_t want = ((uint64_t)c.frames_cap + txdev::kWaves - 1) / txdev::kWaves;
    const uint32_t grid = (uint32_t)(want < (uint64_t)tx_workgroups ? want : (uint64_t)tx_workgroups);
    c.grid_waves = (grid ? grid : 1u) * txdev::kWaves;
    Sums* chunk_sums = reinterpret_cast<Sums*>(scratch + sl.chunk_sums);
    Sums* chunk_base = reinterpret_cast<Sums*>(scratch + sl.chunk_base);
    Head* head = reinterpret_cast<Head*>(scratch + sl.head);
    uint8_t* block = scratch + sl.block;
    hipLaunchKernelGGL(plan_sums_kernel, dim3(plan_grid), dim3(kChunk), 0, stream, c, chunk_sums);
    hipLaunchKernelGGL(plan_cut_kernel, dim3(1), dim3(kChunk), 0, stream, c, chunk_sums, chunk_base, head, block);
    hipLaunchKernelGGL(plan_write_kernel, dim3(plan_grid), dim3(kChunk), 0, stream, c, chunk_base, head, block);
    if (grid) {
        SendArgs a;
        a.recs = nullptr;  // (the kernel takes the three from the head)
        a.prefix = nullptr;
        a.ids = nullptr;
        a.src = rings;
        a.frames = frames;
        a.offsets = offsets;
        a.lengths = lengths;
        a.out = static_cast<uint2*>(out);
        a.status = status;
        a.tables = tables;
        a.n_recs = a.n_frames = a.tile = 0;
        a.mtu = mtu;
        a.flags = c.flags & FS_FCS_APPEND;
        a.align = c.align;
        hipLaunchKernelGGL(send_resident_kernel, dim3(grid), dim3(txdev::kThreads), 0, stream, a, head, block);
    }
    return hipGetLastError();
}

}  // namespace framesum
