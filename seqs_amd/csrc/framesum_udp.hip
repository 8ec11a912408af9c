// The UDP delivery of the UDP call (fs_udp_flows_batch): behind the launches of the connect call
// (framesum_connect.hip), these kernels match every accepted UDP frame to a listed port under the rule of
// framesum_udp.h, rank each port's frames in batch order and copy every admitted datagram into its cell.
//
// The launches on the caller's stream, none of which waits on another workgroup or wave of its own
// launch, every loop bounded by a count known at its start:
//   init      one lane per port: the out record of a port without a frame (the input state, zero counts).
//   mark      one lane per frame: the frame's key record as the flow launches left it (when all of their
//             steps ran; the frame's own header otherwise), the port table's one or two probes, port_of
//             and the rank key port << b | frame, all ones when unmatched.
//   sort      rocprim::radix_sort_keys over the low b + index_bits(n_ports) bits: every port's frames
//             together, in ascending batch index.
//   assign    one lane per sorted position: the binary search for the port's first position gives the
//             rank, the rank the cell or FULL; cell_of; the datagram's `stored` bytes go into the port's
//             sums (a wave whose lanes serve one port adds once); the port's last position writes its
//             counts and state, its first position `first`. Integer sums: their order changes nothing.
//   copy      the hot path, one group of lanes per sorted position: the 32-byte cell header from the frame's
//             own bytes as two 16-byte stores, then the payload from a byte-aligned source. The group is
//             decided per call from the port list (framesum_udp.h copy_lanes): 4 lanes where no cell has
//             room for more than 64 payload bytes (the reference's benchmark: 47-byte frames, 5 payload
//             bytes, 40-byte cells: 64 datagrams per workgroup, two lanes write the header, one the
//             payload), else flows_copy's 16 lanes and codev::copy_payload (1,500-byte frames: 92
//             16-byte pieces, six rounds of 16 lanes).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/framesum_udp.h"
#include "framesum_coalesce.h"
#include "framesum_coalesce_dev.h"
#include "framesum_flows.h"
#include "framesum_internal.h"
#include "framesum_udp.h"

namespace framesum {

namespace {

using namespace codev;
namespace ud = udp;

struct UdArgs {
    const uint8_t* frames;
    const uint64_t* offsets;
    const uint32_t* lengths;
    const uint8_t* status;
    const uint4* keys;  // per frame: the flow launches' key records, or null
    // the staged block
    const fs_udp_port* ports;
    const uint32_t* table;
    // this call's own scratch
    uint64_t* rank_in;
    const uint64_t* rank_sorted;
    uint32_t* cell_at;  // per sorted position: the cell, FULL or NONE
    // the results
    uint8_t* cells;
    fs_udp_port_out* ports_out;
    uint32_t* port_of;
    uint32_t* cell_of;
    uint32_t n, n_blocks, n_ports, tmask, hash_mask, b, lb, fcs;
};

__global__ void __launch_bounds__(kThreads) udp_init(const UdArgs a) {
    const uint32_t n_blocks = (a.n_ports + kScanBlock - 1u) / kScanBlock;
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint32_t p = blk * kScanBlock + threadIdx.x;
        if (p < a.n_ports) a.ports_out[p] = ud::port_out(a.ports[p], 0u);
    }
}

__global__ void __launch_bounds__(kThreads) udp_mark(const UdArgs a) {
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t i = blk * kScanBlock + threadIdx.x;
        if (i >= a.n) continue;
        flows::Key key;
        if (a.keys) {
            const uint4 v = a.keys[i];
            key = flows::Key{{v.x, v.y, v.z, v.w}};
        } else {
            key = ud::key_of_frame(a.frames + a.offsets[i], a.status[i] == FS_OK);
        }
        const uint32_t p = ud::match_port(key, a.ports, a.table, a.n_ports, a.tmask, a.hash_mask);
        if (a.port_of) a.port_of[i] = p;
        a.rank_in[i] = p == ud::kNoPort ? ud::kUnmatched : ud::rank_key(p, i, a.b);
    }
}

// The frame's bytes that count (the FCS does not).
__device__ __forceinline__ uint32_t avail_of(const UdArgs& a, uint32_t i) {
    const uint32_t len = a.lengths[i];
    return len >= a.fcs ? len - a.fcs : 0u;
}

__global__ void __launch_bounds__(kThreads) udp_assign(const UdArgs a) {
    const uint64_t mask = ((uint64_t)1 << (a.b + a.lb)) - 1u;
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t pos = blk * kScanBlock + threadIdx.x;
        const uint64_t rk = pos < a.n ? a.rank_sorted[pos] : ud::kUnmatched;
        uint32_t p = ud::kNoPort, i = 0u;
        // (mark leaves the bits above the port zero, so the shift alone gives it: accept::rank_listener's mask
        // is for keys read under the sort's bit range; `p < n_ports` below guards the rest)
        if (rk != ud::kUnmatched) p = ud::rank_port(rk, a.b), i = ud::rank_frame(rk, a.b);
        const bool mine = p < a.n_ports && i < a.n;  // (mark writes no other key)
        uint32_t cell = ud::kNoPort, stored = 0u, truncated = 0u;
        if (mine) {
            const fs_udp_port port = a.ports[p];
            const uint32_t rank = pos - ud::lower_bound(a.rank_sorted, a.n, (uint64_t)p << a.b, mask);
            cell = ud::cell_of_rank(port, rank);
            if (a.cell_of) a.cell_of[i] = cell;
            if (cell != ud::kCellFull) {
                const ud::Dgram d = ud::dgram_of(a.frames + a.offsets[i], avail_of(a, i), port.cell_size);
                stored = d.stored, truncated = d.stored < d.len ? 1u : 0u;
            }
            const uint64_t after = pos + 1u < a.n ? a.rank_sorted[pos + 1u] : ud::kUnmatched;
            fs_udp_port_out* const o = a.ports_out + p;
            if (rank == 0u) o->first = i;
            if (after == ud::kUnmatched || ud::rank_port(after, a.b) != p) {  // the port's last frame
                const fs_udp_port_out r = ud::port_out(port, rank + 1u);
                o->wcell = r.wcell, o->free = r.free, o->n_matched = r.n_matched, o->n_admitted = r.n_admitted;
            }
        }
        if (pos < a.n) a.cell_at[pos] = cell;
        // the port's sums: when every lane of the wave that has a datagram serves the first such lane's
        // port, one lane adds the wave's sums; otherwise every lane adds its own
        const unsigned long long have = __ballot(mine);
        if (have == 0ull) continue;
        const uint32_t lead = (uint32_t)__builtin_ctzll(have);
        const bool uniform = __ballot(mine && p != lane_value(p, lead)) == 0ull;
        if (uniform) {
            uint32_t s = stored, t = truncated;
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m, 64), t += __shfl_xor(t, m, 64);
            if ((threadIdx.x & 63u) == lead) {
                if (s) atomicAdd(reinterpret_cast<unsigned long long*>(&a.ports_out[p].bytes), (unsigned long long)s);
                if (t) atomicAdd(&a.ports_out[p].n_truncated, t);
            }
        } else if (mine) {
            if (stored) atomicAdd(reinterpret_cast<unsigned long long*>(&a.ports_out[p].bytes), (unsigned long long)stored);
            if (truncated) atomicAdd(&a.ports_out[p].n_truncated, 1u);
        }
    }
}

// The cell header of datagram `d` of frame `i` at `src` as two 16-byte pieces.
__device__ __forceinline__ void header_pieces(const uint8_t* __restrict__ src, uint32_t i, const ud::Dgram& d, Piece& h0, Piece& h1) {
    uint32_t w[8];
    ud::cell_words(src, i, d, w);
    h0.d[0] = w[0], h0.d[1] = w[1], h0.d[2] = w[2], h0.d[3] = w[3];
    h1.d[0] = w[4], h1.d[1] = w[5], h1.d[2] = w[6], h1.d[3] = w[7];
}

// What a group of the copy finds at sorted position `pos`: false where no datagram goes to a cell.
struct CopyJob {
    const uint8_t* src;
    uint8_t* dst;
    uint32_t frame;
    ud::Dgram d;
};
__device__ __forceinline__ bool copy_job(const UdArgs& a, uint32_t pos, CopyJob& j) {
    const uint32_t cell = a.cell_at[pos];  // (loads that do not wait for each other)
    const uint64_t rk = a.rank_sorted[pos];
    if (cell >= ud::kCellFull || rk == ud::kUnmatched) return false;
    const uint32_t p = ud::rank_port(rk, a.b), i = ud::rank_frame(rk, a.b);
    if (p >= a.n_ports || i >= a.n) return false;
    const fs_udp_port port = a.ports[p];
    if (cell >= port.n_cells) return false;  // (assign writes no such cell)
    j.src = a.frames + a.offsets[i];
    j.dst = a.cells + port.cells_off + (uint64_t)cell * port.cell_size;
    j.frame = i;
    j.d = ud::dgram_of(j.src, avail_of(a, i), port.cell_size);
    return true;
}

// 16 lanes per datagram: lane 15, which the payload's head and tail do not use, writes the header.
__global__ void __launch_bounds__(kThreads) udp_copy(const UdArgs a) {
    const uint32_t sub = threadIdx.x & (kGroup - 1u), grp = threadIdx.x / kGroup;
    const uint32_t n_tiles = (a.n + kTileFrames - 1u) / kTileFrames;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t pos = tile * kTileFrames + grp;
        CopyJob j;
        if (pos >= a.n || !copy_job(a, pos, j)) continue;
        if (sub == 15u) {
            Piece h0, h1;
            header_pieces(j.src, j.frame, j.d, h0, h1);
            *reinterpret_cast<Piece*>(j.dst) = h0;
            *reinterpret_cast<Piece*>(j.dst + 16) = h1;
        }
        if (j.d.stored != 0u) copy_payload(j.dst + ud::kCellHeader, j.src + j.d.start, j.d.stored, sub);
    }
}

// 4 lanes per datagram, for port lists whose cells hold at most 64 payload bytes: lanes 0 and 1 write the
// header's halves, and lane s the payload's 16-byte piece s (whole pieces as one store, the last piece's
// 1 .. 15 bytes one by one: at most ud::kNarrowRoom / 16 pieces, so every lane has at most one).
constexpr uint32_t kNarrow = ud::kNarrowLanes, kNarrowTile = (uint32_t)kThreads / kNarrow;
__global__ void __launch_bounds__(kThreads) udp_copy_narrow(const UdArgs a) {
    const uint32_t sub = threadIdx.x & (kNarrow - 1u), grp = threadIdx.x / kNarrow;
    const uint32_t n_tiles = (a.n + kNarrowTile - 1u) / kNarrowTile;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t pos = tile * kNarrowTile + grp;
        CopyJob j;
        if (pos >= a.n || !copy_job(a, pos, j)) continue;
        if (sub < 2u) {
            Piece h0, h1;
            header_pieces(j.src, j.frame, j.d, h0, h1);
            Piece h;  // (chosen word by word: registers, not an indexed copy)
            h.d[0] = sub == 0u ? h0.d[0] : h1.d[0], h.d[1] = sub == 0u ? h0.d[1] : h1.d[1];
            h.d[2] = sub == 0u ? h0.d[2] : h1.d[2], h.d[3] = sub == 0u ? h0.d[3] : h1.d[3];
            *reinterpret_cast<Piece*>(j.dst + 16u * sub) = h;
        }
        const uint32_t stored = j.d.stored <= ud::kNarrowRoom ? j.d.stored : ud::kNarrowRoom;  // (the host chose this kernel for such cells only)
        const uint32_t at = 16u * sub;
        if (at >= stored) continue;
        const uint8_t* __restrict__ s = j.src + j.d.start + at;
        uint8_t* __restrict__ t = j.dst + ud::kCellHeader + at;
        if (stored - at >= 16u) {
            *reinterpret_cast<Piece*>(t) = *reinterpret_cast<const Piece*>(s);
        } else {
            for (uint32_t k = 0; k < 15u && k < stored - at; ++k) t[k] = s[k];
        }
    }
}

}  // namespace

// The rank-by-sort of this call, which the ARP call's launches (framesum_arp.hip) use as it is.
hipError_t rank_sort_keys(void* temp, size_t& temp_bytes, uint64_t* in, uint64_t* out, uint32_t n, uint32_t bits,
                          hipStream_t stream) {
    return rocprim::radix_sort_keys(temp, temp_bytes, in, out, n, 0u, bits, stream);
}

UdpScratch udp_scratch(uint32_t n, uint32_t n_ports) {
    UdpScratch s;
    size_t sort_bytes = 0;
    // (a null pointer: the sort only reports what it needs)
    if (n != 0 && rank_sort_keys(nullptr, sort_bytes, nullptr, nullptr, n, udp::rank_bits(flows::index_bits(n), n_ports), nullptr) !=
                      hipSuccess)
        sort_bytes = 0;
    uint64_t at = 0;
    s.rank_in = at, at += 8ull * n;
    s.rank_sorted = at, at += 8ull * n;
    s.cell_at = at, at += 4ull * n;
    at = (at + 255u) & ~255ull;
    s.sort_temp = at, at += sort_bytes;
    s.sort_bytes = sort_bytes;
    s.bytes = at;
    return s;
}

hipError_t launch_udp(const RxBatch& b, const RxResults& r, const RxUdp& u, const RxLeft& left, const uint8_t* d_block,
                      const RxLaunch& how) {
    uint8_t* const scratch = left.udp_scratch;
    const UdpScratch& s = left.us;
    const uint32_t n = b.n;
    const hipStream_t stream = how.stream;
    const udp::Block blk = udp::block_of(u.n_ports);
    UdArgs a;
    a.frames = b.frames;
    a.offsets = b.offsets;
    a.lengths = b.lengths;
    a.status = r.status;
    // the key records are whole only when every step of the flow launches ran in this call
    a.keys = n != 0 && how.steps == kFlowStepsAll && left.flow_scratch
                 ? reinterpret_cast<const uint4*>(left.flow_scratch + left.fs.keys)
                 : nullptr;
    a.ports = reinterpret_cast<const fs_udp_port*>(d_block);
    a.table = reinterpret_cast<const uint32_t*>(d_block + blk.table);
    a.rank_in = reinterpret_cast<uint64_t*>(scratch + s.rank_in);
    a.rank_sorted = reinterpret_cast<const uint64_t*>(scratch + s.rank_sorted);
    a.cell_at = reinterpret_cast<uint32_t*>(scratch + s.cell_at);
    a.cells = u.cells;
    a.ports_out = u.ports_out;
    a.port_of = u.port_of;
    a.cell_of = u.cell_of;
    a.n = n;
    const ScanGrid g = scan_grid(n, how);
    a.n_blocks = g.blocks;
    a.n_ports = u.n_ports;
    a.tmask = flows::table_slots(u.n_ports) - 1u;
    a.hash_mask = how.hash_mask;
    a.b = flows::index_bits(n);
    a.lb = flows::index_bits(u.n_ports);
    a.fcs = (b.flags & FS_RX_FCS) ? 4u : 0u;
    const uint32_t port_blocks = (u.n_ports + kScanBlock - 1u) / kScanBlock;
    hipLaunchKernelGGL(udp_init, dim3(g.capped(port_blocks)), dim3(kThreads), 0, stream, a);
    if (n == 0) return hipGetLastError();
    hipLaunchKernelGGL(udp_mark, dim3(g.scan), dim3(kThreads), 0, stream, a);
    size_t sort_bytes = s.sort_bytes;
    const hipError_t e = rank_sort_keys(scratch + s.sort_temp, sort_bytes, a.rank_in, reinterpret_cast<uint64_t*>(scratch + s.rank_sorted),
                                   n, udp::rank_bits(a.b, u.n_ports), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(udp_assign, dim3(g.scan), dim3(kThreads), 0, stream, a);
    if (udp::copy_lanes(u.max_cell) == udp::kNarrowLanes) {
        const uint32_t n_tiles = (uint32_t)(((uint64_t)n + kNarrowTile - 1) / kNarrowTile);
        hipLaunchKernelGGL(udp_copy_narrow, dim3(g.capped(n_tiles)), dim3(kThreads), 0, stream, a);
    } else {
        const uint32_t n_tiles = (uint32_t)(((uint64_t)n + kTileFrames - 1) / kTileFrames);
        hipLaunchKernelGGL(udp_copy, dim3(g.capped(n_tiles)), dim3(kThreads), 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace framesum
