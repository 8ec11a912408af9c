// The ARP branch of the ARP call (fs_arp_flows_batch): behind the launches of the UDP call
// (framesum_udp.hip), these kernels classify every frame whose verdict is FS_ARP under the rules of
// framesum_arp.h, rank each host's requests in batch order, resolve each query by its lowest matching
// reply, and build the replies and the flagged who-has frames.
//
// The launches on the caller's stream, none of which waits on another workgroup or wave of its own
// launch, every loop bounded by a count known at its start:
//   init      one lane per host, query and reply slot: the out record of a host without a request, a
//             query's winner (none) and reply count (0), a slot's frame (none).
//   classify  one lane per frame: the verdict, and for a candidate its destination MAC and its 28 header
//             bytes, byte by byte (any alignment, nothing outside the frame's own bytes), the probes of the
//             two staged tables; arp_code and arp_of; a matched request's rank key host << b | frame (all
//             ones otherwise); a matched reply's atomic minimum of the batch index and its count (integer
//             atomics: their order changes nothing).
//   sort      the UDP call's rank_sort_keys over the low b + index_bits(n_hosts) bits.
//   assign    one lane per sorted position: the binary search for the host's first position gives the rank,
//             the rank the slot (FS_ARP_ANSWERED, the slot's frame and host) or FS_ARP_FULL; the host's last
//             position writes its counts, its first position `first`.
//   resolve   one lane per query: the winner's HardwareSender, the out record, the winner's FS_ARP_RESOLVED.
//   build     four lanes per frame slot, the TX frame build's tables in LDS (framesum_tx_dev.h): the frame's
//             fifteen words in registers, each lane's 16 bytes as one store (8 + 4 or 8 + 2 at the frame's
//             end), each lane's CRC piece advanced to the frame's end and XORed together, the FCS, the
//             digest and the verdict. A workgroup none of whose slots takes a frame builds no tables.
// With no host listed only classify runs (it then writes arp_code and arp_of and nothing else).
#include <hip/hip_runtime.h>

#include "../../include/framesum_arp.h"
#include "framesum_arp.h"
#include "framesum_coalesce.h"
#include "framesum_coalesce_dev.h"
#include "framesum_flows.h"
#include "framesum_internal.h"
#include "framesum_tx_dev.h"

namespace framesum {

namespace {

using namespace codev;
namespace ar = arp;

struct ArArgs {
    const uint8_t* frames;
    const uint64_t* offsets;
    const uint8_t* status;
    ar::Tables t;  // the staged block
    // this call's own scratch
    uint64_t* rank_in;
    const uint64_t* rank_sorted;
    uint32_t* slot_frame;  // per reply slot: the request it answers, or none
    uint32_t* slot_host;   // per reply slot with a frame: its host
    uint32_t* win;         // per query: the lowest batch index of a matching reply, or none
    uint32_t* n_rep;       // per query: its matching replies
    // the results
    fs_arp_host_out* hosts_out;
    fs_arp_query_out* queries_out;
    uint8_t* arp_frames;
    uint2* arp_out;
    uint8_t* arp_status;
    uint8_t* arp_code;
    uint32_t* arp_of;
    const SegTables* tables;
    uint32_t n, n_blocks, n_reply_slots, arp_flags, mtu, b, lb;
};

__global__ void __launch_bounds__(kThreads) arp_init(const ArArgs a, uint32_t n_items) {
    const uint32_t n_blocks = (n_items + kScanBlock - 1u) / kScanBlock;
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint32_t k = blk * kScanBlock + threadIdx.x;
        if (k < a.t.n_hosts) a.hosts_out[k] = ar::host_out(a.t.hosts[k], 0u, ar::kNoArp);
        if (k < a.t.n_queries) a.win[k] = ar::kNoArp, a.n_rep[k] = 0u;
        if (k < a.n_reply_slots) a.slot_frame[k] = ar::kNoArp;
    }
}

__global__ void __launch_bounds__(kThreads) arp_classify(const ArArgs a) {
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t i = blk * kScanBlock + threadIdx.x;
        if (i >= a.n) continue;
        const bool candidate = a.status[i] == FS_ARP;
        // (a candidate holds its 42 bytes: the verdict says so; the pointer is not formed otherwise)
        const ar::Class c = ar::classify(a.t, candidate ? a.frames + a.offsets[i] : nullptr, candidate);
        if (a.arp_code) a.arp_code[i] = (uint8_t)c.code;
        if (a.arp_of) a.arp_of[i] = c.of;
        if (a.rank_in) a.rank_in[i] = c.host < a.t.n_hosts ? ar::rank_key(c.host, i, a.b) : ar::kUnmatched;
        if (c.of < a.t.n_queries) {
            atomicMin(&a.win[c.of], i);
            atomicAdd(&a.n_rep[c.of], 1u);
        }
    }
}

__global__ void __launch_bounds__(kThreads) arp_assign(const ArArgs a) {
    const uint64_t mask = ((uint64_t)1 << (a.b + a.lb)) - 1u;
    for (uint32_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const uint32_t pos = blk * kScanBlock + threadIdx.x;
        if (pos >= a.n) continue;
        const uint64_t rk = a.rank_sorted[pos];
        if (rk == ar::kUnmatched) continue;
        const uint32_t h = ar::rank_port(rk, a.b), i = ar::rank_frame(rk, a.b);
        if (h >= a.t.n_hosts || i >= a.n) continue;  // (classify writes no other key)
        const fs_arp_host host = a.t.hosts[h];
        const uint32_t rank = pos - ar::lower_bound(a.rank_sorted, a.n, (uint64_t)h << a.b, mask);
        const uint32_t slot = ar::slot_of_rank(host, rank);
        if (slot < a.n_reply_slots) {  // (the host's checks keep every slot of a range below it)
            a.slot_frame[slot] = i, a.slot_host[slot] = h;
            if (a.arp_of) a.arp_of[i] = slot;
        } else if (a.arp_code) {
            a.arp_code[i] = (uint8_t)FS_ARP_FULL;
        }
        const uint64_t after = pos + 1u < a.n ? a.rank_sorted[pos + 1u] : ar::kUnmatched;
        fs_arp_host_out* const o = a.hosts_out + h;
        if (rank == 0u) o->first = i;
        if (after == ar::kUnmatched || ar::rank_port(after, a.b) != h) {  // the host's last request
            const fs_arp_host_out r = ar::host_out(host, rank + 1u, 0u);
            o->n_requests = r.n_requests, o->n_answered = r.n_answered, o->free = r.free;
        }
    }
}

__global__ void __launch_bounds__(kThreads) arp_resolve(const ArArgs a) {
    const uint32_t n_blocks = (a.t.n_queries + kScanBlock - 1u) / kScanBlock;
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint32_t q = blk * kScanBlock + threadIdx.x;
        if (q >= a.t.n_queries) continue;
        const uint32_t w = a.win[q];
        const bool won = w < a.n;
        ar::Mac sha{0u, 0u};
        if (won) sha = ar::mac_of(a.frames + a.offsets[w] + 22);  // (a matched reply is a candidate: it holds its 42 bytes)
        a.queries_out[q] = ar::query_out(a.t.queries[q], won ? w : ar::kNoArp, sha, a.n_rep[q]);
        if (won && a.arp_code) a.arp_code[w] = (uint8_t)FS_ARP_RESOLVED;
    }
}

// ---- The frames. Four lanes per slot, 192 slots per workgroup at a time.
constexpr uint32_t kBuildLanes = 4, kBuildTile = (uint32_t)txdev::kThreads / kBuildLanes;

// What slot `j` takes: false where it takes no frame.
__device__ __forceinline__ bool build_job(const ArArgs& a, uint32_t j, ar::Fields& f) {
    if (j < a.n_reply_slots) {
        const uint32_t i = a.slot_frame[j];
        if (i >= a.n) return false;
        const uint32_t h = a.slot_host[j];
        if (h >= a.t.n_hosts) return false;  // (assign writes no such host)
        f = ar::reply_fields(a.t.hosts[h], ar::parse(a.frames + a.offsets[i]));
        return true;
    }
    const fs_arp_query q = a.t.queries[j - a.n_reply_slots];
    if (!(q.flags & FS_ARP_SEND_REQUEST) || q.host >= a.t.n_hosts) return false;
    f = ar::request_fields(a.t.hosts[q.host], q);
    return true;
}

template <bool kPad>
__global__ void __launch_bounds__(txdev::kThreads) arp_build(const ArArgs a) {
    constexpr uint32_t L = kPad ? ar::kFramePadded : ar::kFrame;
    const uint32_t sub = threadIdx.x & (kBuildLanes - 1u), grp = threadIdx.x / kBuildLanes;
    const uint32_t n_jobs = a.n_reply_slots + a.t.n_queries;
    const uint32_t n_tiles = (n_jobs + kBuildTile - 1u) / kBuildTile;
    int mine = 0;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t j = tile * kBuildTile + grp;
        ar::Fields f;
        if (j < n_jobs && build_job(a, j, f)) mine = 1;
    }
    if (!__syncthreads_or(mine)) return;
    txdev::load_tables(a.tables);
    const uint32_t fcs = (a.arp_flags & FS_FCS_APPEND) ? 4u : 0u;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t j = tile * kBuildTile + grp;
        ar::Fields f;
        if (j >= n_jobs || !build_job(a, j, f)) continue;  // (the same for the four lanes of a slot)
        uint32_t w[ar::kFrameWords + 1];
        ar::frame_words(f, w);
        w[ar::kFrameWords] = 0u;
        uint8_t* __restrict__ dst = a.arp_frames + (uint64_t)j * FS_ACCEPT_STRIDE;
        // ---- this lane's 16 frame bytes (fewer at the frame's end)
        uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            s0 = sub == (uint32_t)q ? w[4 * q] : s0, s1 = sub == (uint32_t)q ? w[4 * q + 1] : s1;
            s2 = sub == (uint32_t)q ? w[4 * q + 2] : s2, s3 = sub == (uint32_t)q ? w[4 * q + 3] : s3;
        }
        const uint32_t at = 16u * sub, left = L > at ? L - at : 0u;
        if (left >= 16u) {
            Piece p;
            p.d[0] = s0, p.d[1] = s1, p.d[2] = s2, p.d[3] = s3;
            *reinterpret_cast<Piece*>(dst + at) = p;
        } else if (left >= 8u) {  // 12 (60 - 48) or 10 (42 - 32)
            store_at<uint64_t>(dst + at, s0 | ((uint64_t)s1 << 32));
            if (left == 12u) store_at<uint32_t>(dst + at + 8u, s2);
            else store_at<uint16_t>(dst + at + 8u, (uint16_t)s2);
        }
        // ---- the CRC: the frame behind 64 - L zeros as four 16-byte pieces, the first four frame bytes
        // inverted (the register's 0xFFFFFFFF start), each lane's piece advanced over the bytes behind it
        uint32_t img[16];
        if (kPad) {
            img[0] = 0u;
#pragma unroll
            for (int d = 1; d < 16; ++d) img[d] = w[d - 1];
            img[1] ^= 0xFFFFFFFFu;
        } else {
#pragma unroll
            for (int d = 0; d < 5; ++d) img[d] = 0u;
            img[5] = w[0] << 16;
#pragma unroll
            for (int d = 6; d < 16; ++d) img[d] = (w[d - 6] >> 16) | (w[d - 5] << 16);
            img[5] ^= 0xFFFF0000u, img[6] ^= 0x0000FFFFu;
        }
        uint32_t d0 = 0, d1 = 0, d2 = 0, d3 = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            d0 = sub == (uint32_t)q ? img[4 * q] : d0, d1 = sub == (uint32_t)q ? img[4 * q + 1] : d1;
            d2 = sub == (uint32_t)q ? img[4 * q + 2] : d2, d3 = sub == (uint32_t)q ? img[4 * q + 3] : d3;
        }
        uint32_t hs = txdev::crc_piece(d0, d1, d2, d3);
        if (sub == 2u || sub == 0u) hs = txdev::zshift(4, hs);
        if (sub <= 1u) hs = txdev::zshift(5, hs);
        hs ^= __shfl_xor(hs, 1, 64);
        hs ^= __shfl_xor(hs, 2, 64);
        const uint32_t crc = ~hs;
        if (sub == 3u && fcs) store_at<uint32_t>(dst + L, crc);
        if (sub == 0u) {
            const uint32_t verdict = ar::built_verdict(L, a.mtu);
            if (a.arp_out) a.arp_out[j] = make_uint2(crc, verdict == ar::kArpVerdict ? ar::ip_csum_of(w) : 0u);
            if (a.arp_status) a.arp_status[j] = (uint8_t)verdict;
        }
    }
}

}  // namespace

ArpScratch arp_scratch(uint32_t n, uint32_t n_hosts, uint32_t n_queries, uint32_t n_reply_slots) {
    ArpScratch s;
    size_t sort_bytes = 0;
    // (a null pointer: the sort only reports what it needs)
    if (n != 0 && n_hosts != 0 &&
        rank_sort_keys(nullptr, sort_bytes, nullptr, nullptr, n, arp::rank_bits(flows::index_bits(n), n_hosts), nullptr) != hipSuccess)
        sort_bytes = 0;
    uint64_t at = 0;
    s.rank_in = at, at += 8ull * n;
    s.rank_sorted = at, at += 8ull * n;
    s.slot_frame = at, at += 4ull * n_reply_slots;
    s.slot_host = at, at += 4ull * n_reply_slots;
    s.win = at, at += 4ull * n_queries;
    s.n_rep = at, at += 4ull * n_queries;
    at = (at + 255u) & ~255ull;
    s.sort_temp = at, at += sort_bytes;
    s.sort_bytes = sort_bytes;
    s.bytes = at;
    return s;
}

hipError_t launch_arp(const RxBatch& b, const RxResults& r, const RxArp& x, const RxLeft& left, const uint8_t* d_block,
                      const SegTables* tables, int tx_workgroups, const RxLaunch& how) {
    uint8_t* const scratch = left.arp_scratch;
    const ArpScratch& s = left.ars;
    const uint32_t n = b.n;
    const hipStream_t stream = how.stream;
    const bool listed = x.n_hosts != 0;
    ArArgs a;
    a.frames = b.frames;
    a.offsets = b.offsets;
    a.status = r.status;
    a.t = arp::Tables{};  // (no host: no block, and no lookup reads one)
    if (listed) a.t = arp::tables_of(d_block, arp::block_of(x.n_hosts, x.n_queries), x.n_hosts, x.n_queries, how.hash_mask);
    a.rank_in = listed ? reinterpret_cast<uint64_t*>(scratch + s.rank_in) : nullptr;
    a.rank_sorted = listed ? reinterpret_cast<const uint64_t*>(scratch + s.rank_sorted) : nullptr;
    a.slot_frame = listed ? reinterpret_cast<uint32_t*>(scratch + s.slot_frame) : nullptr;
    a.slot_host = listed ? reinterpret_cast<uint32_t*>(scratch + s.slot_host) : nullptr;
    a.win = listed ? reinterpret_cast<uint32_t*>(scratch + s.win) : nullptr;
    a.n_rep = listed ? reinterpret_cast<uint32_t*>(scratch + s.n_rep) : nullptr;
    a.hosts_out = x.hosts_out;
    a.queries_out = x.queries_out;
    a.arp_frames = x.arp_frames;
    a.arp_out = reinterpret_cast<uint2*>(x.arp_out);
    a.arp_status = x.arp_status;
    a.arp_code = x.arp_code;
    a.arp_of = x.arp_of;
    a.tables = tables;
    a.n = n;
    const ScanGrid g = scan_grid(n, how);
    a.n_blocks = g.blocks;
    a.n_reply_slots = x.n_reply_slots;
    a.arp_flags = x.arp_flags;
    a.mtu = b.mtu;
    a.b = flows::index_bits(n);
    a.lb = flows::index_bits(x.n_hosts);
    if (!listed) {  // rule 1: the codes alone
        if (n != 0 && (a.arp_code || a.arp_of)) hipLaunchKernelGGL(arp_classify, dim3(g.scan), dim3(kThreads), 0, stream, a);
        return hipGetLastError();
    }
    const uint32_t n_items = std::max(std::max(x.n_hosts, x.n_queries), x.n_reply_slots);
    hipLaunchKernelGGL(arp_init, dim3(g.capped((n_items + kScanBlock - 1u) / kScanBlock)), dim3(kThreads), 0, stream, a, n_items);
    if (n != 0) {
        hipLaunchKernelGGL(arp_classify, dim3(g.scan), dim3(kThreads), 0, stream, a);
        size_t sort_bytes = s.sort_bytes;
        const hipError_t e = rank_sort_keys(scratch + s.sort_temp, sort_bytes, a.rank_in, reinterpret_cast<uint64_t*>(scratch + s.rank_sorted),
                                            n, arp::rank_bits(a.b, x.n_hosts), stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(arp_assign, dim3(g.scan), dim3(kThreads), 0, stream, a);
    }
    if (x.n_queries != 0)
        hipLaunchKernelGGL(arp_resolve, dim3(g.capped((x.n_queries + kScanBlock - 1u) / kScanBlock)), dim3(kThreads), 0, stream, a);
    const uint32_t n_jobs = x.n_reply_slots + x.n_queries;
    if (n_jobs != 0) {
        const uint32_t want = (n_jobs + kBuildTile - 1u) / kBuildTile, cap = (uint32_t)(tx_workgroups > 0 ? tx_workgroups : 1);
        const dim3 grid(want < cap ? want : cap);
        if (x.arp_flags & FS_ARP_PAD) hipLaunchKernelGGL(arp_build<true>, grid, dim3(txdev::kThreads), 0, stream, a);
        else hipLaunchKernelGGL(arp_build<false>, grid, dim3(txdev::kThreads), 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace framesum
