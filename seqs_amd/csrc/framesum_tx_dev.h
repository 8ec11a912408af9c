// Device code the two frame-building kernel files share (framesum_segment.hip: fs_segment_batch;
// framesum_send.hip: fs_send_rings_batch): the LDS tables, the piece loads and the store, one frame's
// body, the walk of a wave over its tiles of frames, and the launch arguments -- written once over a
// piece source `Src` that each file supplies. HIP only; the arithmetic is in framesum_segment.h.
//
// One wave builds one frame at a time. Its 64 lanes stream the frame's chunk of the payload in
// 16-byte pieces counted back from the chunk's END: piece p is chunk[C - 16(p+1), C - 16p), lane l
// takes pieces l, l + 64, ... Every piece but the chunk's first is whole, so a lane moves it with
// one 16-byte load at the payload's own alignment and one 16-byte store at the frame's (gfx950
// serves global accesses at any byte address; a store writes exactly its 16 bytes, so two frames
// may share a 64-byte block). The chunk's first 1..15 bytes move as one 8-, 4-, 2- and 1-byte access
// each, zero-padded IN FRONT: leading zeros change neither a zero-initialised CRC nor a
// one's-complement sum.
//   CRC-32: a lane keeps s = Z_1024(s) ^ Z_16(d0) ^ Z_12(d1) ^ Z_8(d2) ^ Z_4(d3) over its pieces
//   (Z_k: the CRC register advanced over k zero bytes, 4 LDS lookups; 1024 = the wave's stride), so
//   its state ends 16 l bytes before the chunk's end; a lane tree (Z_16, Z_32, ... Z_512) brings
//   the 64 states together. The header's register (init 0xFFFFFFFF, 4 lanes x 16 bytes) is advanced
//   over the C chunk bytes by the set bits of C (Z_1 ... Z_32768) and XORed in: CRC-32 is linear.
//   Checksums: the lanes add their pieces' little-endian halfwords; an odd C puts every byte in
//   the other half of its word, which a byte swap of the folded sum undoes (RFC 1071 §2B).
// The frame's 54 or 42 header bytes are built in registers from the record's template (IPv4 ID from
// the staged prand16 powers, Seq, flags, lengths, both checksums), stored one byte per lane, and
// the FCS after the frame by 4 lanes. The payload is read once, each frame byte written once,
// nothing read back.
//
// Src, a family's piece source:
//   Src::Rec                 the staged record (segment::SendRec, send::RingRec: the fields the body
//                            reads lie at the same offsets in both, framesum_send.h asserts it)
//   Src::kMayUdp             may a record be UDP? (false: the kernel has no protocol branch)
//   Src::kMssZero            may mss be 0 (the record is one frame of all its bytes)?
//   Src::total(rec)          the record's byte count
//   Src(a, rec, c0, C)       the source of the chunk [c0, c0 + C) of the record's bytes
//   src.load(e, d)           the piece chunk[e - 16, e) as four little-endian dwords: whole (e >= 16),
//                            the chunk's first e bytes behind 16 - e zeros, or zeros (e <= 0)
#pragma once
#include <hip/hip_runtime.h>

#include "framesum_coalesce_dev.h"
#include "framesum_internal.h"
#include "framesum_segment.h"

namespace framesum {
namespace txdev {
namespace {

using codev::load_at;  // 16 bytes, and loads and stores, at any alignment
using codev::Piece;
using codev::store_at;

// 12 waves per workgroup, two workgroups per CU: the tables (68 KB) fit a CU's LDS twice and the
// kernels' 79 and 76 VGPRs allow 6 waves per SIMD (measured against one 16-wave workgroup per CU: 138 us
// against 150 on the segment_bench.py shape; 8 waves per SIMD spill and ran at 172 us)
constexpr int kThreads = 768;
constexpr int kWaves = kThreads / 64;

// The launch arguments. `src`: the bytes the records' offsets count in (the payload, the rings).
template <typename Rec>
struct Args {
    const Rec* recs;
    const uint32_t* prefix;
    const uint16_t* ids;
    const uint8_t* src;
    uint8_t* frames;
    uint64_t* offsets;
    uint32_t* lengths;
    uint2* out;
    uint8_t* status;
    const SegTables* tables;
    uint32_t n_recs, n_frames, tile, mtu, flags, align;
};

// the 17 tables as [4][256] dwords each (68 KB), built by every workgroup from the 2-KB basis
__shared__ uint32_t g_z[kSegTableCount * 1024];

__device__ __forceinline__ uint32_t zshift(int tab, uint32_t v) {
    const uint32_t* T = g_z + tab * 1024;
    return T[v & 255u] ^ T[256 + ((v >> 8) & 255u)] ^ T[512 + ((v >> 16) & 255u)] ^ T[768 + (v >> 24)];
}
// the zero-init CRC register after the 16 bytes d0..d3
__device__ __forceinline__ uint32_t crc_piece(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3) {
    return zshift(4, d0) ^ zshift((int)kSegTableZ12, d1) ^ zshift(3, d2) ^ zshift(2, d3);
}
__device__ __forceinline__ uint32_t halves(uint32_t d) { return (d & 0xFFFFu) + (d >> 16); }
__device__ __forceinline__ uint32_t fold16(uint32_t s) {
    s = (s & 0xFFFFu) + (s >> 16);
    s = (s & 0xFFFFu) + (s >> 16);
    return s;
}
__device__ __forceinline__ uint32_t swap16(uint32_t x) { return ((x & 0xFFu) << 8) | ((x >> 8) & 0xFFu); }
__device__ __forceinline__ uint32_t prand16(uint32_t x) {
    x = (x ^ (x << 7)) & 0xFFFFu;
    x ^= x >> 9;
    x = (x ^ (x << 8)) & 0xFFFFu;
    return x;
}

// bytes [at, at + 8) of the 16-byte value (lo, hi), for at = 0 or at + width <= 8 or at >= 8
__device__ __forceinline__ uint64_t bytes_at(uint64_t lo, uint64_t hi, int at) {
    return at < 8 ? lo >> (8 * at) : hi >> (8 * (at - 8));
}

// The piece src[e - 16, e) of a linear chunk at `src` as four little-endian dwords: whole (e >= 16),
// the chunk's first e bytes behind 16 - e zeros (0 < e < 16), or nothing (e <= 0: zeros). The e head
// bytes move as one 8-, 4-, 2- and 1-byte access each (the bits of e), never past the chunk.
__device__ __forceinline__ void load_linear(const uint8_t* __restrict__ src, int e, uint32_t d[4]) {
    d[0] = d[1] = d[2] = d[3] = 0;
    if (e >= 16) {
        const Piece p = *reinterpret_cast<const Piece*>(src + (e - 16));
        d[0] = p.d[0];
        d[1] = p.d[1];
        d[2] = p.d[2];
        d[3] = p.d[3];
    } else if (e > 0) {
        const int p4 = e & 8, p2 = e & 12, p1 = e & 14;
        const uint64_t v8 = (e & 8) ? load_at<uint64_t>(src) : 0ull;
        const uint64_t v4 = (e & 4) ? load_at<uint32_t>(src + p4) : 0u;
        const uint64_t v2 = (e & 2) ? load_at<uint16_t>(src + p2) : 0u;
        const uint64_t v1 = (e & 1) ? src[p1] : 0u;
        // the head bytes at the low end: (lo, hi) = chunk[0, e)
        uint64_t lo = v8, hi = 0;
        if (p4) hi |= v4; else lo |= v4;
        if (p2 >= 8) hi |= v2 << (8 * (p2 - 8)); else lo |= v2 << (8 * p2);
        if (p1 >= 8) hi |= v1 << (8 * (p1 - 8)); else lo |= v1 << (8 * p1);
        // ... moved up by n = 16 - e bytes
        const int n = 16 - e;
        if (n >= 8) {
            hi = lo << (8 * (n - 8));
            lo = 0;
        } else {
            hi = (hi << (8 * n)) | (lo >> (64 - 8 * n));
            lo <<= 8 * n;
        }
        d[0] = (uint32_t)lo;
        d[1] = (uint32_t)(lo >> 32);
        d[2] = (uint32_t)hi;
        d[3] = (uint32_t)(hi >> 32);
    }
}
// The same piece of a chunk that starts at `src` inside a ring and has `w` bytes before the ring's end
// (`past` = src - ring_size: chunk byte j >= w lies at past + j). w = INT_MAX for a chunk that does
// not wrap.
__device__ __forceinline__ void load_ring(const uint8_t* __restrict__ src, const uint8_t* __restrict__ past, int w, int e,
                                          uint32_t d[4]) {
    if (e <= w || e - 16 >= w) {
        // wholly before the end (and e <= 0: zeros), or wholly behind it (e >= 17: a whole piece)
        load_linear(e <= w ? src : past, e, d);
    } else {
        // the piece that straddles the ring's end; byte b of the 16 is chunk[e - 16 + b], zeros in front
        uint64_t lo = 0, hi = 0;
#pragma unroll 1  // (a rare path: kept small, so that it costs the common one no registers)
        for (int b = 0; b < 16; ++b) {
            const int j = e - 16 + b;
            if (j < 0) continue;
            const uint64_t v = j < w ? src[j] : past[j];
            if (b < 8) lo |= v << (8 * b);
            else hi |= v << (8 * (b - 8));
        }
        d[0] = (uint32_t)lo;
        d[1] = (uint32_t)(lo >> 32);
        d[2] = (uint32_t)hi;
        d[3] = (uint32_t)(hi >> 32);
    }
}
// ... and a piece's bytes to out[e - 16, e) (clipped at out[0]); exactly those bytes are written
__device__ __forceinline__ void store_piece(uint8_t* __restrict__ out, int e, const uint32_t d[4]) {
    if (e >= 16) {
        Piece p;
        p.d[0] = d[0];
        p.d[1] = d[1];
        p.d[2] = d[2];
        p.d[3] = d[3];
        *reinterpret_cast<Piece*>(out + (e - 16)) = p;
    } else if (e > 0) {
        uint64_t lo = d[0] | ((uint64_t)d[1] << 32), hi = d[2] | ((uint64_t)d[3] << 32);
        const int n = 16 - e;  // back down: (lo, hi) = chunk[0, e)
        if (n >= 8) {
            lo = hi >> (8 * (n - 8));
            hi = 0;
        } else {
            lo = (lo >> (8 * n)) | (hi << (64 - 8 * n));
            hi >>= 8 * n;
        }
        const int p4 = e & 8, p2 = e & 12, p1 = e & 14;
        if (e & 8) store_at<uint64_t>(out, lo);
        if (e & 4) store_at<uint32_t>(out + p4, (uint32_t)bytes_at(lo, hi, p4));
        if (e & 2) store_at<uint16_t>(out + p2, (uint16_t)bytes_at(lo, hi, p2));
        if (e & 1) out[p1] = (uint8_t)bytes_at(lo, hi, p1);
    }
}

// One frame, by one wave. h[i] = the header's i-th halfword as a little-endian load sees it.
template <bool kUdp, typename Src>
__device__ __forceinline__ void build_frame(const Args<typename Src::Rec>& a, const typename Src::Rec* rec, uint32_t k,
                                            uint32_t id, uint32_t frame, uint32_t lane) {
    constexpr uint32_t H = kUdp ? segment::kUdpHdr : segment::kTcpHdr;
    constexpr int NH = H / 2;            // header halfwords
    constexpr int PADH = (64 - H) / 2;   // halfwords of zeros in front of them in the 64-byte image
    const uint32_t* rw = reinterpret_cast<const uint32_t*>(rec);
    uint32_t h[27];
#pragma unroll
    for (int i = 0; i < 27; ++i) h[i] = (rw[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
    const uint32_t mss = rec->mss, L = Src::total(rec), S = rec->frames;
    const uint32_t c0 = k * mss;  // (mss == 0: one frame, k == 0; a ring: <= data <= ring_size <= 2^31)
    const uint32_t C = Src::kMssZero && mss == 0 ? L : (L - c0 < mss ? L - c0 : mss);
    const uint32_t len = H + C;
    const uint32_t fcs = (a.flags & FS_FCS_APPEND) ? 4u : 0u;
    const uint64_t slot = ((uint64_t)(H + mss) + fcs + (a.align - 1)) & ~(uint64_t)(a.align - 1);
    const uint64_t off = rec->frame_base + (uint64_t)k * slot;
    const Src src(a, rec, c0, C);
    uint8_t* __restrict__ dst = a.frames + off;

    // ---- the chunk: 16-byte pieces from its end, lane l pieces l, l + 64, ... Two pieces are loaded
    // before either is stored, so that a frame of up to 2 KB pays one load latency.
    const uint32_t D = (C + 15u) >> 4, J = (D + 63u) >> 6;
    uint32_t s = 0, acc = 0;
    for (uint32_t j = J; j > 0;) {
        const bool two = j >= 2;
        const int ea = (int)C - 16 * (int)(lane + 64u * (j - 1));  // the piece is chunk[e - 16, e)
        const int eb = two ? ea + 1024 : 0;
        uint32_t da[4], db[4];
        src.load(ea, da);
        src.load(eb, db);
        store_piece(dst + H, ea, da);
        store_piece(dst + H, eb, db);
        if (j < J) s = zshift(10, s);
        if (ea > 0) {
            s ^= crc_piece(da[0], da[1], da[2], da[3]);
            acc += halves(da[0]) + halves(da[1]) + halves(da[2]) + halves(da[3]);
        }
        if (two) {
            s = zshift(10, s);
            s ^= crc_piece(db[0], db[1], db[2], db[3]);  // (below the top level every lane's piece is whole)
            acc += halves(db[0]) + halves(db[1]) + halves(db[2]) + halves(db[3]);
        }
        j -= two ? 2u : 1u;
    }
    // lane tree: level t folds lanes whose bit t is set (16 * 2^t bytes further from the end)
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        if ((lane & ((2u << t) - 1u)) == (1u << t)) s = zshift(4 + t, s);
        s ^= __shfl_xor(s, 1 << t, 64);
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 64);
    const uint32_t chunk_crc = __builtin_amdgcn_readfirstlane(s);
    uint32_t csum = fold16(__builtin_amdgcn_readfirstlane(acc));
    if (C & 1u) csum = swap16(csum);

    // ---- the header fields of frame k (everything else is the record's template)
    h[7] = (h[7] & 0xFF00u) | 0x45u;
    h[8] = swap16(H - 14 + C);
    h[9] = swap16(id);
    h[12] = 0;
    uint32_t l4 = h[13] + h[14] + h[15] + h[16] + h[17] + h[18] + csum;
    if (kUdp) {
        h[19] = swap16(8u + L);
        h[20] = 0;
        l4 += swap16(17u) + h[19] + h[19];
    } else {
        const uint32_t seq = __builtin_bswap32(h[19] | (h[20] << 16)) + c0;
        const uint32_t sw = __builtin_bswap32(seq);
        h[19] = sw & 0xFFFFu;
        h[20] = sw >> 16;
        if (k + 1 != S) h[23] &= ~0x0900u;  // FIN and PSH only on the last segment
        h[25] = 0;
        h[26] = 0;
        l4 += swap16(6u) + swap16(20u + C) + h[19] + h[20] + h[21] + h[22] + h[23] + h[24];
    }
    uint32_t ip = 0;
#pragma unroll
    for (int i = 7; i < 17; ++i) ip += h[i];
    const uint32_t ipc = ~fold16(ip) & 0xFFFFu, l4c = ~fold16(l4) & 0xFFFFu;
    // RecvEth's gates on the built frame (stacks/portstack.go:167-214, :226-237, :285-299)
    uint32_t verdict = FS_OK;
    if (a.mtu && len > a.mtu) verdict = FS_ERR_EXCEEDS_MTU;
    else if (((len) & 0xFFFFu) < 34u) verdict = FS_ERR_BAD_IP_TOTAL_LEN_OR_IHL;  // uint16 `end` wrapped
    else if (h[17] == 0 || h[18] == 0) verdict = FS_ERR_ZERO_PORT;
    const bool early = a.mtu && len > a.mtu;
    if (verdict == FS_OK) {
        h[12] = ipc;
        h[kUdp ? 20 : 25] = l4c;
    }

    // ---- the 64-byte image: zeros, then the header; stored one byte per lane
    uint32_t img[16];
#pragma unroll
    for (int d = 0; d < 16; ++d) {
        const int x0 = 2 * d - PADH, x1 = 2 * d + 1 - PADH;
        img[d] = (x0 >= 0 && x0 < NH ? h[x0 < 0 ? 0 : x0] : 0u) | ((x1 >= 0 && x1 < NH ? h[x1 < 0 ? 0 : x1] : 0u) << 16);
    }
    if (lane < H) {
        const uint32_t at = 64 - H + lane;
        uint32_t w = 0;
#pragma unroll
        for (int d = 0; d < 16; ++d) w = (at >> 2) == (uint32_t)d ? img[d] : w;
        dst[lane] = (uint8_t)(w >> (8 * (at & 3u)));
    }
    // ---- its CRC register (init 0xFFFFFFFF = the first four bytes inverted), 4 lanes x 16 bytes
    uint32_t hs = 0;
    if (lane < 4) {
        img[PADH / 2] ^= 0xFFFF0000u;  // (PADH is odd: the header starts in a dword's upper half)
        img[PADH / 2 + 1] ^= 0x0000FFFFu;
        uint32_t d0 = 0, d1 = 0, d2 = 0, d3 = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            d0 = lane == (uint32_t)q ? img[4 * q] : d0;
            d1 = lane == (uint32_t)q ? img[4 * q + 1] : d1;
            d2 = lane == (uint32_t)q ? img[4 * q + 2] : d2;
            d3 = lane == (uint32_t)q ? img[4 * q + 3] : d3;
        }
        hs = crc_piece(d0, d1, d2, d3);
        if (lane == 2 || lane == 0) hs = zshift(4, hs);
        if (lane <= 1) hs = zshift(5, hs);
    }
    hs ^= __shfl_xor(hs, 1, 64);
    hs ^= __shfl_xor(hs, 2, 64);
    hs = __builtin_amdgcn_readfirstlane(hs);
    if (lane < 4) {
        for (int b = 0; b < 16; ++b)
            if (C & (1u << b)) hs = zshift(b, hs);
        const uint32_t crc = ~(hs ^ chunk_crc);
        if (fcs) dst[len + lane] = (uint8_t)(crc >> (8 * lane));
        if (lane == 0) {
            if (a.offsets) a.offsets[frame] = off;
            if (a.lengths) a.lengths[frame] = len;
            if (a.out) a.out[frame] = make_uint2(crc, early ? 0u : (swap16(ipc) | (verdict == FS_OK ? swap16(l4c) << 16 : 0u)));
            if (a.status) a.status[frame] = (uint8_t)verdict;
        }
    }
}

// The tables into LDS, from their basis: entry v of a table is the XOR of the basis entries of v's bits.
// Every kernel that runs build_frame starts with this (the accept call's SYN-ACK kernel too,
// framesum_accept.hip).
__device__ __forceinline__ void load_tables(const SegTables* tables) {
    for (uint32_t e = threadIdx.x; e < kSegTableCount * 1024u; e += kThreads) {
        const uint32_t* basis = &tables->basis[0][0][0] + (e >> 8) * 8;
        uint32_t r = 0;
#pragma unroll
        for (int jb = 0; jb < 8; ++jb) r ^= (e & (1u << jb)) ? basis[jb] : 0u;
        g_z[e] = r;
    }
    __syncthreads();
}

// A whole kernel: the tables into LDS, then every wave builds its tiles' frames back to back.
template <typename Src>
__device__ __forceinline__ void build_frames(const Args<typename Src::Rec>& a) {
    load_tables(a.tables);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t n_tiles = (a.n_frames + a.tile - 1) / a.tile;
    for (uint32_t tile = blockIdx.x * kWaves + wave; tile < n_tiles; tile += gridDim.x * kWaves) {
        uint32_t f = tile * a.tile;
        const uint32_t f_end = a.n_frames - f < a.tile ? a.n_frames : f + a.tile;
        // frame -> record: segment::find_send, one probe per lane
        uint32_t lo = 0, hi = a.n_recs;
        while (hi - lo > 1) {
            const uint32_t step = (hi - lo + 63u) / 64u;
            const uint64_t idx = (uint64_t)lo + (uint64_t)lane * step;
            const bool ok = idx < hi && a.prefix[idx] <= f;
            const uint32_t cnt = (uint32_t)__popcll(__ballot(ok));
            lo += (cnt - 1) * step;
            hi = hi - lo < step ? hi : lo + step;
        }
        uint32_t r = __builtin_amdgcn_readfirstlane(lo);
        uint32_t k = f - a.prefix[r];
        const typename Src::Rec* rec = a.recs + r;
        uint32_t id = a.ids[rec->id_at + k / segment::kIdStride];
        for (uint32_t j = k % segment::kIdStride; j > 0; --j) id = prand16(id);
        for (; f < f_end; ++f) {
            if (Src::kMayUdp && __builtin_amdgcn_readfirstlane((uint32_t)rec->hdr[23]) == 17)
                build_frame<true, Src>(a, rec, k, id, f, lane);
            else
                build_frame<false, Src>(a, rec, k, id, f, lane);
            ++k;
            id = prand16(id);
            if (k == rec->frames && f + 1 < f_end) {
                ++r;
                rec = a.recs + r;
                k = 0;
                id = ((uint32_t)rec->hdr[18] << 8) | rec->hdr[19];
            }
        }
    }
}

// The launch arguments of a staged batch (`d_block`: the device copy of the block a family's stage()
// filled, `b` its layout), and the grid: no more workgroups than `workgroups`, nor than there are
// tiles of one frame each for their waves.
template <typename Rec>
uint32_t fill_args(Args<Rec>& a, const uint8_t* d_block, const segment::Block& b, uint32_t n_recs, uint32_t n_frames,
                   const uint8_t* src, uint8_t* frames, uint64_t* offsets, uint32_t* lengths, void* out, uint8_t* status,
                   uint32_t mtu, uint32_t flags, uint32_t align, const SegTables* tables, int workgroups) {
    a.recs = reinterpret_cast<const Rec*>(d_block + b.recs_at);
    a.prefix = reinterpret_cast<const uint32_t*>(d_block + b.prefix_at);
    a.ids = reinterpret_cast<const uint16_t*>(d_block + b.ids_at);
    a.src = src;
    a.frames = frames;
    a.offsets = offsets;
    a.lengths = lengths;
    a.out = static_cast<uint2*>(out);
    a.status = status;
    a.tables = tables;
    a.n_recs = n_recs;
    a.n_frames = n_frames;
    a.mtu = mtu;
    a.flags = flags;
    a.align = align;
    const uint64_t want = ((uint64_t)n_frames + kWaves - 1) / kWaves;
    const uint32_t grid = (uint32_t)(want < (uint64_t)workgroups ? want : (uint64_t)workgroups);
    a.tile = segment::tile_frames(n_frames, grid * kWaves);
    return grid;
}

}  // namespace
}  // namespace txdev
}  // namespace framesum
