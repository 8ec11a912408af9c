// Host-logic checks of seqs_amd/csrc/framesum_plan.h, built on its own under ASan + UBSan
// (tests/csrc/Makefile, run by tests/test_host_sanitizers.py): the chunks of the
// host-staged path, the blocks of fs_digest_batch_multi and the round-robin shard / gather /
// de-interleave maps, on random batches that are in order, shuffled, sparse, overlapping,
// empty, zero-length, huge-offset, and with more contexts than frames; and the description of the
// RX host forms' device result arrays, for every call kind up to 2^30 frames.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../seqs_amd/csrc/framesum_plan.h"

using namespace framesum::plan;

static int g_fail = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            if (++g_fail > 20) std::exit(1);                                  \
        }                                                                     \
    } while (0)

struct Batch {
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    uint64_t bytes = 0;
};

static Batch make_batch(std::mt19937_64& rng, uint32_t n, int kind) {
    Batch b;
    b.off.resize(n);
    b.len.resize(n);
    uint64_t pos = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t L = kind == 3 ? 0u : (uint32_t)(rng() % 9100);
        b.len[i] = L;
        if (kind == 2 && rng() % 4 == 0) pos += rng() % (64u << 20);  // sparse: big gaps
        b.off[i] = pos;
        pos += (L + 3) & ~3u;
        if (kind == 4 && i > 0 && rng() % 3 == 0) b.off[i] = b.off[rng() % i];  // overlapping / repeated
    }
    b.bytes = pos + 16;
    if (kind == 1) {  // shuffled: offsets not in index order
        for (uint32_t i = n; i > 1; --i) {
            const uint32_t j = (uint32_t)(rng() % i);
            std::swap(b.off[i - 1], b.off[j]);
            std::swap(b.len[i - 1], b.len[j]);
        }
    }
    return b;
}

static void check_chunks(const Batch& b, uint64_t chunk_bytes, uint32_t chunk_frames) {
    const uint32_t n = (uint32_t)b.len.size();
    CHECK(first_frame_out_of_range(b.off.data(), b.len.data(), n, b.bytes) == n);
    {   // the one-pass scan of the host-staged call: in range, longest frame, byte span
        const Scan sc = scan_batch(b.off.data(), b.len.data(), n, b.bytes);
        uint64_t lo = UINT64_MAX, hi = 0;
        uint32_t mx = 0;
        for (uint32_t i = 0; i < n; ++i) {
            lo = std::min(lo, b.off[i]);
            hi = std::max(hi, b.off[i] + b.len[i]);
            mx = std::max(mx, b.len[i]);
        }
        CHECK(sc.bad == n && sc.max_len == mx && sc.hi == hi && sc.lo == (n ? lo : 0));
    }
    std::vector<Chunk> ch;
    host_chunks(b.off.data(), b.len.data(), n, b.bytes, chunk_bytes, chunk_frames, ch);
    uint32_t next = 0;
    for (const Chunk& c : ch) {
        CHECK(c.c0 == next && c.c1 > c.c0 && c.c1 <= n);
        CHECK(c.cpy_lo % 16 == 0 && c.cpy_lo <= c.cpy_hi && c.cpy_hi <= b.bytes);
        uint64_t lo = UINT64_MAX, hi = 0;
        for (uint32_t i = c.c0; i < c.c1; ++i) {
            // every byte the engine may touch for frame i lies in the staged copy: 12 B before
            // its start (or the buffer start) up to its dword-rounded end (or the buffer end)
            const uint64_t s = b.off[i], e = s + b.len[i];
            CHECK(c.cpy_lo <= (s >= 12 ? s - 12 : 0));
            CHECK(std::min<uint64_t>((e + 3) & ~uint64_t(3), b.bytes) <= c.cpy_hi);
            lo = std::min(lo, s);
            hi = std::max(hi, e);
        }
        const bool single = c.c1 - c.c0 == 1, rest = c.c1 == n;
        CHECK(single || rest || hi - lo <= chunk_bytes);
        CHECK(c.c1 - c.c0 <= chunk_frames || rest);
        next = c.c1;
    }
    CHECK(next == n);
}

static void check_multi(const Batch& b, int nctx) {
    const uint32_t n = (uint32_t)b.len.size();
    MultiPlan p;
    multi_blocks(b.off.data(), b.len.data(), n, nctx, p);
    CHECK((int)p.cut.size() == nctx + 1 && p.cut[0] == 0 && p.cut[nctx] == n);
    for (int k = 0; k < nctx; ++k) CHECK(p.cut[k] <= p.cut[k + 1]);
    std::vector<uint8_t> seen(n, 0);
    uint64_t total = 0, maxlen = 0;
    for (uint32_t pos = 0; pos < n; ++pos) {
        const uint32_t f = p.frame(pos);
        CHECK(f < n);
        if (f < n) seen[f]++;
        if (pos > 0) CHECK(b.off[p.frame(pos - 1)] <= b.off[f]);  // buffer order inside every block
        total += b.len[f];
        maxlen = std::max<uint64_t>(maxlen, b.len[f]);
    }
    for (uint32_t i = 0; i < n; ++i) CHECK(seen[i] == 1);  // a permutation
    for (int k = 0; k < nctx; ++k) {
        uint64_t bytes = 0;
        for (uint32_t pos = p.cut[k]; pos < p.cut[k + 1]; ++pos) bytes += b.len[p.frame(pos)];
        CHECK(bytes * (uint64_t)nctx <= total + (uint64_t)nctx * maxlen);  // byte balance
    }
}

// A batch moved up by `base` bytes (the buffer grows by as much), and one whose odd frames alone move
// up: offsets then alternate between the two sides of `base`, unordered.
static Batch moved(Batch b, uint64_t base, bool odd_only = false) {
    for (size_t i = 0; i < b.off.size(); ++i)
        if (!odd_only || (i & 1)) b.off[i] += base;
    b.bytes += base;
    return b;
}

// Offsets around and above 2^32 (the ABI's offsets are 64-bit so that batches beyond 4 GiB work): the
// same invariants as below 2^32, and the exact values of the span arithmetic.
static void check_high_offsets(std::mt19937_64& rng) {
    const uint64_t G = uint64_t(1) << 32;
    for (int kind = 0; kind < 5; ++kind)
        for (uint32_t n : {1u, 2u, 65u, 1000u})
            for (uint64_t cb : {uint64_t(4096), uint64_t(16) << 20}) {
                const Batch b = make_batch(rng, n, kind);
                const uint64_t span = std::min<uint64_t>(b.bytes - 16, G);  // (a sparse batch can be longer)
                // lo above 2^32; the span crossing 2^32 (in its middle, one byte in, one byte before its
                // end); the two sides alternating
                for (uint64_t base : {G + 12345 * 4, G + 1, 3 * G - 4, G - span / 2, G - 1, G - (span ? span - 1 : 0)}) {
                    check_chunks(moved(b, base), cb, kind == 0 ? 100u : (1u << 20));
                    for (int nctx : {1, 2, 3}) check_multi(moved(b, base), nctx);
                }
                check_chunks(moved(b, G + 4096, true), cb, 1u << 20);
                for (int nctx : {2, 3}) check_multi(moved(b, G + 4096, true), nctx);
            }
    {   // scan_batch and first_frame_out_of_range with every number above 2^32
        std::vector<uint64_t> off = {G + 500, G + 100, 3 * G + 7, G + 50};
        std::vector<uint32_t> len = {10, 20, 10, 10};
        const Scan sc = scan_batch(off.data(), len.data(), 4, 3 * G + 17);
        CHECK(sc.bad == 4 && sc.lo == G + 50 && sc.hi == 3 * G + 17 && sc.max_len == 20 && sc.min_len == 10);
        CHECK(scan_batch(off.data(), len.data(), 4, 3 * G + 16).bad == 2);  // one byte past the buffer
        CHECK(first_frame_out_of_range(off.data(), len.data(), 4, 3 * G + 17) == 4);
        CHECK(first_frame_out_of_range(off.data(), len.data(), 4, 3 * G + 16) == 2);
        CHECK(first_frame_out_of_range(off.data(), len.data(), 4, 3 * G + 20, 4) == 2);  // ... with the FCS room
        CHECK(scan_batch(off.data(), len.data(), 4, 3 * G + 20, 4).bad == 2);
        CHECK(scan_batch(off.data(), len.data(), 4, 3 * G + 21, 4).bad == 4);
        CHECK(scan_batch(off.data(), len.data(), 2, G + 509).bad == 0);
        CHECK(scan_batch(off.data(), len.data(), 2, G + 510).bad == 2);
        // a buffer that ends below 2^32 holds none of them, whatever their low halves say
        CHECK(scan_batch(off.data(), len.data(), 4, 100000).bad == 0);
        CHECK(first_frame_out_of_range(off.data() + 1, len.data() + 1, 3, G - 1) == 0);
        // offsets near 2^64: offset + length wraps to a small number and must not pass the range check
        std::vector<uint64_t> wrap = {G + 5, UINT64_MAX - 2, G + 9, UINT64_MAX - (G - 1) + 3, UINT64_MAX};
        std::vector<uint32_t> wlen = {10, 10, 10, UINT32_MAX, 1};
        CHECK(scan_batch(wrap.data(), wlen.data(), 5, G + 1000).bad == 1);
        CHECK(first_frame_out_of_range(wrap.data(), wlen.data(), 5, G + 1000) == 1);
        CHECK(scan_batch(wrap.data() + 2, wlen.data() + 2, 3, G + 1000).bad == 1);
        CHECK(scan_batch(wrap.data() + 4, wlen.data() + 4, 1, UINT64_MAX).bad == 0);  // (the per-frame fall-back)
        CHECK(scan_batch(wrap.data() + 4, wlen.data() + 4, 1, UINT64_MAX - 1).bad == 0);
        CHECK(scan_batch(wrap.data() + 1, wlen.data() + 1, 1, UINT64_MAX).bad == 0);
    }
    {   // copy_span: exact values on both sides of 2^32
        uint64_t lo = 0, hi = 0;
        copy_span(G + 17, G + 101, G + 4096, lo, hi);
        CHECK(lo == G && hi == G + 104);
        copy_span(G + 15, G + 101, G + 102, lo, hi);  // the prefix reaches back below 2^32; the end is capped
        CHECK(lo == G - 16 && hi == G + 102);
        copy_span(G - 3, G + 1, G + 4096, lo, hi);  // a frame across 2^32
        CHECK(lo == G - 32 && hi == G + 4);
        copy_span(G - 100, G - 1, 2 * G, lo, hi);  // the end rounds up onto 2^32
        CHECK(lo == G - 128 && hi == G);
        copy_span(5 * G + 16, 5 * G + 16, 6 * G, lo, hi);  // an empty span far up
        CHECK(lo == 5 * G && hi == 5 * G + 16);
        copy_span(3, 2 * G + 1, 2 * G + 2, lo, hi);  // a span longer than 4 GiB
        CHECK(lo == 0 && hi == 2 * G + 2);
    }
    {   // host_chunks: two clusters 4 GiB apart, 70 frames each, chunks of 64 KiB: no chunk spans both
        Batch b;
        for (uint32_t i = 0; i < 140; ++i) {
            b.off.push_back((i < 70 ? G + 4096 : 64) + 128 * (i % 70));
            b.len.push_back(100);
        }
        b.bytes = G + 4096 + 128 * 70;
        check_chunks(b, 65536, 1u << 20);
        std::vector<Chunk> ch;
        host_chunks(b.off.data(), b.len.data(), 140, b.bytes, 65536, 1u << 20, ch);
        CHECK(ch.size() == 2 && ch[0].c1 == 70 && ch[0].cpy_lo == G + 4096 - 16 && ch[0].cpy_hi == G + 4096 + 128 * 69 + 100);
        CHECK(ch.size() == 2 && ch[1].cpy_lo == 48 && ch[1].cpy_hi == 64 + 128 * 69 + 100);
        // multi_blocks puts them in buffer order: the low cluster first, and cuts between the clusters
        MultiPlan p;
        multi_blocks(b.off.data(), b.len.data(), 140, 2, p);
        CHECK(p.order.size() == 140 && p.frame(0) == 70 && p.frame(69) == 139 && p.frame(70) == 0 && p.cut[1] == 70);
    }
}

// What the single-slot host calls take from the plan (fs_fill_batch_host with the 4 FCS bytes as
// `extra`, the RX coalesce host calls with total_length): the span and the range check with `extra`
// at the buffer's very end, beyond 4 GiB and near 2^64, and the sum of the lengths.
static void check_extra_span_and_total(std::mt19937_64& rng) {
    const uint64_t G = uint64_t(1) << 32;
    for (uint64_t base : {uint64_t(0), G + 4096, 5 * G + 3, UINT64_MAX - (uint64_t(1) << 34)}) {
        // the last frame in memory is frame 1; frame 2 lies lowest
        std::vector<uint64_t> off = {base + 1000, base + 5000, base + 7};
        std::vector<uint32_t> len = {60, 1500, 0};
        const uint64_t end = base + 6500;
        for (uint32_t extra : {0u, 4u}) {
            const Scan sc = scan_batch(off.data(), len.data(), 3, end + extra, extra);  // ends exactly at frames_bytes
            CHECK(sc.bad == 3 && sc.lo == base + 7 && sc.hi == end && sc.max_len == 1500 && sc.min_len == 0);
            CHECK(sc.hi + extra == end + extra);  // the fill's copied-back span ends behind the last FCS
            CHECK(first_frame_out_of_range(off.data(), len.data(), 3, end + extra, extra) == 3);
            const Scan past = scan_batch(off.data(), len.data(), 3, end + extra - 1, extra);  // one past frames_bytes
            CHECK(past.bad == 1 && past.lo == base + 7 && past.hi == end);
            CHECK(first_frame_out_of_range(off.data(), len.data(), 3, end + extra - 1, extra) == 1);
        }
        // the frame itself fits, its 4 extra bytes alone overrun: by 4, 3, 2, 1 bytes, then not at all
        for (uint32_t room = 0; room <= 4; ++room)
            CHECK(scan_batch(off.data(), len.data(), 3, end + room, 4).bad == (room < 4 ? 1u : 3u));
        // the staged copy of that span: from 16 B below the lowest frame (16-B aligned) to the buffer's end
        uint64_t lo = 0, hi = 0;
        copy_span(base + 7, end + 4, end + 4, lo, hi);
        CHECK(lo == ((base + 7 >= 16 ? base + 7 - 16 : 0) & ~uint64_t(15)) && hi == end + 4 && lo <= base + 7);
    }
    {   // frames_bytes near 2^64: the per-frame fall-back of scan_from, with and without `extra`
        std::vector<uint64_t> off = {UINT64_MAX - 100, UINT64_MAX - 5000};
        std::vector<uint32_t> len = {96, 1500};
        CHECK(scan_batch(off.data(), len.data(), 2, UINT64_MAX, 4).bad == 2);       // ends at 2^64 - 1 exactly
        CHECK(scan_batch(off.data(), len.data(), 2, UINT64_MAX - 1, 4).bad == 0);   // one past
        CHECK(scan_batch(off.data(), len.data(), 2, UINT64_MAX - 1, 0).bad == 2);
        CHECK(scan_batch(off.data(), len.data(), 2, UINT64_MAX - 5, 0).bad == 0);
        const Scan sc = scan_batch(off.data(), len.data(), 2, UINT64_MAX, 4);
        CHECK(sc.lo == UINT64_MAX - 5000 && sc.hi == UINT64_MAX - 4);
        len[0] = 97;  // offset + length + extra = 2^64 + 1: wraps, and must not pass
        CHECK(scan_batch(off.data(), len.data(), 2, UINT64_MAX, 4).bad == 0);
        CHECK(first_frame_out_of_range(off.data(), len.data(), 2, UINT64_MAX, 4) == 0);
    }
    // total_length: empty, one frame, a sum past 2^32, random batches against a plain loop
    CHECK(total_length(nullptr, 0) == 0);
    {
        const std::vector<uint32_t> big(5, UINT32_MAX);
        CHECK(total_length(big.data(), 1) == UINT32_MAX && total_length(big.data(), 5) == 5 * uint64_t(UINT32_MAX));
    }
    for (int kind = 0; kind < 5; ++kind)
        for (uint32_t n : {1u, 64u, 1000u}) {
            const Batch b = make_batch(rng, n, kind);
            uint64_t sum = 0;
            for (uint32_t l : b.len) sum += l;
            CHECK(total_length(b.len.data(), n) == sum);
        }
}

// The batch tests/test_gpu_host_calls.py fails a digest on at its second chunk: 128 frames of
// 64..1500 B in two groups of 64, the second more than 16 MiB behind the first, in 17 MiB. With the
// library's chunk parameters it is two chunks, [0, 64) and [64, 128): the second group does not fit
// the first chunk's 16 MiB, and a chunk of 64 frames does not take the rest.
static void check_two_chunk_batch() {
    Batch b;
    uint64_t pos = 0;
    for (uint32_t i = 0; i < 128; ++i) {
        if (i == 64) pos = (uint64_t(16) << 20) + 65536;
        b.len.push_back(64 + (i * 379) % 1437);
        b.off.push_back(pos);
        pos += (b.len[i] + 3) & ~3u;
    }
    b.bytes = uint64_t(17) << 20;
    CHECK(pos <= b.bytes);
    const Scan sc = scan_batch(b.off.data(), b.len.data(), 128, b.bytes);
    CHECK(sc.bad == 128 && sc.min_len >= 64 && sc.max_len <= 1500 && sc.hi - sc.lo > (uint64_t(16) << 20));
    check_chunks(b, uint64_t(16) << 20, 1u << 20);
    std::vector<Chunk> ch;
    host_chunks(b.off.data(), b.len.data(), 128, b.bytes, uint64_t(16) << 20, 1u << 20, ch);
    CHECK(ch.size() == 2 && ch[0].c0 == 0 && ch[0].c1 == 64 && ch[1].c0 == 64 && ch[1].c1 == 128);
    CHECK(ch.size() == 2 && ch[0].cpy_lo == 0 && ch[1].cpy_lo == (uint64_t(16) << 20) + 65536 - 16);
}

static void check_shards(uint64_t n, uint32_t N) {
    uint64_t sum = 0;
    for (uint32_t k = 0; k < N; ++k) sum += shard_count(n, N, k);
    CHECK(sum == n);
    const uint64_t m = shard_rows(n, N), sb = slab_bytes(m);
    CHECK(sb % 256 == 0 && sb >= 9 * m);
    // simulate: shard k writes local frame j's digest = global index (j*N + k); the gather puts
    // slab k at k*sb; the de-interleave map must give back global order
    std::vector<uint64_t> gathered((N * sb) / 8 + 1, ~0ull);
    std::vector<uint8_t> gst(N * sb, 0xEE);
    for (uint32_t k = 0; k < N; ++k)
        for (uint64_t j = 0; j < shard_count(n, N, k); ++j) {
            const uint64_t at = k * sb + 8 * j;
            CHECK(at % 8 == 0 && at + 8 <= N * sb);
            gathered[at / 8] = j * N + k;
            const uint64_t sat = k * sb + 8 * m + j;
            CHECK(sat < N * sb && sat >= k * sb + 8 * m);
            gst[sat] = (uint8_t)((j * N + k) & 0x7F);
        }
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t at = gathered_digest_at(i, N, m), sat = gathered_status_at(i, N, m);
        CHECK(at % 8 == 0 && at + 8 <= N * sb && sat < N * sb);
        CHECK(gathered[at / 8] == i);
        CHECK(gst[sat] == (uint8_t)(i & 0x7F));
    }
    // chunked gather: chunk c's pieces of every slab hold exactly global frames [c R N, (c+1) R N)
    for (uint32_t nc : {1u, 2u, 3u, 4u, 8u}) {
        const uint64_t R = chunk_rows(m, nc);
        const uint32_t C = chunk_count(m, R);
        CHECK(m == 0 || (R % 256 == 0 && C >= 1 && C <= nc && (uint64_t)C * R >= m && (uint64_t)(C - 1) * R < m));
        std::vector<uint8_t> hit(n, 0);
        for (uint32_t c = 0; c < C; ++c) {
            const uint64_t lo = c * R, hi = std::min<uint64_t>(m, lo + R);
            uint64_t rows = 0;
            for (uint32_t k = 0; k < N; ++k) {
                const uint64_t r = shard_rows_in(n, N, k, lo, hi);
                CHECK(r <= hi - lo);
                rows += r;
                for (uint64_t j = lo; j < lo + r; ++j) {
                    const uint64_t g = j * N + k;
                    CHECK(g < n && g >= lo * N && g < std::min<uint64_t>(n, hi * N));
                    ++hit[g];
                }
                CHECK((8 * lo) % 2048 == 0 && lo % 256 == 0);
            }
            CHECK(rows == (std::min<uint64_t>(n, hi * N) > lo * N ? std::min<uint64_t>(n, hi * N) - lo * N : 0));
        }
        for (uint64_t i = 0; i < n; ++i) CHECK(hit[i] == 1);
    }
}

// The exact chunk loop of fs_digest_batch_sharded (framesum_group.cpp), replayed on the host with
// memcpy standing in for ncclSend/ncclRecv: every shard's kernel writes its chunk rows into its
// slab (shard 0 in place in the gather buffer), every Piece is copied, and each chunk's
// de-interleave then reads only bytes that a kernel or a transfer of that chunk or an earlier one
// has written, getting back global frame order. Ragged n, n < N and empty shards included.
static void replay_chunks(uint64_t n, uint32_t N, uint32_t maxc, uint64_t target) {
    std::vector<ChunkXfer> plan;
    chunk_plan(n, N, maxc, target, plan);
    if (n == 0) {
        CHECK(plan.empty());
        return;
    }
    const uint64_t m = shard_rows(n, N), sb = slab_bytes(m);
    std::vector<std::vector<uint8_t>> send(N, std::vector<uint8_t>(sb, 0xCD));
    std::vector<uint8_t> recv(N * sb, 0xAB), have(N * sb, 0);
    std::vector<uint32_t> wrote(n, 0);
    uint64_t g_next = 0;
    for (const ChunkXfer& x : plan) {
        CHECK(x.lo < x.hi && x.hi <= m && x.g0 == g_next && x.g0 == x.lo * N && x.g1 <= n && x.g0 < x.g1);
        g_next = x.g1;
        // the kernels: shard k writes local rows [lo, lo + rk)
        for (uint32_t k = 0; k < N; ++k) {
            const uint64_t rk = shard_rows_in(n, N, k, x.lo, x.hi);
            uint8_t* slab = k == 0 ? recv.data() : send[k].data();
            for (uint64_t j = x.lo; j < x.lo + rk; ++j) {
                const uint64_t g = j * N + k;
                CHECK(g < n);
                std::memcpy(slab + 8 * j, &g, 8);
                slab[8 * m + j] = (uint8_t)(g * 7 + 1);
                if (k == 0) {
                    std::fill(have.begin() + 8 * j, have.begin() + 8 * j + 8, 1);
                    have[8 * m + j] = 1;
                }
            }
        }
        // the transfers
        uint32_t prev = 0;
        for (const Piece& p : x.pieces) {
            const uint32_t k = p.shard;
            CHECK(k >= 1 && k < N && k > prev);  // one piece per shard, in shard order
            prev = k;
            CHECK(p.rows == shard_rows_in(n, N, k, x.lo, x.hi) && p.rows > 0);
            CHECK(p.send_dig == 8 * x.lo && p.send_st == 8 * m + x.lo);
            CHECK(p.send_dig + 8 * p.rows <= 8 * m && p.send_st + p.rows <= sb);
            CHECK(p.recv_dig == k * sb + p.send_dig && p.recv_st == k * sb + p.send_st);
            CHECK(p.recv_dig + 8 * p.rows <= k * sb + 8 * m && p.recv_st + p.rows <= (k + 1) * sb);
            std::memcpy(recv.data() + p.recv_dig, send[k].data() + p.send_dig, 8 * p.rows);
            std::memcpy(recv.data() + p.recv_st, send[k].data() + p.send_st, p.rows);
            std::fill(have.begin() + p.recv_dig, have.begin() + p.recv_dig + 8 * p.rows, 1);
            std::fill(have.begin() + p.recv_st, have.begin() + p.recv_st + p.rows, 1);
        }
        for (uint32_t k = 1; k < N; ++k) {  // shards with rows in the chunk have a piece
            bool listed = false;
            for (const Piece& p : x.pieces) listed |= p.shard == k;
            CHECK(listed == (shard_rows_in(n, N, k, x.lo, x.hi) > 0));
        }
        // the de-interleave of [g0, g1): only received bytes, global order back
        for (uint64_t g = x.g0; g < x.g1; ++g) {
            const uint64_t at = gathered_digest_at(g, N, m), sat = gathered_status_at(g, N, m);
            bool ok = at + 8 <= recv.size() && sat < recv.size();
            CHECK(ok);
            if (!ok) continue;
            for (int b = 0; b < 8; ++b) CHECK(have[at + b]);
            CHECK(have[sat]);
            uint64_t v = 0;
            std::memcpy(&v, recv.data() + at, 8);
            CHECK(v == g);
            CHECK(recv[sat] == (uint8_t)(g * 7 + 1));
            ++wrote[g];
        }
    }
    CHECK(g_next == n);
    for (uint64_t g = 0; g < n; ++g) CHECK(wrote[g] == 1);
}

// The device result arrays of the four RX host forms (plan::rx): for every call kind, batch size and
// socket count, the arrays the kind has (stated here again, not read from the header's table), their
// alignment, that they are disjoint and inside the total, that nothing wraps (the sums again in 128
// bits), the predicate on the totals, and that no accepted totals bring back more than an array holds.
static void check_rx_arrays(uint32_t kind_index, uint64_t n, uint64_t n_socks) {
    namespace rx = framesum::plan::rx;
    typedef unsigned __int128 u128;
    const rx::Kind kind = (rx::Kind)kind_index;
    struct Want {
        rx::Array a;
        uint32_t from;  // the first kind that has it: 0 plain, 1 flows, 2 delivery, 3 receive
        uint64_t elem, align;
        bool per_sock;
    };
    const Want want[] = {{rx::kTotals, 0, kind_index == 0 ? 16u : 24u, 8, false},
                         {rx::kRuns, 0, 24, 8, false},     {rx::kFlowRecs, 1, 32, 8, false}, {rx::kOrder, 1, 4, 4, false},
                         {rx::kRunOf, 0, 4, 4, false},     {rx::kDelivered, 2, 1, 1, false}, {rx::kSocksOut, 2, 32, 8, true},
                         {rx::kSndOut, 3, 32, 8, true},    {rx::kCode, 3, 1, 1, false}};
    CHECK(sizeof want / sizeof want[0] == rx::kArrays);  // every array is one of these, and no other
    const rx::Layout L = rx::layout(kind, n, n_socks);
    u128 sum = 0, pad = 0;
    uint32_t seen = 0;
    for (const Want& w : want) {
        const bool present = kind_index >= w.from;
        seen |= 1u << w.a;
        CHECK(L.has(w.a) == present);
        if (!present) {
            CHECK(L.room[w.a] == 0);
            CHECK(rx::bytes_back(kind, w.a, n, n_socks, rx::Totals{n, n, n}) == 0);
            continue;
        }
        const u128 room = (u128)w.elem * (w.a == rx::kTotals ? 1 : w.per_sock ? n_socks : n);
        CHECK((u128)L.room[w.a] == room);
        CHECK(L.at[w.a] % w.align == 0);
        CHECK((u128)L.at[w.a] + room <= (u128)L.bytes);
        sum += room;
        pad += w.align - 1;
        for (const Want& v : want)  // pairwise disjoint
            if (v.a < w.a && kind_index >= v.from)
                CHECK((u128)L.at[v.a] + L.room[v.a] <= (u128)L.at[w.a] || (u128)L.at[w.a] + room <= (u128)L.at[v.a]);
    }
    CHECK(seen == (1u << rx::kArrays) - 1u);
    CHECK((u128)L.bytes >= sum && (u128)L.bytes <= sum + pad);
    // the totals a device may report: around 0, the middle and n in every field
    const uint64_t around[] = {0, 1, n / 2, n ? n - 1 : 0, n, n + 1};
    for (uint64_t runs : around)
        for (uint64_t flows : around)
            for (uint64_t acc : around) {
                const rx::Totals t{runs, flows, acc};
                const bool ok = kind_index == 0 ? runs <= n : acc <= n && runs <= acc && flows <= runs;
                CHECK(rx::consistent(kind, n, t) == ok);
                if (!ok) continue;
                for (const Want& w : want) {
                    if (kind_index < w.from) continue;
                    const uint64_t count = w.a == rx::kTotals ? 1 : w.a == rx::kRuns ? runs : w.a == rx::kFlowRecs ? flows
                                           : w.a == rx::kOrder ? acc : w.per_sock ? n_socks : n;
                    const uint64_t back = rx::bytes_back(kind, w.a, n, n_socks, t);
                    CHECK((u128)back == (u128)w.elem * count);
                    CHECK(back <= L.room[w.a]);
                }
            }
    // each way of being inconsistent, by name
    CHECK(!rx::consistent(rx::kPlain, n, rx::Totals{n + 1, 0, 0}));
    if (kind_index != 0) {
        CHECK(!rx::consistent(kind, n, rx::Totals{n + 1, 0, n}));          // n_runs > n
        CHECK(!rx::consistent(kind, n, rx::Totals{0, 0, n + 1}));          // n_accepted > n
        CHECK(!rx::consistent(kind, n, rx::Totals{n / 2 + 1, 0, n / 2}));  // n_runs > n_accepted
        CHECK(!rx::consistent(kind, n, rx::Totals{n / 2, n / 2 + 1, n}));  // n_flows > n_runs
        CHECK(rx::consistent(kind, n, rx::Totals{n / 2, n / 2, n}));
    }
}

// The own arrays of the accept, the close and the connect call (plan::rx::extra_layout): the thirteen rows
// stated here again in the buffer's order -- the accept call's six, the close call's three, the connect
// call's four -- each laid out behind the one before it at its alignment, from the end of the kind's
// arrays above; a kind has the rows of the kinds up to it and no other; and the offsets of one case as numbers.
static void check_extra_arrays(uint32_t kind_index, uint64_t n, uint64_t n_socks, uint64_t n_listeners, uint64_t n_slots,
                               uint64_t n_closers, uint64_t n_openers) {
    namespace rx = framesum::plan::rx;
    struct Want {
        uint32_t from;  // 4 accept, 5 close, 6 connect
        uint64_t elem, align, count;
        bool goes_in;
    };
    const Want want[] = {{4, 48, 4, n_slots, false},  {4, 16, 4, n_listeners, false}, {4, 4, 4, n, false},
                         {4, 64, 1, n_slots, true},   {4, 8, 8, n_slots, true},       {4, 1, 1, n_slots, true},
                         {5, 32, 4, n_closers, false}, {5, 32, 4, n_socks, false},     {5, 1, 1, n, false},
                         {6, 48, 4, n_openers, false}, {6, 64, 1, n_openers, true},    {6, 8, 8, n_openers, true},
                         {6, 1, 1, n_openers, true}};
    CHECK(sizeof want / sizeof want[0] == rx::kExtraArrays);
    const rx::ExtraCounts counts{{n_slots, n_listeners, n_closers, n_socks, n_openers, n}};
    const uint64_t base = rx::layout((rx::Kind)kind_index, n, n_socks).bytes;
    const rx::ExtraLayout L = rx::extra_layout(rx::kAccept, (rx::Kind)kind_index, base, counts);
    const rx::ExtraLayout alone = rx::extra_layout(rx::kConnect, rx::kConnect, 0, counts);  // the call without a batch
    uint64_t at = base, at_alone = 0;
    for (uint32_t a = 0; a < rx::kExtraArrays; ++a) {
        const Want& w = want[a];
        CHECK(rx::kExtraArrayDesc[a].goes_in == w.goes_in);
        if (w.from == 6) {
            at_alone = (at_alone + w.align - 1) / w.align * w.align;
            CHECK(alone.at[a] == at_alone && alone.room[a] == w.elem * w.count);
            at_alone += w.elem * w.count;
        } else {
            CHECK(!alone.has((rx::ExtraArray)a) && alone.room[a] == 0);
        }
        if (kind_index < w.from) {
            CHECK(!L.has((rx::ExtraArray)a) && L.room[a] == 0);
            continue;
        }
        at = (at + w.align - 1) / w.align * w.align;
        CHECK(L.at[a] == at && L.room[a] == w.elem * w.count);
        at += w.elem * w.count;
    }
    CHECK(L.bytes == at && alone.bytes == at_alone);
}
static void check_extra_arrays_by_number() {
    namespace rx = framesum::plan::rx;
    // 141 frames, 7 sockets, 3 listeners, 5 slots, 2 closers, 9 openers
    const rx::ExtraCounts counts{{5, 3, 2, 7, 9, 141}};
    CHECK(rx::layout(rx::kConnect, 141, 7).bytes == 9781);
    const rx::ExtraLayout L = rx::extra_layout(rx::kAccept, rx::kConnect, 9781, counts);
    const uint64_t at[] = {9784, 10024, 10072, 10636, 10960, 11000, 11008, 11072, 11296, 11440, 11872, 12448, 12520};
    for (uint32_t a = 0; a < rx::kExtraArrays; ++a) CHECK(L.at[a] == at[a]);
    CHECK(L.bytes == 12529);
    const rx::ExtraLayout alone = rx::extra_layout(rx::kConnect, rx::kConnect, 0, counts);
    CHECK(alone.at[rx::kOpenersOut] == 0 && alone.at[rx::kReplies] == 432 && alone.at[rx::kReplyOut] == 1008 &&
          alone.at[rx::kReplyStatus] == 1080 && alone.bytes == 1089);
}

int main() {
    std::mt19937_64 rng(12345);
    for (uint32_t kind = 0; kind < 7; ++kind)
        for (uint64_t n : {uint64_t(1), uint64_t(3), uint64_t(141), uint64_t(65793)})
            for (uint64_t lists : {uint64_t(0), uint64_t(1), uint64_t(3), uint64_t(65536)})
                check_extra_arrays(kind, n, lists, lists ? lists - 1 : 2, lists + 1, lists ? 5 : 0, lists * 3);
    check_extra_arrays_by_number();
    for (uint32_t kind = 0; kind < 4; ++kind)
        for (uint64_t n : {uint64_t(0), uint64_t(1), uint64_t(2), uint64_t(3), uint64_t(63), uint64_t(64), uint64_t(65),
                           uint64_t(255), uint64_t(256), uint64_t(257), uint64_t(65793), uint64_t(1) << 30})
            for (uint64_t n_socks : {uint64_t(0), uint64_t(1), uint64_t(3), uint64_t(64), uint64_t(65536)})
                check_rx_arrays(kind, n, n_socks);
    // chunks: every batch kind, several chunk sizes (small ones force many chunks)
    for (int kind = 0; kind < 5; ++kind)
        for (uint32_t n : {0u, 1u, 2u, 7u, 63u, 64u, 65u, 1000u, 5000u})
            for (uint64_t cb : {uint64_t(4096), uint64_t(65536), uint64_t(16) << 20}) {
                const Batch b = make_batch(rng, n, kind);
                check_chunks(b, cb, kind == 0 ? 100u : (1u << 20));
            }
    // out-of-range detection, including offsets whose end would overflow 64 bits
    {
        std::vector<uint64_t> off = {0, 100, UINT64_MAX - 2, 50};
        std::vector<uint32_t> len = {10, 20, 10, 10};
        CHECK(first_frame_out_of_range(off.data(), len.data(), 4, 1000) == 2);
        CHECK(first_frame_out_of_range(off.data(), len.data(), 2, 1000) == 2);
        CHECK(first_frame_out_of_range(off.data(), len.data(), 2, 120) == 2);
        CHECK(first_frame_out_of_range(off.data(), len.data(), 2, 119) == 1);
        CHECK(first_frame_out_of_range(off.data(), len.data(), 1, 13, 4) == 0);
        CHECK(first_frame_out_of_range(off.data(), len.data(), 1, 14, 4) == 1);
        // scan_batch reports the same first bad frame
        CHECK(scan_batch(off.data(), len.data(), 4, 1000).bad == 2);
        CHECK(scan_batch(off.data(), len.data(), 2, 1000).bad == 2);
        CHECK(scan_batch(off.data(), len.data(), 2, 119).bad == 1);
        CHECK(scan_batch(off.data(), len.data(), 1, 13, 4).bad == 0);
        CHECK(scan_batch(off.data(), len.data(), 1, 14, 4).bad == 1);
        CHECK(scan_batch(off.data(), len.data(), 0, 14).bad == 0);
    }
    check_high_offsets(rng);
    check_extra_span_and_total(rng);
    check_two_chunk_batch();
    // multi blocks: more contexts than frames, empty batches, unordered and overlapping batches
    for (int kind = 0; kind < 5; ++kind)
        for (uint32_t n : {0u, 1u, 3u, 8u, 9u, 100u, 4097u})
            for (int nctx : {1, 2, 3, 8, 16})
                check_multi(make_batch(rng, n, kind), nctx);
    // shard maps for the group entry and the bench's gather
    for (uint32_t N : {1u, 2u, 3u, 4u, 8u})
        for (uint64_t n : {uint64_t(0), uint64_t(1), uint64_t(2), uint64_t(7), uint64_t(8), uint64_t(9),
                           uint64_t(1000), uint64_t(65537), uint64_t(1) << 20})
            check_shards(n, N);
    // the sharded call's chunk loop replayed with memcpy transfers, N = 1..8,
    // ragged n, n < N, empty shards, the library's chunk parameters and small ones (many chunks)
    for (uint32_t N = 1; N <= 8; ++N)
        for (uint64_t n : {uint64_t(0), uint64_t(1), uint64_t(3), uint64_t(7), uint64_t(8), uint64_t(9), uint64_t(255),
                           uint64_t(257), uint64_t(1000), uint64_t(4097), uint64_t(65537), uint64_t(300001)}) {
            replay_chunks(n, N, 8, 32768);
            replay_chunks(n, N, 8, 256);
            replay_chunks(n, N, 3, 1);
        }
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("plan checks OK\n");
    return 0;
}
