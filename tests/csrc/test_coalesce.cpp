// The arithmetic of the RX coalesce (seqs_amd/csrc/framesum_coalesce.h) on the CPU, built alone under
// ASan + UBSan by tests/test_coalesce_host.py: the payload ranges, the join predicate with each excluded
// field varied and each compared bit flipped, Seq wrap, the per-frame record, and the copy plan replayed
// byte for byte on exactly sized heap buffers (an access outside the payload or its destination is an
// ASan report).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../seqs_amd/csrc/framesum_coalesce.h"

using namespace framesum::coalesce;

static int g_failed = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                  \
        }                                                                \
    } while (0)

static void put16(std::vector<uint8_t>& f, size_t at, uint32_t v) {
    f[at] = (uint8_t)(v >> 8);
    f[at + 1] = (uint8_t)v;
}
static void put32(std::vector<uint8_t>& f, size_t at, uint32_t v) {
    put16(f, at, v >> 16);
    put16(f, at + 2, v & 0xFFFFu);
}

// A 54-byte header of one flow with pseudo-random filler, TCP, IHL 5, data offset 5, flags ACK.
static std::vector<uint8_t> flow(uint32_t seed) {
    std::vector<uint8_t> f(54);
    uint32_t x = seed * 2654435761u + 12345u;
    for (auto& b : f) {
        x = x * 1664525u + 1013904223u;
        b = (uint8_t)(x >> 24);
    }
    f[12] = 0x08, f[13] = 0x00, f[14] = 0x45, f[23] = 6, f[46] = 0x50, f[47] = 0x10;
    return f;
}
static Info info_of(const std::vector<uint8_t>& f, uint32_t payload) {
    std::vector<uint8_t> g = f;
    put16(g, 16, 40 + payload);
    const Hdr h = load_hdr_bytes(g.data(), (uint32_t)g.size());
    return payload_range(h, byte_of(h, 46), byte_of(h, 47));
}
static bool joined(const std::vector<uint8_t>& p, uint32_t plen, const std::vector<uint8_t>& c, uint32_t clen) {
    const Info pi = info_of(p, plen), ci = info_of(c, clen);
    return joins(load_hdr_bytes(p.data(), 54), pi, load_hdr_bytes(c.data(), 54), ci);
}

static void test_header_load() {
    std::vector<uint8_t> f(54);
    for (size_t i = 0; i < f.size(); ++i) f[i] = (uint8_t)(i + 1);
    const Hdr h = load_hdr_bytes(f.data(), 54);
    for (uint32_t i = 0; i < 54; ++i) CHECK(byte_of(h, i) == i + 1);
    CHECK(byte_of(h, 54) == 0 && byte_of(h, 55) == 0);
    CHECK(be16_of(h, 16) == 0x1112u && be32_of(h, 38) == 0x2728292Au);
    // a short frame: only its own bytes are read (the vector is exactly that long)
    for (uint32_t avail = 0; avail <= 54; ++avail) {
        std::vector<uint8_t> g(f.begin(), f.begin() + avail);
        const Hdr s = load_hdr_bytes(g.data(), avail);
        for (uint32_t i = 0; i < 56; ++i) CHECK(byte_of(s, i) == (i < avail ? i + 1 : 0));
    }
}

static void test_payload_ranges() {
    for (uint32_t ihl = 5; ihl <= 15; ++ihl) {
        std::vector<uint8_t> f = flow(ihl);
        f[14] = (uint8_t)(0x40 | ihl);
        // UDP: frame[14 + IHL*4 + 8 : 14 + TotalLength)
        f[23] = 17;
        for (uint32_t pay : {0u, 1u, 1472u, 65507u - 4 * (ihl - 5)}) {
            put16(f, 16, 4 * ihl + 8 + pay);
            const Hdr h = load_hdr_bytes(f.data(), 54);
            const Info r = payload_range(h, 0xF0, 0xFF);  // (the TCP bytes are ignored)
            CHECK(r.accepted && !r.plain_tcp && r.tcp_flags == 0);
            CHECK(r.start == 14 + 4 * ihl + 8 && r.len == pay);
        }
        // TCP: frame[14 + IHL*4 + dataoff*4 : 14 + TotalLength)
        f[23] = 6;
        for (uint32_t doff = 5; doff <= 15; ++doff)
            for (uint32_t pay : {0u, 1u, 1446u, 60000u}) {
                put16(f, 16, 4 * ihl + 4 * doff + pay);
                const Hdr h = load_hdr_bytes(f.data(), 54);
                CHECK(tcp_bytes_at(h) == 14 + 4 * ihl + 12);
                const Info r = payload_range(h, doff << 4 | 0x0F, 0x19);
                CHECK(r.accepted && r.tcp_flags == 0x19 && r.plain_tcp == (ihl == 5 && doff == 5));
                CHECK(r.start == 14 + 4 * ihl + 4 * doff && r.len == pay);
                CHECK(r.start < 256 && r.len < 65536);
                const uint32_t x = pack_info(r);
                CHECK(rec_len(x) == r.len && rec_start(x) == r.start && rec_flags(x) == 0x19);
            }
    }
    // a TotalLength below the headers (FS_OK rules it out) gives an empty payload, not a wrapped one
    std::vector<uint8_t> f = flow(1);
    put16(f, 16, 30);
    const Hdr h = load_hdr_bytes(f.data(), 54);
    CHECK(payload_range(h, 0x50, 0x10).len == 0);
    const Info none = rejected();
    CHECK(!none.accepted && !none.plain_tcp && none.len == 0);
    CHECK(run_flags(0x10, 0x19) == 0x19 && run_flags(0x10, 0x16) == 0x10 && run_flags(0x18, 0x10) == 0x18);
}

static void test_join() {
    const std::vector<uint8_t> base = flow(7);
    std::vector<uint8_t> p = base, c = base;
    put32(p, 38, 5000);
    put32(c, 38, 5100);
    CHECK(joined(p, 100, c, 50));
    // the fields segmentation varies may differ: TotalLength, ID, IPv4 checksum, TCP checksum ...
    for (size_t at : {16u, 17u, 18u, 19u, 24u, 25u, 50u, 51u})
        for (int bit = 0; bit < 8; ++bit) {
            std::vector<uint8_t> d = c;
            d[at] ^= (uint8_t)(1u << bit);
            const Info pi = info_of(p, 100), ci = info_of(c, 50);  // (the lengths as before)
            CHECK(joins(load_hdr_bytes(p.data(), 54), pi, load_hdr_bytes(d.data(), 54), ci));
        }
    // ... and FIN and PSH on the later frame
    for (uint8_t fl : {0x11, 0x18, 0x19}) {
        std::vector<uint8_t> d = c;
        d[47] = fl;
        CHECK(joined(p, 100, d, 50));
    }
    // ... but not on the earlier one
    for (uint8_t fl : {0x11, 0x18, 0x19}) {
        std::vector<uint8_t> q = p;
        q[47] = fl;
        CHECK(!joined(q, 100, c, 50));
        std::vector<uint8_t> d = c;  // (even when the later frame carries the same flags)
        d[47] = fl;
        CHECK(!joined(q, 100, d, 50));
    }
    // Seq must continue exactly, mod 2^32
    for (uint32_t seq : {5099u, 5101u, 5000u, 0u}) {
        std::vector<uint8_t> d = c;
        put32(d, 38, seq);
        CHECK(!joined(p, 100, d, 50));
    }
    for (uint32_t s0 : {0xFFFFFFF0u, 0xFFFFFF9Cu, 0xFFFFFFFFu}) {
        std::vector<uint8_t> q = p, d = c;
        put32(q, 38, s0);
        put32(d, 38, s0 + 100u);  // wraps through 2^32
        CHECK(joined(q, 100, d, 50));
        put32(d, 38, s0 + 101u);
        CHECK(!joined(q, 100, d, 50));
    }
    // every compared bit of the header splits the run, in either frame
    uint32_t compared_bytes = 0;
    for (size_t at = 0; at < 54; ++at) {
        const bool varied = (at >= 16 && at <= 19) || at == 24 || at == 25 || (at >= 38 && at <= 41) || at == 50 || at == 51;
        if (varied) continue;
        ++compared_bytes;
        for (int bit = 0; bit < 8; ++bit) {
            if (at == 47 && ((1u << bit) & (kFin | kPsh))) continue;
            const Info pi = info_of(p, 100), ci = info_of(c, 50);  // (as classified before the flip)
            std::vector<uint8_t> d = c, q = p;
            d[at] ^= (uint8_t)(1u << bit);
            q[at] ^= (uint8_t)(1u << bit);
            CHECK(!joins(load_hdr_bytes(p.data(), 54), pi, load_hdr_bytes(d.data(), 54), ci));
            CHECK(!joins(load_hdr_bytes(q.data(), 54), pi, load_hdr_bytes(c.data(), 54), ci));
            CHECK(same_flow_header(load_hdr_bytes(q.data(), 54), load_hdr_bytes(d.data(), 54)));
        }
    }
    CHECK(compared_bytes == 42);
    // SYN, RST or URG on either frame; an empty payload; options; UDP; a frame not accepted
    for (uint8_t fl : {(uint8_t)kSyn, (uint8_t)kRst, (uint8_t)kUrg}) {
        std::vector<uint8_t> q = p, d = c;
        q[47] |= fl;
        d[47] |= fl;
        CHECK(!joined(q, 100, c, 50) && !joined(p, 100, d, 50) && !joined(q, 100, d, 50));
    }
    CHECK(!joined(p, 100, c, 0));
    {
        std::vector<uint8_t> d = c;
        put32(d, 38, 5000);
        CHECK(!joined(p, 0, d, 50));
    }
    {
        const Hdr hp = load_hdr_bytes(p.data(), 54), hc = load_hdr_bytes(c.data(), 54);
        Info pi = info_of(p, 100), ci = info_of(c, 50);
        CHECK(joins(hp, pi, hc, ci));
        Info x = pi;
        x.accepted = false;
        CHECK(!joins(hp, x, hc, ci));
        x = ci;
        x.accepted = false;
        CHECK(!joins(hp, pi, hc, x));
        x = pi;
        x.plain_tcp = false;
        CHECK(!joins(hp, x, hc, ci));
        x = ci;
        x.plain_tcp = false;
        CHECK(!joins(hp, pi, hc, x));
    }
    {
        std::vector<uint8_t> q = p, d = c;  // data offset 6 on both: equal headers, still no join
        q[46] = d[46] = 0x60;
        const Hdr hq = load_hdr_bytes(q.data(), 54), hd = load_hdr_bytes(d.data(), 54);
        const Info qi = payload_range(hq, 0x60, 0x10), di = payload_range(hd, 0x60, 0x10);
        CHECK(same_flow_header(hq, hd) && !qi.plain_tcp && !joins(hq, qi, hd, di));
    }
}

// The kernel's copy, lane by lane: which bytes each access moves.
static void replay_copy(uint8_t* dst, const uint8_t* src, uint32_t len, uint64_t dst_addr, std::vector<int>& hits) {
    const CopyPlan c = copy_plan(dst_addr, len);
    auto move = [&](size_t at, size_t n) {
        std::memcpy(dst + at, src + at, n);
        for (size_t i = 0; i < n; ++i) ++hits[at + i];
    };
    CHECK(c.head < 16 && c.tail < 16 && c.head + 16ull * c.body + c.tail == len);
    if (c.body || c.tail) CHECK((dst_addr + c.head) % 16 == 0);  // the body is stored aligned
    for (uint32_t p = 0; p < c.body; ++p) move(c.head + 16ull * p, 16);
    if (c.head & 1u) move(0, 1);
    if (c.head & 2u) move(c.head & 1u, 2);
    if (c.head & 4u) move(c.head & 3u, 4);
    if (c.head & 8u) move(c.head & 7u, 8);
    const size_t t0 = c.head + 16ull * c.body;
    if (c.tail & 8u) move(t0, 8);
    if (c.tail & 4u) move(t0 + (c.tail & 8u), 4);
    if (c.tail & 2u) move(t0 + (c.tail & 12u), 2);
    if (c.tail & 1u) move(t0 + (c.tail & 14u), 1);
}

static void test_copy_plan() {
    for (uint32_t len : {0u, 1u, 2u, 3u, 7u, 8u, 15u, 16u, 17u, 31u, 32u, 33u, 63u, 64u, 65u, 100u, 1446u})
        for (uint64_t addr = 0; addr < 16; ++addr) {
            // exactly `len` bytes on the heap each: any access outside them is an ASan report
            uint8_t* src = (uint8_t*)std::malloc(len ? len : 1);
            uint8_t* dst = (uint8_t*)std::malloc(len ? len : 1);
            for (uint32_t i = 0; i < len; ++i) src[i] = (uint8_t)(i * 7 + addr), dst[i] = 0xEE;
            std::vector<int> hits(len, 0);
            replay_copy(dst, src, len, 0x1000 + addr, hits);
            for (uint32_t i = 0; i < len; ++i) CHECK(hits[i] == 1 && dst[i] == src[i]);
            std::free(src);
            std::free(dst);
        }
}

int main() {
    static_assert(kScanBlock >= 64 && kScanBlock % 64 == 0 && kScanBlock <= 1024, "one frame per lane of whole waves");
    test_header_load();
    test_payload_ranges();
    test_join();
    test_copy_plan();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("coalesce checks OK\n");
    return 0;
}
