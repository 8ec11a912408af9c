// The arithmetic of the flow-aware RX coalesce (seqs_amd/csrc/framesum_flows.h) on the CPU, built
// alone under ASan + UBSan by tests/test_flows_host.py: key extraction for every IHL and for frames
// too short to fill the 54-byte header (on exactly sized heap buffers: a read past the frame is an
// ASan report), key equality byte by byte, the hash's independence of the bytes outside the key, the
// table size, and the sort key's packing at the smallest and the largest batch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../seqs_amd/csrc/framesum_flows.h"

using namespace framesum::coalesce;
namespace fl = framesum::flows;

static int g_failed = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                  \
        }                                                                \
    } while (0)

// The key of the frame of `len` bytes at `p`, as the kernel forms it, from a heap copy of exactly
// the frame's bytes.
static fl::Key key_of_frame(const std::vector<uint8_t>& f) {
    uint8_t* p = (uint8_t*)std::malloc(f.size() ? f.size() : 1);
    std::memcpy(p, f.data(), f.size());
    const Hdr h = load_hdr_bytes(p, (uint32_t)f.size());
    const fl::Key k = fl::key_of(h, p, (uint32_t)f.size());
    std::free(p);
    return k;
}

static std::vector<uint8_t> frame(uint32_t ihl, uint8_t proto, size_t len, uint32_t seed) {
    std::vector<uint8_t> f(len);
    uint32_t x = seed * 2654435761u + 99u;
    for (auto& b : f) {
        x = x * 1664525u + 1013904223u;
        b = (uint8_t)(x >> 24);
    }
    f[12] = 0x08, f[13] = 0x00, f[14] = (uint8_t)(0x40 | ihl), f[23] = proto;
    return f;
}

static void test_key_extraction() {
    for (uint32_t ihl = 5; ihl <= 15; ++ihl)
        for (uint8_t proto : {(uint8_t)6, (uint8_t)17}) {
            const uint32_t l4 = 14 + 4 * ihl;
            const std::vector<uint8_t> f = frame(ihl, proto, l4 + 20, ihl * 3 + proto);
            const fl::Key k = key_of_frame(f);
            CHECK(fl::key_accepted(k));
            CHECK(fl::key_byte(k, 0) == proto);
            for (uint32_t i = 0; i < 8; ++i) CHECK(fl::key_byte(k, 1 + i) == f[26 + i]);
            for (uint32_t i = 0; i < 4; ++i) CHECK(fl::key_byte(k, 9 + i) == f[l4 + i]);  // the ports move with IHL
            CHECK(fl::key_byte(k, 13) == 0 && fl::key_byte(k, 14) == 0 && fl::key_byte(k, 15) == 1);
            CHECK(fl::l4_of(load_hdr_bytes(f.data(), 54)) == l4);
        }
    // UDP frames of 42 .. 54 bytes with IHL 5: the header is shorter than 54 bytes, the ports lie in it
    for (size_t len = 42; len <= 54; ++len) {
        const std::vector<uint8_t> f = frame(5, 17, len, (uint32_t)len);
        const fl::Key k = key_of_frame(f);
        for (uint32_t i = 0; i < 4; ++i) CHECK(fl::key_byte(k, 9 + i) == f[34 + i]);
        for (uint32_t i = 0; i < 8; ++i) CHECK(fl::key_byte(k, 1 + i) == f[26 + i]);
        // ... and with IHL 6 .. 9 a frame that ends right behind its ports
        for (uint32_t ihl = 6; ihl <= 9; ++ihl) {
            const std::vector<uint8_t> g = frame(ihl, 17, 14 + 4 * ihl + 4, ihl);
            const fl::Key kg = key_of_frame(g);
            for (uint32_t i = 0; i < 4; ++i) CHECK(fl::key_byte(kg, 9 + i) == g[14 + 4 * ihl + i]);
        }
    }
    // a frame cut short in front of its ports (FS_OK rules it out): zero ports, nothing read past it
    for (uint32_t ihl = 10; ihl <= 15; ++ihl) {
        const std::vector<uint8_t> g = frame(ihl, 6, 14 + 4 * ihl + 3, ihl);
        const fl::Key kg = key_of_frame(g);
        for (uint32_t i = 0; i < 4; ++i) CHECK(fl::key_byte(kg, 9 + i) == 0);
    }
    const fl::Key none = fl::no_key();
    CHECK(!fl::key_accepted(none));
}

static void test_key_equality_and_hash() {
    const std::vector<uint8_t> base = frame(5, 6, 60, 1);
    const fl::Key kb = key_of_frame(base);
    CHECK(fl::same_key(kb, kb));
    // every bit of every key byte tells two keys apart
    const size_t key_at[13] = {23, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37};
    for (size_t at : key_at)
        for (int bit = 0; bit < 8; ++bit) {
            std::vector<uint8_t> g = base;
            g[at] ^= (uint8_t)(1u << bit);
            const fl::Key kg = key_of_frame(g);
            CHECK(!fl::same_key(kb, kg) && !fl::same_key(kg, kb));
        }
    // no other byte of the frame is part of the key: MAC addresses, TotalLength, ID, Seq, flags, payload
    for (size_t at = 0; at < base.size(); ++at) {
        bool in_key = false;
        for (size_t k : key_at) in_key |= k == at;
        if (in_key || at == 14) continue;  // (byte 14 holds IHL, which moves the ports)
        std::vector<uint8_t> g = base;
        g[at] ^= 0xFF;
        const fl::Key kg = key_of_frame(g);
        CHECK(fl::same_key(kb, kg) && fl::key_hash(kb) == fl::key_hash(kg));
        CHECK(std::memcmp(&kb, &kg, sizeof kb) == 0);
    }
    // the same ports behind IP options: the same key
    {
        std::vector<uint8_t> g = frame(7, 6, 80, 5);
        std::memcpy(&g[26], &base[26], 8);
        std::memcpy(&g[14 + 28], &base[34], 4);
        const fl::Key kg = key_of_frame(g);
        CHECK(fl::same_key(kb, kg) && fl::key_hash(kb) == fl::key_hash(kg));
    }
    // the accepted bit is not part of the comparison, only the 13 bytes are
    fl::Key odd = kb;
    odd.w[3] ^= 0xFFFFFF00u;
    CHECK(fl::same_key(kb, odd) && fl::key_hash(kb) == fl::key_hash(odd));
}

static void test_table_and_sort_keys() {
    CHECK(fl::table_slots(0) == 2 && fl::table_slots(1) == 2 && fl::table_slots(2) == 4 && fl::table_slots(3) == 8);
    CHECK(fl::table_slots(65536) == 131072 && fl::table_slots(65793) == 262144);
    CHECK(fl::table_slots(1u << 30) == (1u << 31));
    for (uint32_t n : {1u, 2u, 3u, 255u, 256u, 65793u, (1u << 30) - 1u, 1u << 30}) {
        const uint32_t t = fl::table_slots(n);
        CHECK((t & (t - 1u)) == 0 && (uint64_t)t >= 2ull * n && (n < 2 || (uint64_t)t < 4ull * n));
    }
    CHECK(fl::index_bits(1) == 1 && fl::index_bits(2) == 2 && fl::index_bits(3) == 2 && fl::index_bits(4) == 3);
    CHECK(fl::index_bits(1u << 30) == 31 && fl::index_bits((1u << 30) - 1u) == 30);
    for (uint32_t n : {1u, 2u, 1u << 30}) {
        const uint32_t b = fl::index_bits(n), last = n - 1u;
        CHECK(fl::sort_bits(b) <= 63);
        const uint64_t limit = (uint64_t)1 << fl::sort_bits(b);
        // every index and every first frame of the batch packs and unpacks, below the sorted bits' limit
        for (uint32_t i : {0u, last / 2u, last})
            for (uint32_t rep : {0u, i / 2u, i}) {
                const uint64_t k = fl::sort_key(rep, i, b);
                CHECK(k < limit && fl::sort_index(k, b) == i && fl::sort_rep(k, b) == rep);
                // a frame that is not accepted lies above every accepted one and keeps its index
                const uint64_t r = fl::sort_key_rejected(i, b);
                CHECK(r < limit && r > fl::sort_key(last, last, b) && fl::sort_index(r, b) == i);
                CHECK(fl::sort_rep(r, b) > last);
            }
        // flows by first frame, then frames by index
        if (n >= 2) {
            CHECK(fl::sort_key(0, last, b) < fl::sort_key(1, 1, b));
            CHECK(fl::sort_key(0, 0, b) < fl::sort_key(0, 1, b));
        }
    }
}

int main() {
    static_assert(fl::kMaxFrames == (1u << 30) && fl::kEmpty == 0xFFFFFFFFu && sizeof(fl::Key) == 16, "flow constants");
    test_key_extraction();
    test_key_equality_and_hash();
    test_table_and_sort_keys();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("flows checks OK\n");
    return 0;
}
