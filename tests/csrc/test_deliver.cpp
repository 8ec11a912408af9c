// The arithmetic of the in-order TCP delivery (seqs_amd/csrc/framesum_deliver.h) on the CPU, built
// alone under ASan + UBSan by tests/test_deliver_host.py: every rejection of the socket list, the
// socket table's build and lookup under the hash masks 0 and ~0 (on exactly sized heap arrays: a probe
// past the table is an ASan report), the admission rule at each of its boundaries, and the split of a
// ring write at the wrap against a byte-by-byte model of the ring.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../seqs_amd/csrc/framesum_connect.h"
#include "../../seqs_amd/csrc/framesum_deliver.h"

namespace dl = framesum::deliver;
namespace fl = framesum::flows;
using framesum::coalesce::kFin;
using framesum::coalesce::kRst;
using framesum::coalesce::kSyn;

static int g_failed = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                  \
        }                                                                \
    } while (0)

static fs_rx_sock sock(uint32_t id, uint64_t ring_off, uint32_t ring_size) {
    fs_rx_sock s;
    std::memset(&s, 0, sizeof s);
    s.key[0] = 6;
    for (int k = 0; k < 4; ++k) s.key[1 + k] = (uint8_t)(id >> (8 * k));
    s.key[9] = 0x12, s.key[11] = 0x50;
    s.rcv_wnd = 65535;
    s.ring_size = ring_size;
    s.ring_off = ring_off;
    s.ring_free = ring_size;
    return s;
}

static dl::Bad verdict(const std::vector<fs_rx_sock>& socks, uint64_t rings_bytes, uint32_t* which = nullptr,
                       bool have_rings = true, bool have_out = true, uint32_t n_socks = 0xFFFFFFFFu) {
    std::vector<uint32_t> table;
    const dl::Check c = dl::check_socks(socks.empty() ? nullptr : socks.data(),
                                        n_socks == 0xFFFFFFFFu ? (uint32_t)socks.size() : n_socks, have_rings, have_out,
                                        rings_bytes, 0xFFFFFFFFu, table);
    if (which) *which = c.sock;
    return c.bad;
}

static void test_checks() {
    const std::vector<fs_rx_sock> good = {sock(1, 0, 100), sock(2, 100, 28), sock(3, 200, 1)};
    uint32_t which = 99;
    CHECK(verdict(good, 201) == dl::kGood);
    CHECK(verdict({}, 0) == dl::kGood);  // no sockets: nothing to check, null pointers and all
    {
        std::vector<uint32_t> table;
        const dl::Check c = dl::check_socks(good.data(), 3, true, true, 201, 0xFFFFFFFFu, table);
        CHECK(c.bad == dl::kGood && c.lo == 0 && c.hi == 201 && table.size() == 8);
        CHECK(dl::check_socks(nullptr, 0, false, false, 0, 0, table).bad == dl::kGood);
        CHECK(dl::check_socks(nullptr, 3, true, true, 201, 0, table).bad == dl::kNullPointer);
    }
    CHECK(verdict(good, 201, nullptr, false, true) == dl::kNullPointer);
    CHECK(verdict(good, 201, nullptr, true, false) == dl::kNullPointer);
    CHECK(verdict(good, 201, nullptr, true, true, dl::kMaxSocks + 1u) == dl::kTooManySocks);  // (before any record is read)
    CHECK(verdict(good, 200, &which) == dl::kRingOutside && which == 2);
    auto with = [&](uint32_t i, auto change) {
        std::vector<fs_rx_sock> v = good;
        change(v[i]);
        return v;
    };
    CHECK(verdict(with(1, [](fs_rx_sock& s) { s.key[0] = 17; }), 201, &which) == dl::kKeyNotTcp && which == 1);
    CHECK(verdict(with(2, [](fs_rx_sock& s) { s.reserved[2] = 1; }), 201, &which) == dl::kReservedNotZero && which == 2);
    CHECK(verdict(with(0, [](fs_rx_sock& s) { s.reserved[0] = 0x80; }), 201) == dl::kReservedNotZero);
    CHECK(verdict(with(2, [&](fs_rx_sock& s) { std::memcpy(s.key, good[0].key, 13); }), 201, &which) == dl::kEqualKeys &&
          which == 2);
    CHECK(verdict(with(1, [](fs_rx_sock& s) { s.ring_size = 0; }), 201) == dl::kRingSize);
    CHECK(verdict(with(1, [](fs_rx_sock& s) { s.ring_size = (1u << 31) + 1u; }), ~0ull) == dl::kRingSize);
    CHECK(verdict(with(1, [](fs_rx_sock& s) { s.ring_off = 1000, s.ring_size = s.ring_free = 1u << 31; }), 1ull << 32) ==
          dl::kGood);
    CHECK(verdict(with(1, [](fs_rx_sock& s) { s.ring_wpos = 28; }), 201) == dl::kRingState);
    CHECK(verdict(with(1, [](fs_rx_sock& s) { s.ring_wpos = 27; }), 201) == dl::kGood);
    CHECK(verdict(with(1, [](fs_rx_sock& s) { s.ring_free = 29; }), 201) == dl::kRingState);
    CHECK(verdict(with(1, [](fs_rx_sock& s) { s.ring_free = 0; }), 201) == dl::kGood);
    CHECK(verdict(with(2, [](fs_rx_sock& s) { s.ring_off = ~0ull; }), 201) == dl::kRingOutside);  // (no wrap of off + size)
    CHECK(verdict(with(1, [](fs_rx_sock& s) { s.ring_off = 99; }), 201, &which) == dl::kRingsOverlap && which == 1);
    CHECK(verdict(with(2, [](fs_rx_sock& s) { s.ring_off = 127; }), 201, &which) == dl::kRingsOverlap && which == 2);
    CHECK(verdict(with(2, [](fs_rx_sock& s) { s.ring_off = 128; }), 201) == dl::kGood);  // rings may touch
    for (int b = dl::kNullPointer; b <= dl::kRingsOverlap; ++b) CHECK(dl::bad_text((dl::Bad)b)[0] != 0);
}

static void test_table() {
    for (uint32_t mask : {0u, 0xFu, 0xFFFFFFFFu})
        for (uint32_t n : {1u, 2u, 3u, 64u, 300u}) {
            std::vector<fs_rx_sock> socks;
            for (uint32_t i = 0; i < n; ++i) socks.push_back(sock(7919u * i + 1u, 64ull * i, 64));
            const uint32_t slots = fl::table_slots(n);
            CHECK(slots >= 2 * n && (slots & (slots - 1)) == 0);
            uint32_t* table = (uint32_t*)std::malloc(4ull * slots);  // exactly sized
            fs_rx_sock* recs = (fs_rx_sock*)std::malloc(sizeof(fs_rx_sock) * n);
            std::memcpy(recs, socks.data(), sizeof(fs_rx_sock) * n);
            CHECK(fl::build_table(recs, n, mask, table) == dl::kNone);
            uint32_t used = 0;
            for (uint32_t s = 0; s < slots; ++s) used += table[s] != dl::kNone;
            CHECK(used == n);
            for (uint32_t i = 0; i < n; ++i) CHECK(fl::lookup(fl::wire_key(recs[i].key), recs, table, slots - 1, mask) == i);
            // keys that differ from a socket's in one byte, and a key the frames' records never carry
            for (uint32_t at = 0; at < 13; ++at) {
                fs_rx_sock other = recs[n / 2];
                other.key[at] ^= 0x40;
                bool is_another = false;
                for (uint32_t i = 0; i < n; ++i) is_another |= std::memcmp(other.key, recs[i].key, 13) == 0;
                if (!is_another) CHECK(fl::lookup(fl::wire_key(other.key), recs, table, slots - 1, mask) == dl::kNone);
            }
            // a frame's key record equals the socket's whatever its byte 15 and bytes 13, 14 say
            fl::Key k = fl::wire_key(recs[0].key);
            k.w[3] &= 0xFFu;
            CHECK(fl::lookup(k, recs, table, slots - 1, mask) == 0);
            // an equal key is found by the build
            if (n > 1) {
                std::memcpy(recs[n - 1].key, recs[0].key, 13);
                CHECK(fl::build_table(recs, n, mask, table) == n - 1);
            }
            std::free(table);
            std::free(recs);
        }
    CHECK(dl::block_of(3).table == 144 && dl::block_of(3).bytes == 144 + 4 * 8);
}

// The one table template (framesum_flows.h) over the three record types that begin with the 13 key bytes:
// the same keys give the same table, the same lookups and the same duplicate, whatever else a record holds
// and however long it is. Exactly sized heap arrays again.
template <class Rec>
static Rec* keyed_list(const std::vector<fs_rx_sock>& keys, uint8_t fill) {
    Rec* recs = (Rec*)std::malloc(sizeof(Rec) * keys.size());
    std::memset(recs, fill, sizeof(Rec) * keys.size());  // (the rest of a record does not matter)
    for (size_t i = 0; i < keys.size(); ++i) std::memcpy(recs[i].key, keys[i].key, 13);
    return recs;
}
static void test_one_table_for_all_records() {
    for (uint32_t mask : {0u, 1u, 0xFFu, 0xFFFFFFFFu})
        for (uint32_t n : {1u, 2u, 3u, 64u, 65u}) {
            std::vector<fs_rx_sock> keys;
            for (uint32_t i = 0; i < n; ++i) keys.push_back(sock(104729u * i + 5u, 0, 1));
            const fs_rx_sock absent = sock(104729u * n + 5u, 0, 1);
            fs_rx_sock* rx = keyed_list<fs_rx_sock>(keys, 0x00);
            fs_cl_sock* cl = keyed_list<fs_cl_sock>(keys, 0x5A);
            fs_cn_sock* cn = keyed_list<fs_cn_sock>(keys, 0xFF);
            const uint32_t slots = fl::table_slots(n);
            uint32_t* t_rx = (uint32_t*)std::malloc(4ull * slots);
            uint32_t* t_cl = (uint32_t*)std::malloc(4ull * slots);
            uint32_t* t_cn = (uint32_t*)std::malloc(4ull * slots);
            CHECK(fl::build_table(rx, n, mask, t_rx) == dl::kNone);
            CHECK(fl::build_table(cl, n, mask, t_cl) == dl::kNone);
            CHECK(fl::build_table(cn, n, mask, t_cn) == dl::kNone);
            CHECK(std::memcmp(t_rx, t_cl, 4ull * slots) == 0 && std::memcmp(t_rx, t_cn, 4ull * slots) == 0);
            for (uint32_t i = 0; i < n; ++i) {
                const fl::Key k = fl::wire_key(keys[i].key);
                CHECK(fl::lookup(k, rx, t_rx, slots - 1, mask) == i);
                CHECK(fl::lookup(k, cl, t_cl, slots - 1, mask) == i);
                CHECK(fl::lookup(k, cn, t_cn, slots - 1, mask) == i);
            }
            const fl::Key none = fl::wire_key(absent.key);
            CHECK(fl::lookup(none, rx, t_rx, slots - 1, mask) == dl::kNone);
            CHECK(fl::lookup(none, cl, t_cl, slots - 1, mask) == dl::kNone);
            CHECK(fl::lookup(none, cn, t_cn, slots - 1, mask) == dl::kNone);
            if (n > 1) {  // the last key repeats the first
                std::memcpy(rx[n - 1].key, rx[0].key, 13);
                std::memcpy(cl[n - 1].key, cl[0].key, 13);
                std::memcpy(cn[n - 1].key, cn[0].key, 13);
                CHECK(fl::build_table(rx, n, mask, t_rx) == n - 1);
                CHECK(fl::build_table(cl, n, mask, t_cl) == n - 1);
                CHECK(fl::build_table(cn, n, mask, t_cn) == n - 1);
            }
            std::free(t_rx), std::free(t_cl), std::free(t_cn);
            std::free(rx), std::free(cl), std::free(cn);
        }
}

static bool admit(dl::State st, uint32_t seq, uint32_t ack, uint32_t len, uint32_t flags, uint32_t wnd, uint32_t snd) {
    const bool whole = dl::admitted(st, seq, ack, len, flags, wnd, snd);
    // the kernel's two halves give the same answer
    const uint32_t w = dl::mark_word(len, flags, ack, wnd, snd);
    const bool halves = (w & dl::kMkConsidered) && !(w & dl::kMkStop) && (w & dl::kMkFixedOk) &&
                        dl::in_order_and_fits(st, seq, w & 0xFFFFu);
    CHECK(whole == halves);
    CHECK(((w & dl::kMkFin) != 0) == ((flags & kFin) != 0));
    return whole;
}

static void test_admission() {
    const uint32_t A = dl::kAck;
    for (uint32_t nxt : {1000u, 0u, 0xFFFFFFFFu, 0x80000000u}) {
        const dl::State st{nxt, 0, 500};
        CHECK(admit(st, nxt, 7, 100, A, 65535, 7));
        CHECK(!admit(st, nxt + 1u, 7, 100, A, 65535, 7));  // (a)
        CHECK(!admit(st, nxt - 1u, 7, 100, A, 65535, 7));
    }
    const dl::State st{1000, 0, 500};
    // (b): len + fin against the window
    CHECK(admit(st, 1000, 0, 100, 0, 100, 0) && !admit(st, 1000, 0, 100, 0, 99, 0));
    CHECK(admit(st, 1000, 0, 99, kFin, 100, 0) && !admit(st, 1000, 0, 100, kFin, 100, 0) && admit(st, 1000, 0, 100, kFin, 101, 0));
    CHECK(!admit(st, 1000, 0, 1, 0, 0, 0) && !admit(st, 1000, 0, 0, kFin, 0, 0) && admit(st, 1000, 0, 0, kFin, 1, 0));
    CHECK(admit(st, 1000, 0, 500, 0, 0xFFFFFFFFu, 0));
    // (c): Ack against snd_nxt, across 2^31 and 2^32
    for (uint32_t snd : {5000u, 0u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu}) {
        CHECK(admit(st, 1000, snd, 10, A, 65535, snd));
        CHECK(!admit(st, 1000, snd + 1u, 10, A, 65535, snd));
        CHECK(admit(st, 1000, snd - 1u, 10, A, 65535, snd));
        CHECK(!admit(st, 1000, snd + 0x7FFFFFFFu, 10, A, 65535, snd));
        CHECK(admit(st, 1000, snd + 0x80000000u, 10, A, 65535, snd));  // (int32)(Ack - snd_nxt) = -2^31
        CHECK(admit(st, 1000, snd + 1u, 10, 0, 65535, snd));           // no ACK flag: the field is not looked at
    }
    // (d): len against free
    CHECK(admit(dl::State{1000, 3, 100}, 1000, 0, 100, 0, 65535, 0) && !admit(dl::State{1000, 3, 100}, 1000, 0, 101, 0, 65535, 0));
    CHECK(admit(dl::State{1000, 3, 0}, 1000, 0, 0, kFin, 65535, 0) && !admit(dl::State{1000, 3, 0}, 1000, 0, 1, 0, 65535, 0));
    // considered, and the frames that end the walk
    CHECK(!dl::considered(0, A) && dl::considered(0, A | kFin) && dl::considered(1, A));
    CHECK(dl::stops_walk(kSyn) && dl::stops_walk(kRst | A) && !dl::stops_walk(A | kFin));
    CHECK(!admit(st, 1000, 0, 0, A, 65535, 0) && !admit(st, 1000, 0, 10, kSyn, 65535, 0) && !admit(st, 1000, 0, 10, kRst, 65535, 0));
    // the state behind a segment
    dl::State n = dl::advance(dl::State{0xFFFFFFF0u, 90, 40}, 30, true, 100);
    CHECK(n.nxt == 15 && n.wpos == 20 && n.free == 10);
    n = dl::advance(dl::State{5, 70, 30}, 30, false, 100);
    CHECK(n.nxt == 35 && n.wpos == 0 && n.free == 0);
    n = dl::advance(dl::State{5, (1u << 31) - 1u, 1u << 31}, 65535, false, 1u << 31);
    CHECK(n.wpos == 65534 && n.free == (1u << 31) - 65535u);
    n = dl::advance(dl::State{5, 0, 1}, 1, false, 1);
    CHECK(n.wpos == 0 && n.free == 0 && n.nxt == 6);
}

// ring.Write's placement, byte by byte.
static void test_wrap_split() {
    for (uint32_t size : {1u, 2u, 64u, 100u})
        for (uint32_t wpos = 0; wpos < size; ++wpos)
            for (uint32_t len = 0; len <= size; ++len) {
                const dl::Split sp = dl::split_at_wrap(wpos, len, size);
                CHECK(sp.first + sp.second == len && wpos + sp.first <= size && sp.second <= wpos);
                std::vector<int> ring(size, -1), model(size, -1);
                for (uint32_t j = 0; j < sp.first; ++j) ring[wpos + j] = (int)j;
                for (uint32_t j = 0; j < sp.second; ++j) ring[j] = (int)(sp.first + j);
                for (uint32_t j = 0; j < len; ++j) model[(wpos + j) % size] = (int)j;
                CHECK(ring == model);
                CHECK(dl::advance(dl::State{0, wpos, size}, len, false, size).wpos == (wpos + len) % size);
            }
    // the three ends the issue names: wpos + len = size - 1, size, size + 1
    CHECK(dl::split_at_wrap(4000, 95, 4096).second == 0 && dl::split_at_wrap(4000, 96, 4096).second == 0);
    CHECK(dl::split_at_wrap(4000, 97, 4096).first == 96 && dl::split_at_wrap(4000, 97, 4096).second == 1);
    const fs_rx_sock s = sock(9, 77, 50);
    const fs_rx_sock_out o = dl::untouched(s);
    CHECK(o.rcv_nxt == 0 && o.ring_free == 50 && o.flow == dl::kNone && o.stop == dl::kNone && o.bytes == 0);
}

int main() {
    test_checks();
    test_table();
    test_one_table_for_all_records();
    test_admission();
    test_wrap_split();
    if (g_failed) {
        std::printf("%d deliver checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("deliver checks OK\n");
    return 0;
}
