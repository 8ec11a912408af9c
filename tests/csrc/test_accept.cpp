// The arithmetic of the accept call (seqs_amd/csrc/framesum_accept.h) on the CPU, built alone under
// ASan + UBSan by tests/test_accept_host.py: the option walk over every truncation and every malformed
// length of option fields up to 40 bytes (each field in a buffer of exactly its size, so that a read past
// it is an error), the listener lookup under hash masks 0, 0xF and full, every rejection of the lists,
// the candidate test, the rank keys with the binary search, and the records of a filled slot.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../seqs_amd/csrc/framesum_accept.h"

namespace ac = framesum::accept;

static int g_failed = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                  \
        }                                                                \
    } while (0)

// The walk again, as the header of the call words it, over a vector (at() throws past its end).
static uint32_t mss_by_the_words(const std::vector<uint8_t>& o) {
    size_t at = 0;
    for (int step = 0; step < 40; ++step) {
        if (at >= o.size()) return 0;
        const uint8_t kind = o.at(at);
        if (kind == 0) return 0;
        if (kind == 1) {
            at += 1;
            continue;
        }
        if (at + 1 >= o.size()) return 0;
        const uint8_t len = o.at(at + 1);
        if (len < 2 || at + len > o.size()) return 0;
        if (kind == 2 && len == 4) return (uint32_t)(o.at(at + 2) << 8) | o.at(at + 3);
        at += len;
    }
    return 0;
}
static uint32_t walk(const std::vector<uint8_t>& o) {
    // a heap copy of exactly o.size() bytes: ASan sees a read past the field
    uint8_t* p = static_cast<uint8_t*>(std::malloc(o.size() ? o.size() : 1));
    if (!o.empty()) std::memcpy(p, o.data(), o.size());
    const uint32_t got = ac::peer_mss(p, (uint32_t)o.size());
    std::free(p);
    return got;
}

static void test_option_walk() {
    const uint8_t mss[4] = {2, 4, 0x05, 0xB4};
    // the MSS option behind k NOPs, cut at every length 0 .. 40
    for (uint32_t nops = 0; nops <= 36; ++nops) {
        std::vector<uint8_t> full(nops, 1);
        full.insert(full.end(), mss, mss + 4);
        full.resize(40, 1);
        for (uint32_t cut = 0; cut <= 40; ++cut) {
            const std::vector<uint8_t> o(full.begin(), full.begin() + cut);
            const uint32_t want = cut >= nops + 4 ? 1460u : 0u;
            CHECK(walk(o) == want && mss_by_the_words(o) == want);
        }
    }
    // every kind with every length byte at every position of a 40-byte field, the MSS option behind it
    for (uint32_t at = 0; at < 40; ++at)
        for (uint32_t kind : {0u, 1u, 2u, 3u, 8u, 255u})
            for (uint32_t len = 0; len < 256; len += (len < 45 ? 1 : 53)) {
                std::vector<uint8_t> o(40, 1);
                o[at] = (uint8_t)kind;
                if (at + 1 < 40) o[at + 1] = (uint8_t)len;
                for (uint32_t k = 0; k < 4 && at + len + k < 40 && len >= 2; ++k) o[at + len + k] = mss[k];
                CHECK(walk(o) == mss_by_the_words(o));
                for (uint32_t cut : {at, at + 1, at + 2, at + len, at + len + 3, at + len + 4})
                    if (cut <= 40) {
                        const std::vector<uint8_t> c(o.begin(), o.begin() + cut);
                        CHECK(walk(c) == mss_by_the_words(c));
                    }
            }
    // a kind 2 of another length is skipped, the first well-formed one counts, kind 0 ends the walk
    CHECK(walk({2, 6, 9, 9, 9, 9, 2, 4, 1, 2}) == 0x0102u);
    CHECK(walk({2, 4, 0, 7, 2, 4, 0, 9}) == 7u);
    CHECK(walk({0, 2, 4, 5, 0xB4}) == 0u);
    CHECK(walk({3, 3, 7, 2, 4, 5, 0xB4}) == 1460u);
    CHECK(walk({3, 1, 2, 4, 5, 0xB4}) == 0u && walk({3, 0, 2, 4, 5, 0xB4}) == 0u);
    CHECK(walk({}) == 0u);
    // 40 steps: 40 NOPs use them all
    CHECK(walk(std::vector<uint8_t>(40, 1)) == 0u);
}

static fs_listener listener(uint32_t addr, uint32_t port, uint32_t first, uint32_t count) {
    fs_listener l;
    std::memset(&l, 0, sizeof l);
    l.local[0] = (uint8_t)(addr >> 24), l.local[1] = (uint8_t)(addr >> 16), l.local[2] = (uint8_t)(addr >> 8), l.local[3] = (uint8_t)addr;
    l.local[4] = (uint8_t)(port >> 8), l.local[5] = (uint8_t)port;
    l.mac[0] = 2, l.mac[5] = (uint8_t)port;
    l.slot_first = first, l.n_slots = count;
    return l;
}

static void test_lookup() {
    for (uint32_t n : {1u, 2u, 3u, 17u, 64u, 1000u}) {
        std::vector<fs_listener> ls;
        for (uint32_t i = 0; i < n; ++i) ls.push_back(listener(0x0A000001u + (i % 3), 1 + i / 3 * 7, i, 1));
        for (uint32_t mask : {0u, 0xFu, 0xFFFFFFFFu}) {
            std::vector<uint32_t> table(ac::table_slots(n));
            CHECK(ac::build_listener_table(ls.data(), n, mask, table.data()) == ac::kNone);
            const uint32_t tmask = (uint32_t)table.size() - 1u;
            for (uint32_t i = 0; i < n; ++i)
                CHECK(ac::lookup_listener(ac::local_of(ls[i].local), ls.data(), table.data(), tmask, mask) == i);
            // the same address with a port nobody listens on, and the same port at another address
            fs_listener other = listener(0x0A000001u, 60000, 0, 0);
            CHECK(ac::lookup_listener(ac::local_of(other.local), ls.data(), table.data(), tmask, mask) == ac::kNone);
            other = listener(0x0B000001u, 1, 0, 0);
            CHECK(ac::lookup_listener(ac::local_of(other.local), ls.data(), table.data(), tmask, mask) == ac::kNone);
            // through a key record: bytes 5..8 and 11..12
            ac::Key key{{0, 0, 0, 0}};
            uint8_t kb[16] = {6, 9, 9, 9, 9, 0, 0, 0, 0, 0x12, 0x34, 0, 0, 0, 0, 1};
            std::memcpy(kb + 5, ls[n - 1].local, 4);
            std::memcpy(kb + 11, ls[n - 1].local + 4, 2);
            std::memcpy(key.w, kb, 16);
            CHECK(ac::lookup_listener(ac::local_of_key(key), ls.data(), table.data(), tmask, mask) == n - 1);
        }
    }
}

static ac::CheckAccept check(const std::vector<fs_listener>& ls, const std::vector<fs_accept_slot>& ss, uint32_t flags = 0,
                             bool conns = true, bool lout = true, bool synacks = true) {
    std::vector<uint32_t> table;
    return ac::check_accept(ls.empty() ? nullptr : ls.data(), (uint32_t)ls.size(), ss.empty() ? nullptr : ss.data(),
                            (uint32_t)ss.size(), flags, conns, lout, synacks, 0xFFFFFFFFu, table);
}

static void test_checks() {
    const std::vector<fs_accept_slot> slots(8, fs_accept_slot{1, 2, 3, 0});
    std::vector<fs_listener> ls = {listener(1, 80, 0, 3), listener(1, 81, 5, 3), listener(2, 80, 3, 2)};
    CHECK(check(ls, slots).bad == ac::kAcceptGood);
    CHECK(check({}, {}).bad == ac::kAcceptGood && check({}, slots).bad == ac::kAcceptGood);
    CHECK(check(ls, slots, FS_FCS_APPEND).bad == ac::kAcceptGood);
    CHECK(check(ls, slots, 1).bad == ac::kSynackFlags && check(ls, slots, 4).bad == ac::kSynackFlags);
    CHECK(check(ls, slots, 0, false).bad == ac::kAcceptNull && check(ls, slots, 0, true, false).bad == ac::kAcceptNull);
    CHECK(check(ls, slots, 0, true, true, false).bad == ac::kAcceptNull);
    std::vector<uint32_t> table;
    CHECK(ac::check_accept(nullptr, 3, slots.data(), 8, 0, true, true, true, ~0u, table).bad == ac::kAcceptNull);
    CHECK(ac::check_accept(ls.data(), 3, nullptr, 8, 0, true, true, true, ~0u, table).bad == ac::kAcceptNull);
    CHECK(ac::check_accept(ls.data(), 65537, slots.data(), 8, 0, true, true, true, ~0u, table).bad == ac::kTooManyListeners);
    CHECK(ac::check_accept(ls.data(), 3, slots.data(), 65537, 0, true, true, true, ~0u, table).bad == ac::kTooManySlots);
    // no slots at all: conns and synacks may be null, and every range must be empty
    std::vector<fs_listener> none = {listener(1, 80, 0, 0)};
    CHECK(check(none, {}, 0, false, true, false).bad == ac::kAcceptGood);
    auto bad = ls;
    bad[1].reserved = 1;
    CHECK(check(bad, slots).bad == ac::kListenerReserved && check(bad, slots).index == 1);
    auto bad_slots = slots;
    bad_slots[6].reserved = 1;
    CHECK(check(ls, bad_slots).bad == ac::kSlotReserved && check(ls, bad_slots).index == 6);
    bad = ls, bad[2] = listener(1, 81, 3, 2);
    CHECK(check(bad, slots).bad == ac::kEqualLocal && check(bad, slots).index == 2);
    bad = ls, bad[0] = listener(1, 0, 0, 3);
    CHECK(check(bad, slots).bad == ac::kZeroPort && check(bad, slots).index == 0);
    bad = ls, bad[1].n_slots = 4;
    CHECK(check(bad, slots).bad == ac::kSlotRange);
    bad = ls, bad[1].slot_first = 9, bad[1].n_slots = 0;
    CHECK(check(bad, slots).bad == ac::kSlotRange);
    bad = ls, bad[1].slot_first = 0xFFFFFFFFu, bad[1].n_slots = 2;  // (the sum wraps)
    CHECK(check(bad, slots).bad == ac::kSlotRange);
    bad = ls, bad[2].n_slots = 3;  // 3..6 overlaps 5..8
    CHECK(check(bad, slots).bad == ac::kSlotsOverlap);
    bad = ls, bad[0].n_slots = 4;  // 0..4 overlaps 3..5
    CHECK(check(bad, slots).bad == ac::kSlotsOverlap);
    bad = ls, bad[2].slot_first = 4, bad[2].n_slots = 0;  // an empty range overlaps nothing
    CHECK(check(bad, slots).bad == ac::kAcceptGood);
    for (int b = ac::kAcceptNull; b <= ac::kSlotsOverlap; ++b) CHECK(ac::bad_accept_text((ac::BadAccept)b)[0] != 0);
}

static void test_candidates_and_records() {
    uint8_t l4[20] = {0x12, 0x34, 0, 80, 0xFF, 0xFF, 0xFF, 0xFF, 0, 0, 0, 0, 0x60, 0x02, 0x12, 0x34, 0, 0, 0, 0};
    ac::Syn s = ac::syn_of(l4);
    CHECK(s.seq == 0xFFFFFFFFu && s.ack == 0 && s.flags9 == ac::kSyn && s.window == 0x1234u && s.doff == 6);
    CHECK(ac::first_syn(6, s, 0) && !ac::first_syn(17, s, 0) && !ac::first_syn(6, s, 1));
    for (uint32_t bit = 0; bit < 9; ++bit) {
        ac::Syn t = s;
        t.flags9 ^= 1u << bit;
        CHECK(!ac::first_syn(6, t, 0));
    }
    l4[12] = 0x61;  // NS
    CHECK(ac::syn_of(l4).flags9 == (ac::kSyn | ac::kNs) && !ac::first_syn(6, ac::syn_of(l4), 0));
    l4[12] = 0x60, l4[11] = 1;
    CHECK(!ac::first_syn(6, ac::syn_of(l4), 0));
    // the records
    const fs_listener lis = listener(0x0A000001u, 80, 0, 1);
    for (uint32_t wnd : {0u, 65535u, 65536u, 0xFFFFFFFFu}) {
        const fs_accept_slot slot{0xFFFFFFFFu, wnd, 0xBEEF, 0};
        ac::Key key{{0, 0, 0, 0}};
        const uint8_t kb[16] = {6, 192, 168, 0, 9, 10, 0, 0, 1, 0x12, 0x34, 0, 80, 0, 0, 1};
        std::memcpy(key.w, kb, 16);
        const uint8_t mac[6] = {9, 8, 7, 6, 5, 4};
        const fs_accept_conn c = ac::conn_of(slot, key, mac, s, 1460, 77, 5);
        CHECK(std::memcmp(c.key, kb, 13) == 0 && c.used == 1 && std::memcmp(c.remote_mac, mac, 6) == 0 && c.peer_mss == 1460);
        CHECK(c.reserved == 0 && c.frame == 77 && c.flow == 5 && c.irs == 0xFFFFFFFFu && c.rcv_nxt == 0 && c.snd_nxt == 0);
        CHECK(c.snd_wnd == 0x1234u);
        uint8_t h[54];
        ac::synack_template(lis, slot, c, h);
        const uint32_t w = wnd > 65535u ? 65535u : wnd;
        const uint8_t want[54] = {9, 8, 7, 6, 5, 4, 2, 0, 0, 0, 0, 80, 8, 0, 0x45, 0, 0, 0, 0xBE, 0xEF, 0, 0, 64, 6, 0, 0,
                                  10, 0, 0, 1, 192, 168, 0, 9, 0, 80, 0x12, 0x34, 0xFF, 0xFF, 0xFF, 0xFF, 0, 0, 0, 0, 0x50, 0x12,
                                  (uint8_t)(w >> 8), (uint8_t)w, 0, 0, 0, 0};
        CHECK(std::memcmp(h, want, 54) == 0);
    }
}

static void test_rank() {
    // keys of candidates among all-ones entries, sorted as the radix sort leaves them
    for (uint32_t n : {1u, 5u, 300u, 70000u})
        for (uint32_t nl : {1u, 3u, 65536u}) {
            const uint32_t b = ac::index_bits(n), lb = ac::index_bits(nl);
            CHECK(ac::rank_bits(b, nl) == b + lb && b + lb <= 47);
            const uint64_t mask = ((uint64_t)1 << (b + lb)) - 1u;
            std::vector<uint64_t> keys;
            for (uint32_t f = 0; f < n; ++f)
                keys.push_back(f % 3 == 1 ? ac::kNoCandidate : ac::rank_key((f * 7u) % nl, f, b));
            std::sort(keys.begin(), keys.end(), [&](uint64_t x, uint64_t y) { return (x & mask) < (y & mask); });
            uint32_t run = 0;
            for (uint32_t p = 0; p < n; ++p) {
                if (keys[p] == ac::kNoCandidate) {
                    for (uint32_t q = p; q < n; ++q) CHECK(keys[q] == ac::kNoCandidate);  // they lie behind the candidates
                    break;
                }
                const uint32_t l = ac::rank_listener(keys[p], b, lb);
                CHECK(l == (uint32_t)(keys[p] >> b) && l == (ac::rank_flow(keys[p], b) * 7u) % nl);
                run = p > 0 && ac::rank_listener(keys[p - 1], b, lb) == l ? run + 1 : 0;
                CHECK(p - ac::lower_bound(keys.data(), n, (uint64_t)l << b, mask) == run);
                if (run) CHECK(ac::rank_flow(keys[p - 1], b) < ac::rank_flow(keys[p], b));  // ascending flow numbers
            }
        }
    const ac::Block blk = ac::block_of(3, 5);
    CHECK(blk.table == 72 && blk.slots == 72 + 4 * 8 && blk.bytes == blk.slots + 60);
}

int main() {
    test_option_walk();
    test_lookup();
    test_checks();
    test_candidates_and_records();
    test_rank();
    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("accept checks OK\n");
    return 0;
}
