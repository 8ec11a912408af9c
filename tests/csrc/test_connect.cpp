// The arithmetic of the connect call (seqs_amd/csrc/framesum_connect.h) on the CPU, built alone under
// ASan + UBSan by tests/test_connect_host.py: code_of and apply over the grid of one-frame cases against
// the rule as the header of the call words it (written here again, rule 2 in its one-line form), rule
// 5's literal comparisons around iss + 1 and 2^31 away, the opener table under hash masks 0, 0xF and full
// (tables and record lists in heap blocks of exactly their size), the option walk over every truncation
// of an option block (each in a heap block of exactly its size), every rejection of the opener list, the
// staged block, the record without a flow and the reply templates.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../seqs_amd/csrc/framesum_connect.h"

namespace cn = framesum::connect;
namespace fl = framesum::flows;
namespace cl = framesum::closing;
namespace dl = framesum::deliver;
namespace ac = framesum::accept;

static int g_failed = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                  \
        }                                                                \
    } while (0)

constexpr uint32_t FIN = 1, SYN = 2, RST = 4, PSH = 8, ACK = 16;

static fs_cn_sock opener(uint32_t i, uint32_t iss = 1000, uint32_t rcv_wnd = 4096, uint8_t flags = 0) {
    fs_cn_sock s;
    std::memset(&s, 0, sizeof s);
    s.key[0] = 6;
    for (uint32_t b = 1; b < 13; ++b) s.key[b] = (uint8_t)(i * 31u + b * 7u + (i >> 8));
    s.key[9] = (uint8_t)(i >> 8), s.key[10] = (uint8_t)i;
    s.flags = flags;
    for (uint32_t b = 0; b < 6; ++b) s.local_mac[b] = (uint8_t)(0x10 + b), s.remote_mac[b] = (uint8_t)(0xA0 + b + i);
    s.iss = iss, s.rcv_wnd = rcv_wnd, s.ip_id = (uint16_t)(0x1234 + i);
    return s;
}

// The rule by the words of include/framesum_connect.h: the code (0xFE / 0xFF: the walk ends in front).
static uint32_t by_the_words(uint32_t iss, uint32_t rcv_wnd, const cn::Seg& f) {
    const bool syn = f.flags9 & SYN, ack = f.flags9 & ACK, fin = f.flags9 & FIN;
    if (f.seq == 0xFFFFFFFFu && f.flags9 == ACK && f.ack == iss + 1u && f.len == 0) return 5;
    if (!syn) {
        const bool passes = f.seq == 0 && (f.len == 0 || (rcv_wnd > 0 && (uint64_t)f.len + (fin ? 1 : 0) - 1 < rcv_wnd));
        if (!passes) return 4;
    }
    if (f.flags9 & RST) return 0xFE;
    if (syn && (f.len > 0 || (f.flags9 & ~(SYN | ACK)))) return 0xFF;
    if (ack && f.ack != iss + 1u) return 11;
    if (!syn) return 10;
    return 1;
}

static void test_rule_over_the_grid() {
    const uint32_t isses[] = {0u, 1000u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    const uint32_t wnds[] = {0u, 1u, 1000u, 0xFFFFFFFFu};
    uint32_t seen[256] = {};
    for (uint32_t iss : isses)
        for (uint32_t rcv_wnd : wnds) {
            const uint32_t seqs[] = {0u, 1u, 0xFFFFFFFFu, rcv_wnd - 1u, rcv_wnd};
            const uint32_t acks[] = {iss, iss + 1u, iss + 2u, iss + 1u + 0x80000000u, iss + 0x80000000u, iss + 2u + 0x80000000u, 0u};
            const uint32_t lens[] = {0u, 1u, rcv_wnd > 65535u ? 65535u : rcv_wnd, rcv_wnd > 65534u ? 65535u : rcv_wnd + 1u};
            for (uint32_t bits = 0; bits < 32; ++bits) {
                const uint32_t flags9 = (bits & 1 ? SYN : 0) | (bits & 2 ? ACK : 0) | (bits & 4 ? RST : 0) | (bits & 8 ? FIN : 0) |
                                        (bits & 16 ? PSH : 0);
                for (uint32_t seq : seqs)
                    for (uint32_t ack : acks)
                        for (uint32_t len : lens) {
                            const cn::Seg f{seq, ack, 777u, flags9, len};
                            const uint32_t code = cn::code_of(iss, rcv_wnd, f);
                            CHECK(code == by_the_words(iss, rcv_wnd, f));
                            ++seen[code];
                            CHECK(cn::is_event(code) == (code == 1 || code == 11 || code == 0xFE || code == 0xFF));
                            CHECK(cn::counts_rejected(code) == (code == 4 || code == 10));
                            // the record behind the frame
                            const fs_cn_sock s = opener(3, iss, rcv_wnd);
                            const fs_cn_out u = cn::untouched(s);
                            if (!cn::is_event(code)) continue;
                            const fs_cn_out o = cn::apply(u, s, code, f, 70, 9, 1460);
                            if (code == 0xFE || code == 0xFF) {
                                CHECK(o.stop == 70 && o.flags == (code == 0xFE ? FS_CN_STOP_RST : FS_CN_STOP_SYN));
                                CHECK(o.state == 3 && o.reply == 0 && o.frame == cn::kNone && o.snd_una == iss && o.snd_nxt == iss + 1u);
                            } else if (code == 11) {
                                CHECK(o.stop == 71 && o.frame == 9 && o.state == 3 && o.reply == FS_CN_REPLY_RST && o.rst_seq == ack);
                                CHECK(o.snd_una == iss && o.snd_nxt == iss && o.snd_wnd == 777 && o.irs == 0 && o.rcv_nxt == 0);
                                CHECK(o.peer_mss == 0);
                            } else if (flags9 == (SYN | ACK)) {
                                CHECK(o.stop == 71 && o.frame == 9 && o.state == 4 && o.reply == FS_CN_REPLY_ACK && o.rst_seq == 0);
                                CHECK(o.irs == seq && o.rcv_nxt == seq + 1u && o.snd_una == iss + 1u && o.snd_nxt == iss + 1u);
                                CHECK(o.snd_wnd == 777 && o.peer_mss == 1460 && ack == iss + 1u);
                            } else {
                                CHECK(flags9 == SYN && o.stop == 71 && o.state == 2 && o.reply == FS_CN_REPLY_SYNACK);
                                CHECK(o.irs == seq && o.rcv_nxt == seq + 1u && o.snd_una == iss && o.snd_nxt == iss && o.snd_wnd == 777);
                            }
                        }
            }
        }
    for (uint32_t code : {1u, 4u, 5u, 10u, 11u, 0xFEu, 0xFFu}) CHECK(seen[code] > 0);
}

// Rule 2: the four literal cases against the one-line form, over windows and lengths a frame cannot
// carry too.
static void test_rule2_derivation() {
    const uint32_t wnds[] = {0u, 1u, 2u, 1000u, 65535u, 65536u, 0x80000000u, 0xFFFFFFFFu};
    for (uint32_t rcv_wnd : wnds)
        for (uint32_t seq : {0u, 1u, 2u, 999u, 1000u, 65535u, 0x80000000u, 0xFFFFFFFFu, rcv_wnd - 1u, rcv_wnd})
            for (uint32_t len : {0u, 1u, 2u, 999u, 1000u, 1001u, 65534u, 65535u})
                for (uint32_t fin : {0u, 1u}) {
                    const cn::Seg f{seq, 0u, 0u, fin ? FIN : 0u, len};
                    const bool one_line = seq == 0 && (len == 0 || (rcv_wnd > 0 && len + fin - 1u < rcv_wnd));
                    CHECK(cn::seq_checks_pass(rcv_wnd, f) == one_line);
                }
}

// Rule 5: only iss + 1 passes, by the literal LessThan / LessThanEq forms.
static void test_rule5_derivation() {
    for (uint32_t iss : {0u, 1u, 1000u, 0x7FFFFFFEu, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu})
        for (uint32_t d : {0u, 1u, 2u, 3u, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0x80000002u, 0xFFFFFFFEu, 0xFFFFFFFFu}) {
            const uint32_t ack = iss + d;
            const bool acks_old = !cn::less_than(iss, ack), acks_unsent = !cn::less_than_eq(ack, iss + 1u);
            CHECK(cn::bad_ack(iss, ack) == (acks_old || acks_unsent));
            CHECK(cn::bad_ack(iss, ack) == (d != 1u));
            // which of the two refuses: old at 0 and from 2^31 + 1 on, unsent from 2 up to 2^31
            CHECK(acks_old == (d == 0u || d > 0x80000000u));
            CHECK(acks_unsent == (d >= 2u && d <= 0x80000000u));
        }
}

static void test_opener_table() {
    const uint32_t masks[] = {0u, 0xFu, 0xFFFFFFFFu};
    const uint32_t counts[] = {1u, 2u, 17u, 300u};
    for (uint32_t mask : masks)
        for (uint32_t n : counts) {
            // heap blocks of exactly their size: ASan sees a read or a write past them
            fs_cn_sock* list = static_cast<fs_cn_sock*>(std::malloc(n * sizeof(fs_cn_sock)));
            for (uint32_t i = 0; i < n; ++i) list[i] = opener(i);
            const uint32_t slots = cn::table_slots(n);
            uint32_t* table = static_cast<uint32_t*>(std::malloc(4ull * slots));
            CHECK(fl::build_table(list, n, mask, table) == cn::kNone);
            uint32_t filled = 0;
            for (uint32_t s = 0; s < slots; ++s) filled += table[s] != cn::kNone;
            CHECK(filled == n);
            for (uint32_t i = 0; i < n; ++i) CHECK(fl::lookup(fl::wire_key(list[i].key), list, table, slots - 1u, mask) == i);
            for (uint32_t i = n; i < n + 50u; ++i)
                CHECK(fl::lookup(fl::wire_key(opener(i).key), list, table, slots - 1u, mask) == cn::kNone);
            // one bit away from a listed key, in every key byte behind the protocol
            for (uint32_t b = 1; b < 13; ++b) {
                fs_cn_sock near = list[n / 2];
                near.key[b] ^= (uint8_t)(1u << (b % 8));
                const uint32_t hit = fl::lookup(fl::wire_key(near.key), list, table, slots - 1u, mask);
                CHECK(hit == cn::kNone || std::memcmp(list[hit].key, near.key, 13) == 0);
            }
            // the staged block holds the records, then the table
            const cn::Block b = cn::block_of(n);
            CHECK(b.table == (uint64_t)n * 40 && b.bytes == b.table + 4ull * slots);
            uint8_t* block = static_cast<uint8_t*>(std::malloc(b.bytes));
            cn::stage(list, n, table, b, block);
            CHECK(std::memcmp(block, list, b.table) == 0 && std::memcmp(block + b.table, table, 4ull * slots) == 0);
            if (n > 1) {  // a duplicate is found wherever it stands
                list[n - 1] = list[n / 2 - (n / 2 == n - 1 ? 1 : 0)];
                CHECK(fl::build_table(list, n, mask, table) == n - 1);
            }
            std::free(block), std::free(table), std::free(list);
        }
    const cn::Block none = cn::block_of(0);
    CHECK(none.table == 0 && none.bytes == 4ull * cn::table_slots(0));
}

// The option walk of framesum_accept.h, which the connect call runs on the frame of rule 7 or 8: every
// truncation of each block, in a heap block of exactly its size.
static void test_option_walk() {
    const std::vector<std::vector<uint8_t>> blocks = {
        {2, 4, 0x05, 0xB4},                                    // MSS first
        {1, 1, 1, 2, 4, 0x23, 0x28},                           // behind NOPs
        {3, 3, 7, 2, 4, 0x02, 0x18, 1},                        // behind a window scale
        {2, 3, 9, 2, 4, 0x01, 0x02},                           // a malformed MSS (length 3) in front of a good one
        {0, 2, 4, 0x05, 0xB4},                                 // behind the end of the list
        {8, 10, 1, 2, 3, 4, 5, 6, 7, 8, 2, 4, 0x11, 0x22},      // behind a timestamp
        {4, 0, 2, 4, 9, 9},                                    // a length of 0
        {5, 200, 2, 4, 9, 9},                                  // a length past the block
    };
    const uint32_t whole[] = {0x05B4, 0x2328, 0x0218, 0x0102, 0, 0x1122, 0, 0};
    for (size_t k = 0; k < blocks.size(); ++k) {
        std::vector<uint8_t> full = blocks[k];
        while (full.size() < 40) full.push_back(1);
        for (uint32_t n = 0; n <= 40; ++n) {
            uint8_t* p = static_cast<uint8_t*>(std::malloc(n ? n : 1));
            std::memcpy(p, full.data(), n);
            const uint32_t got = ac::peer_mss(p, n);
            // the value is the whole block's once the option lies inside the truncation, else 0
            CHECK(got == whole[k] || got == 0);
            if (n == 40) CHECK(got == whole[k]);
            if (n == 0) CHECK(got == 0);
            std::free(p);
        }
    }
}

static void test_rejections() {
    std::vector<uint32_t> table, sock_table, closer_table;
    std::vector<fs_cn_sock> good = {opener(1), opener(2, 5, 0, FS_CN_SEND_SYN), opener(3)};
    const auto check = [&](const std::vector<fs_cn_sock>& list, uint32_t reply_flags = 0, bool out = true, bool replies = true,
                           const fs_rx_sock* socks = nullptr, uint32_t n_socks = 0, const fs_cl_sock* closers = nullptr,
                           uint32_t n_closers = 0, uint32_t mask = 0xFFFFFFFFu) {
        return cn::check_openers(list.empty() ? nullptr : list.data(), (uint32_t)list.size(), reply_flags, out, replies, socks,
                                 n_socks, sock_table.data(), closers, n_closers, closer_table.data(), mask, table);
    };
    CHECK(check(good).bad == cn::kConnectGood && table.size() == cn::table_slots(3));
    CHECK(check(good, FS_FCS_APPEND).bad == cn::kConnectGood);
    CHECK(check({}).bad == cn::kConnectGood);
    CHECK(check({}, 0, false, false).bad == cn::kConnectGood);  // nothing listed: no array is needed
    CHECK(check(good, 0, false).bad == cn::kConnectNull);
    CHECK(check(good, 0, true, false).bad == cn::kConnectNull);
    CHECK(cn::check_openers(nullptr, 1, 0, true, true, nullptr, 0, nullptr, nullptr, 0, nullptr, 0xFFFFFFFFu, table).bad ==
          cn::kConnectNull);
    CHECK(cn::check_openers(nullptr, 65537, 0, true, true, nullptr, 0, nullptr, nullptr, 0, nullptr, 0xFFFFFFFFu, table).bad ==
          cn::kTooManyOpeners);
    for (uint32_t rf : {1u, 3u, 4u, 0x80000000u}) CHECK(check(good, rf).bad == cn::kReplyFlags);
    CHECK(check({}, 1).bad == cn::kReplyFlags);
    {
        std::vector<fs_cn_sock> l = good;
        for (uint32_t f : {2u, 3u, 128u}) {
            l = good, l[1].flags = (uint8_t)f;
            CHECK(check(l).bad == cn::kConnectFlags && check(l).index == 1);
        }
        l = good, l[2].key[0] = 17;
        CHECK(check(l).bad == cn::kConnectKeyNotTcp && check(l).index == 2);
        l = good, l[0].reserved[1] = 1;
        CHECK(check(l).bad == cn::kConnectReserved && check(l).index == 0);
        l = good, l[0].reserved[0] = 1;
        CHECK(check(l).bad == cn::kConnectReserved);
        l = good, l[1].reserved2 = 1;
        CHECK(check(l).bad == cn::kConnectReserved && check(l).index == 1);
        l = good, l[2] = good[0], l[2].iss = 77;
        for (uint32_t mask : {0u, 0xFu, 0xFFFFFFFFu}) {
            const cn::CheckConnect c = check(l, 0, true, true, nullptr, 0, nullptr, 0, mask);
            CHECK(c.bad == cn::kConnectEqualKeys && c.index == 2);
        }
    }
    // an opener's key equal to a listed socket's or a closer's, under each mask
    for (uint32_t mask : {0u, 0xFu, 0xFFFFFFFFu}) {
        fs_rx_sock socks[2];
        std::memset(socks, 0, sizeof socks);
        std::memcpy(socks[0].key, opener(9).key, 13);
        std::memcpy(socks[1].key, good[1].key, 13);
        for (fs_rx_sock& s : socks) s.ring_size = 64, s.ring_free = 64;
        socks[1].ring_off = 64;
        CHECK(dl::check_socks(socks, 2, true, true, 128, mask, sock_table).bad == dl::kGood);
        cn::CheckConnect c = check(good, 0, true, true, socks, 2, nullptr, 0, mask);
        CHECK(c.bad == cn::kConnectKeyListed && c.index == 1);
        std::memcpy(socks[1].key, opener(8).key, 13);
        CHECK(dl::check_socks(socks, 2, true, true, 128, mask, sock_table).bad == dl::kGood);
        CHECK(check(good, 0, true, true, socks, 2, nullptr, 0, mask).bad == cn::kConnectGood);
        fs_cl_sock closers[2];
        std::memset(closers, 0, sizeof closers);
        std::memcpy(closers[0].key, opener(7).key, 13);
        std::memcpy(closers[1].key, good[2].key, 13);
        closers[0].state = closers[1].state = 5;
        std::vector<uint32_t> none;
        CHECK(cl::check_closers(closers, 2, true, true, nullptr, 0, none.data(), mask, closer_table).bad == cl::kCloseGood);
        c = check(good, 0, true, true, socks, 2, closers, 2, mask);
        CHECK(c.bad == cn::kConnectKeyCloser && c.index == 2);
        std::memcpy(closers[1].key, opener(6).key, 13);
        CHECK(cl::check_closers(closers, 2, true, true, nullptr, 0, none.data(), mask, closer_table).bad == cl::kCloseGood);
        CHECK(check(good, 0, true, true, socks, 2, closers, 2, mask).bad == cn::kConnectGood);
    }
    for (int b = cn::kConnectNull; b <= cn::kConnectKeyCloser; ++b) CHECK(cn::bad_connect_text((cn::BadConnect)b)[0] != 0);
}

static uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

static void test_untouched_and_templates() {
    const fs_cn_sock s = opener(5, 0xFFFFFFFFu, 70000, FS_CN_SEND_SYN);
    fs_cn_out o = cn::untouched(s);
    CHECK(o.state == 3 && o.irs == 0 && o.rcv_nxt == 0 && o.snd_una == 0xFFFFFFFFu && o.snd_nxt == 0 && o.snd_wnd == 1);
    CHECK(o.n_rejected == 0 && o.n_keepalive == 0 && o.stop == cn::kNone && o.frame == cn::kNone && o.peer_mss == 0);
    CHECK(o.reply == 0 && o.flags == 0 && o.rst_seq == 0);
    CHECK(cn::with_syn(o, s).reply == FS_CN_REPLY_SYN && cn::with_syn(o, opener(5)).reply == 0);
    o.reply = FS_CN_REPLY_ACK;
    CHECK(cn::with_syn(o, s).reply == FS_CN_REPLY_ACK);  // the ACK wins
    uint8_t* h = static_cast<uint8_t*>(std::malloc(54));
    const struct {
        uint8_t reply;
        uint32_t seq, ack, flags;
    } want[] = {{FS_CN_REPLY_ACK, 0u, 0x80000000u, ACK}, {FS_CN_REPLY_SYNACK, 0xFFFFFFFFu, 0x80000000u, SYN | ACK},
                {FS_CN_REPLY_RST, 4242u, 0u, RST}, {FS_CN_REPLY_SYN, 0xFFFFFFFFu, 0u, SYN}};
    for (const auto& w : want) {
        o.reply = w.reply, o.irs = 0x7FFFFFFFu, o.rst_seq = 4242u;
        cn::reply_template(s, o, h);
        CHECK(std::memcmp(h, s.remote_mac, 6) == 0 && std::memcmp(h + 6, s.local_mac, 6) == 0 && h[12] == 8 && h[13] == 0);
        CHECK(h[14] == 0x45 && h[16] == 0 && h[17] == 0 && h[18] == (s.ip_id >> 8) && h[19] == (s.ip_id & 255) && h[22] == 64 && h[23] == 6);
        CHECK(std::memcmp(h + 26, s.key + 5, 4) == 0 && std::memcmp(h + 30, s.key + 1, 4) == 0);
        CHECK(std::memcmp(h + 34, s.key + 11, 2) == 0 && std::memcmp(h + 36, s.key + 9, 2) == 0);
        CHECK(be32(h + 38) == w.seq && be32(h + 42) == w.ack && h[46] == 0x50 && h[47] == w.flags);
        CHECK(h[48] == 0xFF && h[49] == 0xFF && h[50] == 0 && h[51] == 0 && h[52] == 0 && h[53] == 0);  // min(70000, 65535)
    }
    std::free(h);
}

int main() {
    test_rule_over_the_grid();
    test_rule2_derivation();
    test_rule5_derivation();
    test_opener_table();
    test_option_walk();
    test_rejections();
    test_untouched_and_templates();
    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("connect checks OK\n");
    return 0;
}
