// The arithmetic of the close call (seqs_amd/csrc/framesum_close.h) on the CPU, built alone under
// ASan + UBSan by tests/test_close_host.py: code_of and step over the grid of one-frame cases against the
// rule as the header of the call words it (written here again), rule 5's literal window checks against
// its one-line form, is_event against what step does, the closer table under hash masks 0, 0xF and full
// (tables and record lists in heap blocks of exactly their size), every rejection of the closer list, and
// the staged block.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../seqs_amd/csrc/framesum_close.h"

namespace cl = framesum::closing;
namespace fl = framesum::flows;
namespace dl = framesum::deliver;

static int g_failed = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                  \
        }                                                                \
    } while (0)

constexpr uint32_t FIN = 1, SYN = 2, RST = 4, ACK = 16;

// The rule by the words of include/framesum_close.h. Returns the code (0xFF: the walk ends) and the
// connection behind the frame.
struct Conn {
    uint32_t state, nxt, una, wnd, flags;
};
static uint32_t by_the_words(Conn& c, uint32_t snd_nxt, uint32_t rcv_wnd, const cl::Seg& f) {
    (void)rcv_wnd;  // a frame without data passes rule 5 iff Seq == nxt, at every window
    const bool fin = f.flags9 & FIN, ack = f.flags9 & ACK;
    if (c.state == 8 || c.state == 0) return 8;
    if (f.flags9 & SYN) return 0xFF;
    if (f.seq == c.nxt - 1u && f.flags9 == ACK && f.ack == snd_nxt && f.len == 0) return 5;
    if (f.len > 0) return 7;
    if (f.seq != c.nxt) return 4;
    if (f.flags9 & RST) {
        c.state = 0, c.flags |= FS_CL_RESET;
        return 9;
    }
    uint32_t next = c.state;
    bool owed = false;
    if (c.state == 5) {
        if (fin && ack && f.ack == snd_nxt) next = 8;
        else if (fin) next = 7;
        else if (ack) next = 6;
        else return 10;
        owed = true;
    } else if (c.state == 6) {
        if (!(fin && ack)) return 10;
        next = 8, owed = true;
    } else if (c.state == 7) {
        if (ack) next = 8;
    } else if (c.state == 10) {
        if (ack) next = 0;
    }
    c.state = next;
    if (owed) c.flags |= FS_CL_ACK_OWED;
    c.wnd = f.window;
    if (ack) c.una = f.ack;
    if (fin) c.nxt += 1u, c.flags |= FS_CL_FIN;
    return 1;
}

static void test_rule_over_the_grid() {
    const uint32_t states[] = {4, 5, 6, 7, 8, 9, 10, 0};
    const uint32_t nxts[] = {1000u, 0u, 0xFFFFFFFFu};        // Seq and nxt - 1 cross 2^32
    const uint32_t snd_nxts[] = {5000u, 0u, 0xFFFFFFFFu};
    const uint32_t wnds[] = {0u, 1u, 65535u};
    unsigned long cases = 0, events = 0;
    for (uint32_t state : states)
        for (uint32_t nxt : nxts)
            for (uint32_t snd_nxt : snd_nxts)
                for (uint32_t rcv_wnd : wnds)
                    for (uint32_t bits = 0; bits < 16; ++bits)
                        for (uint32_t len = 0; len < 2; ++len)
                            for (int ds = -1; ds <= 1; ++ds)
                                for (int da = -1; da <= 2; ++da) {
                                    const uint32_t una = snd_nxt - 7u;
                                    cl::Seg f;
                                    f.flags9 = ((bits & 1) ? FIN : 0) | ((bits & 2) ? SYN : 0) | ((bits & 4) ? RST : 0) | ((bits & 8) ? ACK : 0);
                                    f.seq = nxt + (uint32_t)ds;
                                    f.ack = da == 2 ? una : snd_nxt + (uint32_t)da;
                                    f.window = 4321u, f.len = len;
                                    if (state == 4 && (!(f.flags9 & RST) || (f.flags9 & SYN))) continue;  // the receive call's frames
                                    const cl::Fixed x{snd_nxt, rcv_wnd};
                                    Conn want{state, nxt, una, 77u, 0u};
                                    const uint32_t wcode = by_the_words(want, snd_nxt, rcv_wnd, f);
                                    const uint32_t code = cl::code_of(state, nxt, x, f);
                                    CHECK(code == wcode);
                                    ++cases;
                                    if (code == cl::kEnds) {
                                        CHECK(cl::is_event(state, code, x, f));
                                        continue;
                                    }
                                    const cl::Ctl before{state, nxt, una, 77u, 0u};
                                    const cl::Ctl got = cl::step(before, code, x, f);
                                    CHECK(got.state == want.state && got.nxt == want.nxt && got.una == want.una &&
                                          got.wnd == want.wnd && got.flags == want.flags);
                                    // an event is exactly a frame that changes the state or rcv.NXT
                                    const bool changes = got.state != state || got.nxt != nxt;
                                    CHECK(cl::is_event(state, code, x, f) == changes);
                                    events += changes;
                                    // what is no event may change snd.UNA and snd.WND only, and only with code 1
                                    if (!changes) CHECK(got.flags == 0u && (code == 1u || (got.una == una && got.wnd == 77u)));
                                    CHECK(cl::counts_rejected(code) == (code == 4u || code == 7u || code == 10u));
                                    // a Closed record carries 0 in its three numbers
                                    const fs_cl_out o = cl::out_of(got, 3u, 4u, 9u);
                                    if (got.state == 0u) CHECK(o.rcv_nxt == 0u && o.snd_una == 0u && o.snd_wnd == 0u);
                                    else CHECK(o.rcv_nxt == got.nxt && o.snd_una == got.una && o.snd_wnd == got.wnd);
                                    CHECK(o.state == got.state && o.n_taken == 3u && o.n_rejected == 4u && o.stop == 9u && o.flags == got.flags);
                                }
    CHECK(cases > 20000 && events > 1000);
}

// Rule 5: the literal cases of control.go:299-311 against "passes iff Seq == nxt", at every window and
// distance that could tell them apart.
static void test_rule5_derivation() {
    const uint32_t nxts[] = {0u, 1u, 1000u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
    const uint32_t wnds[] = {0u, 1u, 2u, 65535u, 65536u, 0x80000000u, 0xFFFFFFFFu};
    const int32_t ds[] = {-65536, -2, -1, 0, 1, 2, 65534, 65535, 65536, INT32_MIN};
    for (uint32_t nxt : nxts)
        for (uint32_t wnd : wnds)
            for (int32_t d : ds)
                for (uint32_t fin = 0; fin < 2; ++fin) {
                    cl::Seg f{nxt + (uint32_t)d, 0u, 0u, fin ? (FIN | ACK) : ACK, 0u};
                    CHECK(cl::seq_checks_pass(nxt, wnd, f) == (d == 0));
                }
}

static fs_cl_sock closer(uint32_t id, uint8_t state = 5) {
    fs_cl_sock c;
    std::memset(&c, 0, sizeof c);
    c.key[0] = 6;
    c.key[1] = 10, c.key[4] = (uint8_t)id, c.key[3] = (uint8_t)(id >> 8), c.key[2] = (uint8_t)(id >> 16);
    c.key[5] = 10, c.key[8] = 1;
    c.key[9] = 0x30, c.key[10] = 0x39, c.key[12] = 80;
    c.state = state;
    c.rcv_nxt = 100 + id, c.rcv_wnd = 8192, c.snd_una = 7, c.snd_nxt = 9, c.snd_wnd = 65535;
    return c;
}

static void test_closer_table() {
    const uint32_t masks[] = {0u, 0xFu, 0xFFFFFFFFu};
    const uint32_t counts[] = {1u, 2u, 17u, 300u};
    for (uint32_t mask : masks)
        for (uint32_t n : counts) {
            // heap blocks of exactly their size: ASan sees a read or a write past them
            fs_cl_sock* list = static_cast<fs_cl_sock*>(std::malloc(n * sizeof(fs_cl_sock)));
            for (uint32_t i = 0; i < n; ++i) list[i] = closer(i, (uint8_t)(5 + i % 6));
            const uint32_t slots = cl::table_slots(n);
            uint32_t* table = static_cast<uint32_t*>(std::malloc(4ull * slots));
            CHECK(fl::build_table(list, n, mask, table) == cl::kNone);
            uint32_t filled = 0;
            for (uint32_t s = 0; s < slots; ++s) filled += table[s] != cl::kNone;
            CHECK(filled == n);
            for (uint32_t i = 0; i < n; ++i) CHECK(fl::lookup(fl::wire_key(list[i].key), list, table, slots - 1u, mask) == i);
            for (uint32_t i = n; i < n + 50u; ++i) {
                const fs_cl_sock other = closer(i);
                CHECK(fl::lookup(fl::wire_key(other.key), list, table, slots - 1u, mask) == cl::kNone);
            }
            // the staged block holds the records, the table and the sockets' fixed values
            fs_rx_sock socks[3];
            std::memset(socks, 0, sizeof socks);
            for (uint32_t i = 0; i < 3; ++i) socks[i].snd_nxt = 50 + i, socks[i].rcv_wnd = 60 + i;
            const cl::Block b = cl::block_of(n, 3);
            CHECK(b.table == (uint64_t)n * 40 && b.socks == b.table + 4ull * slots && b.bytes == b.socks + 24);
            uint8_t* block = static_cast<uint8_t*>(std::malloc(b.bytes));
            cl::stage(list, n, table, socks, 3, b, block);
            CHECK(std::memcmp(block, list, b.table) == 0 && std::memcmp(block + b.table, table, 4ull * slots) == 0);
            cl::Fixed x;
            std::memcpy(&x, block + b.socks + 16, sizeof x);
            CHECK(x.snd_nxt == 52 && x.rcv_wnd == 62);
            // a duplicate is found wherever it stands
            if (n > 1) {
                list[n - 1] = list[n / 2 - (n / 2 == n - 1 ? 1 : 0)];
                CHECK(fl::build_table(list, n, mask, table) == n - 1);
            }
            std::free(block), std::free(table), std::free(list);
        }
}

static void test_rejections() {
    std::vector<uint32_t> table, sock_table;
    std::vector<fs_cl_sock> good = {closer(1, 5), closer(2, 10), closer(3, 8)};
    const auto check = [&](const std::vector<fs_cl_sock>& list, bool out = true, bool sc = true, const fs_rx_sock* socks = nullptr,
                           uint32_t n_socks = 0, uint32_t mask = 0xFFFFFFFFu) {
        return cl::check_closers(list.empty() ? nullptr : list.data(), (uint32_t)list.size(), out, sc, socks, n_socks,
                                 sock_table.data(), mask, table);
    };
    CHECK(check(good).bad == cl::kCloseGood && table.size() == cl::table_slots(3));
    CHECK(check({}).bad == cl::kCloseGood);
    CHECK(check({}, false, false).bad == cl::kCloseGood);  // nothing listed: no array is needed
    CHECK(check(good, false).bad == cl::kCloseNull);
    CHECK(cl::check_closers(nullptr, 1, true, true, nullptr, 0, nullptr, 0xFFFFFFFFu, table).bad == cl::kCloseNull);
    CHECK(cl::check_closers(nullptr, 65537, true, true, nullptr, 0, nullptr, 0xFFFFFFFFu, table).bad == cl::kTooManyClosers);
    for (uint32_t state : {0u, 1u, 4u, 11u, 255u}) {
        std::vector<fs_cl_sock> l = good;
        l[1].state = (uint8_t)state;
        const cl::CheckClose c = check(l);
        CHECK(c.bad == cl::kCloseState && c.index == 1);
    }
    for (uint32_t state = 5; state <= 10; ++state) {
        std::vector<fs_cl_sock> l = good;
        l[2].state = (uint8_t)state;
        CHECK(check(l).bad == cl::kCloseGood);
    }
    {
        std::vector<fs_cl_sock> l = good;
        l[2].key[0] = 17;
        CHECK(check(l).bad == cl::kCloseKeyNotTcp && check(l).index == 2);
        l = good, l[0].reserved[1] = 1;
        CHECK(check(l).bad == cl::kCloseReserved && check(l).index == 0);
        l = good, l[0].reserved[0] = 1;
        CHECK(check(l).bad == cl::kCloseReserved);
        l = good, l[1].reserved2 = 1;
        CHECK(check(l).bad == cl::kCloseReserved && check(l).index == 1);
        l = good, l[1].snd_wnd = 65536;
        CHECK(check(l).bad == cl::kCloseSndWnd && check(l).index == 1);
        l[1].snd_wnd = 65535;
        CHECK(check(l).bad == cl::kCloseGood);
        l = good, l[2] = good[0], l[2].state = 9;
        for (uint32_t mask : {0u, 0xFu, 0xFFFFFFFFu}) {
            const cl::CheckClose c = check(l, true, true, nullptr, 0, mask);
            CHECK(c.bad == cl::kCloseEqualKeys && c.index == 2);
        }
    }
    // a closer's key equal to a listed socket's, under each mask; socks_close is needed with sockets
    for (uint32_t mask : {0u, 0xFu, 0xFFFFFFFFu}) {
        fs_rx_sock socks[2];
        std::memset(socks, 0, sizeof socks);
        std::memcpy(socks[0].key, closer(9).key, 13);
        std::memcpy(socks[1].key, good[1].key, 13);
        for (fs_rx_sock& s : socks) s.ring_size = 64, s.ring_free = 64;
        socks[1].ring_off = 64;
        const dl::Check ok = dl::check_socks(socks, 2, true, true, 128, mask, sock_table);
        CHECK(ok.bad == dl::kGood);
        const cl::CheckClose c = check(good, true, true, socks, 2, mask);
        CHECK(c.bad == cl::kCloseKeyListed && c.index == 1);
        CHECK(check(good, true, false, socks, 2, mask).bad == cl::kCloseNull);
        CHECK(check({}, false, false, socks, 2, mask).bad == cl::kCloseNull);
        std::memcpy(socks[1].key, closer(8).key, 13);
        CHECK(dl::check_socks(socks, 2, true, true, 128, mask, sock_table).bad == dl::kGood);
        CHECK(check(good, true, true, socks, 2, mask).bad == cl::kCloseGood);
    }
    for (int b = cl::kCloseNull; b <= cl::kCloseSndWnd; ++b) CHECK(cl::bad_close_text((cl::BadClose)b)[0] != 0);
}

static void test_untouched() {
    const fs_cl_sock c = closer(5, 9);
    const fs_cl_out o = cl::untouched_closer(c);
    CHECK(o.state == 9 && o.rcv_nxt == c.rcv_nxt && o.snd_una == 7 && o.snd_wnd == 65535 && o.n_taken == 0 && o.n_rejected == 0 &&
          o.stop == FS_DELIVER_NONE && o.flags == 0);
    const fs_cl_out s = cl::untouched_sock(11, 12, 13, 14);
    CHECK(s.state == 4 && s.rcv_nxt == 11 && s.snd_una == 12 && s.snd_wnd == 13 && s.stop == 14 && s.flags == 0);
}

int main() {
    test_rule_over_the_grid();
    test_rule5_derivation();
    test_closer_table();
    test_rejections();
    test_untouched();
    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("close checks OK\n");
    return 0;
}
