// The arithmetic of the receive call (seqs_amd/csrc/framesum_recv.h) on the CPU, built alone under
// ASan + UBSan by tests/test_recv_host.py: every rejection of the send-side list, code_of on both
// sides of every comparison, the dword at L4 + 12, and the scan operator -- associativity over a
// small exhaustive set of values and folds by composition against frame-by-frame stepping, both with
// the distance 2^31 among the values.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../seqs_amd/csrc/framesum_recv.h"

namespace rv = framesum::recv;
using framesum::coalesce::kFin;
using framesum::coalesce::kPsh;
using framesum::deliver::kAck;

static int g_failed = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                  \
        }                                                                \
    } while (0)

static rv::Frame frame(uint32_t seq, uint32_t ack, uint32_t flags9, uint32_t len, bool admitted = false, uint32_t window = 777) {
    rv::Frame f;
    f.seq = seq, f.ack = ack, f.window = window, f.flags9 = flags9, f.len = len, f.admitted = admitted;
    return f;
}

static void test_checks() {
    std::vector<fs_rx_sock> socks(3);
    std::memset(socks.data(), 0, 3 * sizeof(fs_rx_sock));
    std::vector<fs_rx_snd> snd(3);
    for (uint32_t i = 0; i < 3; ++i) socks[i].snd_nxt = 1000u, snd[i] = fs_rx_snd{990u, 65535u};
    CHECK(rv::check_snd(socks.data(), snd.data(), 3, true).bad == rv::kSndGood);
    CHECK(rv::check_snd(nullptr, nullptr, 0, false).bad == rv::kSndGood);  // no sockets: nothing to check
    CHECK(rv::check_snd(socks.data(), nullptr, 3, true).bad == rv::kSndNull);
    CHECK(rv::check_snd(socks.data(), snd.data(), 3, false).bad == rv::kSndNull);
    snd[2].snd_wnd = 65536u;
    rv::CheckSnd c = rv::check_snd(socks.data(), snd.data(), 3, true);
    CHECK(c.bad == rv::kSndWnd && c.sock == 2);
    snd[2].snd_wnd = 0u;
    // snd_una against snd_nxt: equal, one ahead, 2^31 - 1 ahead (ahead), 2^31 behind (passes), one behind
    const struct { uint32_t una; bool good; } cases[] = {{1000u, true}, {1001u, false}, {1000u + 0x7FFFFFFFu, false},
                                                         {1000u + 0x80000000u, true}, {999u, true}};
    for (const auto& k : cases) {
        snd[1].snd_una = k.una;
        c = rv::check_snd(socks.data(), snd.data(), 3, true);
        CHECK((c.bad == rv::kSndGood) == k.good);
        if (!k.good) CHECK(c.bad == rv::kSndUnaAhead && c.sock == 1);
    }
    snd[1].snd_una = 5u, socks[1].snd_nxt = 3u;  // across 2^32: 0xFFFFFFFE .. 3 .. 5
    CHECK(rv::check_snd(socks.data(), snd.data(), 3, true).bad == rv::kSndUnaAhead);
    snd[1].snd_una = 0xFFFFFFFEu;
    CHECK(rv::check_snd(socks.data(), snd.data(), 3, true).bad == rv::kSndGood);
    for (int b = rv::kSndNull; b <= rv::kSndUnaAhead; ++b) CHECK(std::strlen(rv::bad_snd_text((rv::BadSnd)b)) > 0);
    std::vector<rv::Sock> staged(3);
    socks[0].rcv_nxt = 7, socks[0].rcv_wnd = 8, snd[0] = fs_rx_snd{11u, 12u};
    rv::stage(socks.data(), snd.data(), 3, staged.data());
    CHECK(staged[0].snd_una == 11 && staged[0].snd_wnd == 12 && staged[0].snd_nxt == 1000 && staged[0].rcv_wnd == 8 &&
          staged[0].rcv_nxt == 7 && staged[1].snd_nxt == 3);
    const fs_rx_snd_out u = rv::untouched(5u, 6u);
    CHECK(u.snd_una == 5 && u.snd_wnd == 6 && (u.n_taken | u.n_dup | u.n_unsent | u.n_rejected | u.n_keepalive | u.flags) == 0);
}

static void test_dword12() {
    // bytes: data offset 5 with NS, flags ACK | PSH, window 0x1234 -- as a little-endian load sees them
    const uint32_t w = 0x51u | (0x18u << 8) | (0x12u << 16) | (0x34u << 24);
    CHECK(rv::flags9_of(w) == (rv::kNs | kAck | kPsh) && rv::window_of(w) == 0x1234u);
    CHECK(rv::flags9_of(0xFFFF00FEu) == 0u && rv::window_of(0xFFFF00FEu) == 0xFFFFu);
    CHECK(rv::flags9_of(0x0000FF01u) == 0x1FFu && rv::window_of(0x0000FF01u) == 0u);
}

static void test_comparisons() {
    CHECK(rv::less_than(1u, 2u) && !rv::less_than(2u, 2u) && !rv::less_than(3u, 2u));
    CHECK(rv::less_than(0xFFFFFFFFu, 0u) && !rv::less_than(0u, 0xFFFFFFFFu));
    // exactly half the space apart: each is "less than" the other
    CHECK(rv::less_than(0u, 0x80000000u) && rv::less_than(0x80000000u, 0u));
    CHECK(!rv::less_than(0u, 0x7FFFFFFFu + 2u) && rv::less_than(0u, 0x7FFFFFFFu));
    CHECK(rv::less_than_eq(5u, 5u) && rv::less_than_eq(4u, 5u) && !rv::less_than_eq(6u, 5u));
}

static void test_code_of() {
    const uint32_t bases[] = {1000u, 0xFFFFFFFFu, 0u, 1u};  // rcv.NXT and snd.NXT on both sides of 2^32
    for (uint32_t nxt : bases)
        for (uint32_t snd : bases) {
            const uint32_t una = snd - 10u;
            // the keepalive comes first: Seq, the flags and the Ack must all fit
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt - 1u, snd, kAck, 0)) == rv::kKeepalive);
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt - 1u, snd - 1u, kAck, 0)) == rv::kRejected);
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt - 1u, snd, kAck | kPsh, 0)) == rv::kRejected);
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt - 1u, snd, kAck | rv::kNs, 0)) == rv::kRejected);
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt - 2u, snd, kAck, 0)) == rv::kRejected);
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt - 1u, snd, kAck, 1)) == rv::kRejected);  // with data: no keepalive
            // Seq
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt + 1u, snd, kAck, 0)) == rv::kRejected);
            CHECK(rv::code_of(una, nxt, snd, 0, frame(nxt, snd, kAck, 0)) == rv::kTaken);  // zeroWindowOK
            // the duplicate test: Ack below, at and above una
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt, una - 1u, kAck, 0)) == rv::kDuplicate);
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt, una, kAck, 0)) == rv::kDuplicate);
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt, una + 1u, kAck, 0)) == rv::kTaken);
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt, una, 0, 0)) == rv::kTaken);       // no ACK flag: no test
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt, una, kPsh, 0)) == rv::kTaken);
            // unsent data: Ack at and above snd_nxt
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt, snd, kAck, 0)) == rv::kTaken);
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt, snd + 1u, kAck, 0)) == rv::kUnsent);
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt, snd + 1u, kPsh, 0)) == rv::kTaken);
            // the 2^31 point: una == snd_nxt, an Ack exactly 2^31 behind compares as newer
            CHECK(rv::code_of(snd, nxt, snd, 100, frame(nxt, snd - rv::kHalf, kAck, 0)) == rv::kTaken);
            CHECK(rv::code_of(snd, nxt, snd, 100, frame(nxt, snd - rv::kHalf + 1u, kAck, 0)) == rv::kDuplicate);
            CHECK(rv::code_of(snd, nxt, snd, 100, frame(nxt, snd - rv::kHalf - 1u, kAck, 0)) == rv::kUnsent);
            CHECK(rv::code_of(snd - 1u, nxt, snd, 100, frame(nxt, snd - rv::kHalf, kAck, 0)) == rv::kDuplicate);
            // considered frames: admitted is the delivery's word
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt, una - 5u, kAck, 10, true)) == rv::kTaken);  // no duplicate test
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt, snd, kAck | kFin, 0, true)) == rv::kTaken);
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt + 1u, snd, kAck, 10)) == rv::kRejected);     // (a)
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt, snd, kAck, 101)) == rv::kRejected);         // (b)
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt, snd, kAck | kFin, 100)) == rv::kRejected);  // (b): the FIN counts
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt, snd, kAck, 100)) == rv::kRingFull);
            CHECK(rv::code_of(una, nxt, snd, 0, frame(nxt, snd, kAck | kFin, 0)) == rv::kRejected);
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt, snd + 1u, kAck, 10)) == rv::kUnsent);       // (c)
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt, snd + 1u, kPsh, 10)) == rv::kRingFull);     // (c) needs ACK
            CHECK(rv::code_of(una, nxt, snd, 100, frame(nxt + 1u, snd + 1u, kAck, 10)) == rv::kRejected);  // (a) before (c)
        }
    // step and owes_ack
    rv::Snd s{5u, 6u};
    rv::Snd t = rv::step(s, rv::kTaken, frame(0, 9u, kAck, 0, false, 4321u));
    CHECK(t.una == 9u && t.wnd == 4321u);
    t = rv::step(s, rv::kTaken, frame(0, 9u, kPsh, 0, false, 4321u));
    CHECK(t.una == 5u && t.wnd == 4321u);
    for (uint32_t c = rv::kDuplicate; c <= rv::kRingFull; ++c) {
        t = rv::step(s, c, frame(0, 9u, kAck, 0, false, 4321u));
        CHECK(t.una == 5u && t.wnd == 6u);
    }
    CHECK(rv::owes_ack(rv::kTaken, frame(0, 0, kAck, 1, true)) && rv::owes_ack(rv::kTaken, frame(0, 0, kAck | kFin, 0, true)));
    CHECK(!rv::owes_ack(rv::kTaken, frame(0, 0, kAck, 0)) && rv::owes_ack(rv::kUnsent, frame(0, 0, kAck, 0)));
    CHECK(!rv::owes_ack(rv::kDuplicate, frame(0, 0, kAck, 0)) && !rv::owes_ack(rv::kRingFull, frame(0, 0, kAck, 1)));
}

static void test_operator() {
    // associativity, exhaustively over a small set of values with 2^31 among them
    const uint32_t vals[] = {0u, 1u, 2u, 0x7FFFFFFFu, rv::kHalf, 0xFFFFFFFFu};
    std::vector<rv::Fn> fns;
    for (uint32_t set = 0; set < 2; ++set)
        for (uint32_t v : vals) fns.push_back(rv::Fn{set, v});
    for (const rv::Fn& f : fns)
        for (const rv::Fn& g : fns)
            for (const rv::Fn& h : fns) {
                const rv::Fn a = rv::compose(rv::compose(f, g), h), b = rv::compose(f, rv::compose(g, h));
                for (uint32_t d : vals) {
                    if (d > rv::kHalf) continue;
                    CHECK(rv::apply(a, d) == rv::apply(b, d));
                    CHECK(rv::apply(a, d) == rv::apply(h, rv::apply(g, rv::apply(f, d))));
                }
            }
    for (const rv::Fn& f : fns)
        for (uint32_t d : vals)
            CHECK(rv::apply(rv::compose(rv::identity(), f), d) == rv::apply(f, d) &&
                  rv::apply(rv::compose(f, rv::identity()), d) == rv::apply(f, d));

    // folds by composition against frame-by-frame stepping: random frames around snd_nxt, whose Acks
    // lie at the distances 0, 1, 2, 2^31 - 1, 2^31, 2^31 + 1 and -1 behind it. A sequence with a frame
    // at the 2^31 point is the walk's lane-by-lane case: there the fold may differ, and does when una
    // is snd_nxt.
    const uint32_t dist[] = {0u, 1u, 2u, 5u, 0x7FFFFFFFu, rv::kHalf, rv::kHalf + 1u, 0xFFFFFFFFu};
    uint32_t rng = 12345u;
    auto next = [&]() { return rng = rng * 1664525u + 1013904223u, rng >> 8; };
    int with_half = 0, fold_differs = 0, folds = 0;
    for (int round = 0; round < 20000; ++round) {
        const uint32_t snd = (round & 1) ? 3u : 0x9000000u, nxt0 = (round & 2) ? 0xFFFFFFFDu : 500u;
        const uint32_t una0 = snd - dist[next() % 6u];  // at most 2^31 behind
        const uint32_t count = 1u + next() % 9u;
        uint32_t una = una0, nxt = nxt0;
        rv::Fn fold = rv::identity();
        uint64_t least = rv::kKeyIdentity;  // the fold as the minimum of the lanes' keys
        uint32_t constants = 0;
        bool half = false;
        for (uint32_t k = 0; k < count; ++k) {
            const uint32_t kind = next() % 6u;
            const uint32_t ack = snd - dist[next() % 8u];
            const uint32_t flags9 = (next() % 4u ? kAck : 0u) | (next() % 8u == 0 ? kPsh : 0u);
            rv::Frame f;
            if (kind < 3) f = frame(nxt - (kind == 2 ? 1u : 0u), ack, flags9, 0);                    // pure, in or out of order
            else if (kind == 3) f = frame(nxt, ack, flags9, 7, rv::less_than_eq(ack, snd) || !(flags9 & kAck));  // data
            else if (kind == 4) f = frame(nxt + 3u, ack, flags9, 7);                                  // data out of order
            else f = frame(nxt, ack, flags9, 70000u);                                                 // above the window
            half = half || rv::at_half(nxt, snd, f);
            const rv::Fn fn = rv::fn_of(nxt, snd, f);
            fold = rv::compose(fold, fn);
            constants += fn.set;
            const uint64_t key = rv::scan_key(fn, constants);
            least = key < least ? key : least;
            CHECK(rv::fn_of_key(least).set == fold.set && rv::apply(rv::fn_of_key(least), snd - una0) == rv::apply(fold, snd - una0));
            const uint32_t c = rv::code_of(una, nxt, snd, 65535u, f);
            una = rv::step(rv::Snd{una, 0u}, c, f).una;
            if (f.admitted) nxt += f.len;
            CHECK(snd - una <= rv::kHalf);  // the invariant the distance form rests on
        }
        const uint32_t folded = snd - rv::apply(fold, snd - una0);
        if (half) {
            ++with_half;
            if (folded != una) ++fold_differs;
        } else {
            ++folds;
            CHECK(folded == una);
        }
    }
    CHECK(folds > 5000 && with_half > 1000 && fold_differs > 0);
    // 64 constants in a chunk: the key's high word reaches 0, and the identity key is the identity
    CHECK(rv::fn_of_key(rv::scan_key(rv::Fn{1u, 7u}, 64u)).set == 1u && rv::scan_key(rv::Fn{1u, 7u}, 64u) == 7u);
    CHECK(rv::fn_of_key(rv::kKeyIdentity).set == 0u && rv::apply(rv::fn_of_key(rv::kKeyIdentity), rv::kHalf) == rv::kHalf);
    CHECK(rv::scan_key(rv::identity(), 0u) == rv::kKeyIdentity);
    // the point itself: una == snd_nxt, an Ack 2^31 behind is taken by the literal rule, not by min()
    const uint32_t snd = 77u;
    const rv::Frame f = frame(500u, snd - rv::kHalf, kAck, 0);
    CHECK(rv::at_half(500u, snd, f) && !rv::at_half(501u, snd, f) && !rv::at_half(500u, snd + 1u, f));
    CHECK(rv::code_of(snd, 500u, snd, 100u, f) == rv::kTaken);
    CHECK(rv::apply(rv::fn_of(500u, snd, f), 0u) == 0u);  // what the fold would say: una stays
    CHECK(rv::step(rv::Snd{snd, 0u}, rv::kTaken, f).una == snd - rv::kHalf);
}

int main() {
    test_checks();
    test_dword12();
    test_comparisons();
    test_code_of();
    test_operator();
    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("recv checks OK\n");
    return 0;
}
