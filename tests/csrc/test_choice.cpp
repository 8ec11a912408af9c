// Checks of seqs_amd/csrc/framesum_choice.h (which kernel a launch runs, what it is asked to
// report, the grid), built on its own under ASan + UBSan (tests/csrc/Makefile, run by
// tests/test_host_sanitizers.py). choose() is driven by a model of what the kernels post into the
// report block, every scenario once with the posts visible to the next launch (a caller that
// synchronizes) and once with posts that land kLate launches later (launches enqueued ahead of the GPU).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <deque>

#include "../../seqs_amd/csrc/framesum_choice.h"

using namespace framesum;

static int g_fail = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            if (++g_fail > 20) std::exit(1);                                  \
        }                                                                     \
    } while (0)

// A batch as the kernels' reports see it: how the lengths of its tiles mix (mixed_class), whether
// the grid's first tile holds a frame longer than kSmallMaxLen, and whether any other tile does.
enum Mix { kNone, kPieces, kGiant };
struct Traffic {
    Mix mix;
    bool first_long, other_long;
};
constexpr Traffic kShort{kNone, false, false};     // 47-B frames
constexpr Traffic kUniform{kNone, true, true};     // 1500-B frames
constexpr Traffic kMixedLen{kPieces, true, true};  // short and long frames in one tile
constexpr Traffic kGiantLen{kGiant, true, true};   // ... and one longer than the pieces cover
constexpr Traffic kOneLong{kNone, false, true};    // short frames, a long one in a later tile

constexpr uint32_t kLate = 5;

// A context and its report block. Launch k's posts are in the block when launch k + 1 + late chooses.
struct Sim {
    ChoiceState st;
    Reports blk{0u, 0u, 0u};
    bool has_block = true;
    uint32_t late = 0;
    uint32_t launches = 0;
    struct Post {
        uint32_t due;
        int word;
        uint32_t value;
    };
    std::deque<Post> inflight;

    void post(int word, uint32_t value) { inflight.push_back(Post{launches + 1u + late, word, value}); }

    // the kernels' posting rules: tile_posts / post_tile, the segment kernel's posts_of, and the
    // small-frame kernel's loop (framesum_kernel.hip)
    void run_kernel(const Choice& c, const Traffic& t) {
        if (c.variant == (uint32_t)kKernelSmall) {
            if (t.first_long || t.other_long) post(kReportLong, c.id);
            return;
        }
        const bool ask_ran = (c.bits & kAskRan) != 0u, watch = (c.bits & kReportWatch) != 0u;
        if (t.mix != kNone && (c.variant == (uint32_t)kKernelOnePass || (c.bits & kAskMixed) != 0u))
            post(kReportLatest, c.id | (t.mix == kGiant ? kReportMixedGiant : 0u));
        if (ask_ran) post(kReportRan, c.id | (t.first_long ? kReportRanLong : 0u));
        if (watch && (t.other_long || (t.first_long && !ask_ran))) post(kReportLong, c.id);
    }

    Choice launch(int force, const Traffic& t, bool fill = false) {
        ++launches;
        while (!inflight.empty() && inflight.front().due <= launches) {
            const Post p = inflight.front();
            inflight.pop_front();
            (p.word == kReportLatest ? blk.latest : p.word == kReportLong ? blk.lng : blk.ran) = p.value;
        }
        const uint32_t seq = st.next_seq;
        const Choice c = choose(st, has_block ? &blk : nullptr, force, fill);
        CHECK(st.next_seq == seq + 1u && st.chosen == c.variant);
        CHECK(c.id == ((seq & 0xFFFFu) ? (seq & 0xFFFFu) : 0x8000u));
        CHECK((c.bits & ~(kAskRan | kAskMixed | kReportWatch)) == 0u);
        CHECK(c.variant == 2u || c.variant == 3u || c.variant == 4u || c.variant == 8u);
        if (has_block) run_kernel(c, t);
        else CHECK(c.bits == 0u);
        return c;
    }
};

static Sim fresh(uint32_t late) {
    Sim s;
    s.late = late;
    return s;
}

// 1. uniform 1500-B traffic, automatic: the mixed-length kernel for the initial window, then the
// one-pass kernel; "ran" asked on every 4th launch only (each answer carries the long flag, so no
// short streak starts); "mixed" asked on every launch, as no mixed report ever arrives
static void uniform_traffic(uint32_t late) {
    Sim s = fresh(late);
    for (uint32_t i = 1; i <= 300; ++i) {
        const Choice c = s.launch(kKernelAuto, kUniform);
        CHECK(c.variant == (i <= kInitialMixedLaunches ? 2u : 4u));
        CHECK(c.bits == (kAskMixed | (i % kRanSample == 0u ? kAskRan : 0u)));
    }
    CHECK(s.st.short_streak == 0u && s.st.long_ever == 1u && s.st.initial == 0u);
}

// 2. mixed traffic keeps the mixed-length kernel from the first launch, asked for its mixed tiles
// until the first report is in and on every 32nd launch after; once the traffic is uniform the
// window ends kStickyLaunches launches after the host last saw the report word change
static void mixed_traffic(uint32_t late) {
    Sim s = fresh(late);
    for (uint32_t i = 1; i <= 300; ++i) {
        const Choice c = s.launch(kKernelAuto, kMixedLen);
        CHECK(c.variant == 2u);
        const bool ask_mixed = i <= 1u + late || i % kMixedSample == 0u;
        CHECK(c.bits == ((ask_mixed ? kAskMixed : 0u) | (i % kRanSample == 0u ? kAskRan : 0u)));
    }
    // the latest post (launch 288) was seen by launch 289 + late
    CHECK(s.st.seen == 288u && s.st.seen_seq == 289u + late);
    const uint32_t last = 289u + late + kStickyLaunches;  // = 4385 + late
    for (uint32_t i = 301; i <= last + 200u; ++i) {
        const Choice c = s.launch(kKernelAuto, kUniform);
        CHECK(c.variant == (i <= last ? 2u : 4u));
    }
    CHECK(s.st.seen_seq == 289u + late);
}

// 3. the 16-bit ids wrap: an old report whose id comes round again is not taken for a new one, and
// mixed traffic keeps its kernel across the wrap, where id 0 is replaced by 0x8000
static void id_wrap(uint32_t late) {
    Sim s = fresh(late);
    CHECK(s.launch(kKernelAuto, kMixedLen).variant == 2u);  // posts kReportLatest = 1
    const uint32_t last = 2u + late + kStickyLaunches;
    for (uint32_t i = 2; i <= 70001u; ++i) {
        const Choice c = s.launch(kKernelAuto, kUniform);
        CHECK(c.variant == (i <= last ? 2u : 4u));  // (launch 65537 carries id 1 again)
    }
    CHECK(s.blk.latest == 1u && s.st.seen_seq == 2u + late);

    Sim m = fresh(late);
    for (uint32_t i = 1; i <= 66000u; ++i) {
        const Choice c = m.launch(kKernelAuto, kMixedLen);
        CHECK(c.variant == 2u);
        if (i == 65536u) CHECK(c.id == 0x8000u && (c.bits & kAskMixed) != 0u);
        if (i == 65537u + late) CHECK(m.blk.latest == 0x8000u && m.st.seen_seq == i);
    }
}

// 4. tiles with a frame longer than the pieces cover: the automatic choice moves to the segment
// kernel once the report is in; a forced kernel stays
static void giant_tiles(uint32_t late) {
    Sim a = fresh(late);
    for (uint32_t i = 1; i <= 300; ++i) CHECK(a.launch(kKernelAuto, kGiantLen).variant == (i <= 1u + late ? 2u : 3u));
    for (int force : {kKernelMixed, kKernelOnePass, kKernelSegment}) {
        Sim s = fresh(late);
        for (uint32_t i = 1; i <= 300; ++i) CHECK(s.launch(force, kGiantLen).variant == (uint32_t)force);
    }
    // the one-pass kernel reported the giant tiles all along: the automatic choice takes them up
    Sim s = fresh(late);
    for (uint32_t i = 1; i <= 40; ++i) s.launch(kKernelOnePass, kGiantLen);
    CHECK((s.blk.latest & kReportMixedGiant) != 0u);
    CHECK(s.launch(kKernelAuto, kGiantLen).variant == 3u);
    Sim n = fresh(late);  // the segment kernel forced, with no report block
    n.has_block = false;
    for (uint32_t i = 1; i <= 40; ++i) CHECK(n.launch(kKernelSegment, kGiantLen).variant == 3u);
}

// 5. 47-B traffic, automatic: the small-frame kernel once kShortLaunchesAuto launches were seen to
// run short (the first "ran" is asked at launch 4 and, while the host counts, on every launch), a
// long frame under it brings the 4-lane kernels back, and 16 more counted launches the small one
static void short_traffic(uint32_t late, uint32_t first_small) {
    Sim s = fresh(late);
    for (uint32_t i = 1; i < first_small + 39u; ++i) {
        const Choice c = s.launch(kKernelAuto, kShort);
        CHECK(c.variant == (i <= kInitialMixedLaunches ? 2u : i < first_small ? 4u : 8u));
        // the first answer (launch 4's) is in at launch 5 + late: from then on the host counts
        const bool counting = i >= 5u + late;
        CHECK(c.bits == (kAskMixed | (counting ? kAskRan | kReportWatch : i % kRanSample == 0u ? kAskRan : 0u)));
    }
    if (late != 0u) return;
    // (posts visible at once) launch L meets a long frame under the small-frame kernel
    const uint32_t L = s.launches + 1u;
    CHECK(L % 4u == 3u);
    CHECK(s.launch(kKernelAuto, kOneLong).variant == 8u);
    // L + 1 sees the report; it is a multiple of 4, so it asks "ran", and L + 2 counts 1
    for (uint32_t i = L + 1u; i <= L + 60u; ++i) {
        const Choice c = s.launch(kKernelAuto, kShort);
        CHECK(c.variant == (i < L + 17u ? 4u : 8u));
        CHECK(s.st.short_streak == (i < L + 17u ? i - (L + 1u) : 16u));
    }
}

// 6. variant 8: the small-frame kernel from the first launch, the 4-lane choice after a long
// report until kShortLaunchesSmall launches ran short; with no report block always the small one
static void variant8(uint32_t late) {
    Sim s = fresh(late);
    for (uint32_t i = 1; i <= 19; ++i) {
        const Choice c = s.launch(kKernelSmall, kShort);
        CHECK(c.variant == 8u && c.bits == (kAskRan | kAskMixed));
    }
    CHECK(s.st.initial == 0u);  // (the initial window counts down under any choice)
    CHECK(s.launch(kKernelSmall, kOneLong).variant == 8u);  // launch 20 posts the long report
    // ... which is in at launch 21 + late; the two 4-lane launches after it answer "ran" short, and
    // the second answer is in 2 + late launches after the report
    for (uint32_t i = 21; i <= 60; ++i) {
        const Choice c = s.launch(kKernelSmall, kShort);
        const bool four_lane = i >= 21u + late && i < 23u + 2u * late;
        CHECK(c.variant == (four_lane ? 4u : 8u));
        CHECK((c.bits & kAskRan) != 0u);
    }
    CHECK(s.st.long_ever == 1u && s.st.short_streak >= kShortLaunchesSmall);

    Sim n = fresh(late);
    n.has_block = false;
    for (uint32_t i = 1; i <= 40; ++i) CHECK(n.launch(kKernelSmall, i % 7u == 0u ? kUniform : kShort).variant == 8u);
    CHECK(n.launch(kKernelSmall, kShort, true).variant == 4u);  // (a fill: never the small-frame kernel)
}

// 7. the host-staged path's force values
static void host_forces(uint32_t late) {
    Sim s = fresh(late);
    CHECK(s.launch(kForceSmallExact, kShort).variant == 8u);
    CHECK(s.launch(kForceSmallExact, kShort, true).variant == 2u);  // a fill (in the initial window)
    CHECK(s.st.initial == kInitialMixedLaunches - 2u);
    Sim u = fresh(late);
    CHECK(u.launch(kForceUniformHost, kUniform).variant == 4u);
    CHECK(u.st.initial == kInitialMixedLaunches - 1u);
    CHECK(u.launch(kKernelAuto, kUniform).variant == 2u);  // (the window is still the device-resident launches')
    // a long short streak, then kForceNoSmall: the 4-lane choice, and the streak goes on
    Sim n = fresh(late);
    for (uint32_t i = 1; i <= 80; ++i) n.launch(kKernelAuto, kShort);
    CHECK(n.st.chosen == 8u && n.st.short_streak >= kShortLaunchesAuto);
    for (uint32_t i = 1; i <= 80; ++i) {
        const Choice c = n.launch(kForceNoSmall, kShort);
        CHECK(c.variant == 4u && (c.bits & (kAskRan | kReportWatch)) == (kAskRan | kReportWatch));
    }
    CHECK(n.launch(kKernelAuto, kShort).variant == 8u);
    CHECK(n.launch(kForceUniformHost, kShort).variant == 4u);
    CHECK(n.launch(kForceSmallExact, kUniform).variant == 8u);

    // host_force: the context's variant unless it is 0 or 8; then by the batch's lengths
    for (int v : {kKernelMixed, kKernelSegment, kKernelOnePass, kForceSmallExact, kForceNoSmall, kForceUniformHost}) {
        CHECK(host_force(v, 47u, 47u) == v);
        CHECK(host_force(v, 9000u, 1u) == v);
    }
    for (int v : {kKernelAuto, kKernelSmall}) {
        CHECK(host_force(v, 0u, 0u) == kForceSmallExact);
        CHECK(host_force(v, 128u, 1u) == kForceSmallExact);
        CHECK(host_force(v, 129u, 1u) == kForceUniformHost);  // span 128
        CHECK(host_force(v, 129u, 129u) == kForceUniformHost);
        CHECK(host_force(v, 1500u, 1245u) == kForceUniformHost);  // span 255
        CHECK(host_force(v, 1500u, 1244u) == kForceNoSmall);      // span 256
        CHECK(host_force(v, 9000u, 0u) == kForceNoSmall);
        CHECK(host_force(v, 0xFFFFFFFFu, 0u) == kForceNoSmall);
    }
}

// 8. a TX fill never runs the small-frame kernel, whatever the streak or the force value
static void fill_never_small(uint32_t late) {
    Sim s = fresh(late);
    for (uint32_t i = 1; i <= 80; ++i) s.launch(kKernelAuto, kShort);
    CHECK(s.st.chosen == 8u);
    for (int force : {kKernelAuto, kKernelSmall, kForceSmallExact, kForceNoSmall, kForceUniformHost})
        CHECK(s.launch(force, kShort, true).variant == 4u);
    CHECK(s.launch(kKernelMixed, kShort, true).variant == 2u);
    CHECK(s.launch(kKernelSegment, kShort, true).variant == 3u);
    CHECK(s.launch(kKernelAuto, kShort).variant == 8u);
}

// 9. no report block, automatic: the one-pass kernel, nothing asked, nothing remembered
static void no_block() {
    Sim s = fresh(0);
    s.has_block = false;
    for (uint32_t i = 1; i <= 100; ++i) {
        const Choice c = s.launch(kKernelAuto, i % 3u ? kMixedLen : kShort);
        CHECK(c.variant == 4u && c.bits == 0u);
    }
    CHECK(s.st.initial == kInitialMixedLaunches && s.st.seen == 0u && s.st.short_streak == 0u && s.st.long_ever == 0u);
}

// 10. the grids
static void grids() {
    constexpr uint32_t kWaves = 16, kFpt = 16, kSmallWaves = 4;
    auto g4 = [&](uint32_t n, uint32_t mb) { return grid_4lane(n, mb, kWaves, kFpt); };
    for (uint32_t mb : {1u, 3u, 256u}) {
        const uint32_t W = kWaves * mb;  // the grid's waves
        // 16 frames per tile while that gives every wave a tile, else 8, else 4
        for (uint32_t f : {16u, 8u}) {
            CHECK(g4(f * W, mb).fpt == f && g4(f * W, mb).blocks == mb);
            CHECK(g4(f * W - 1u, mb).fpt == f && g4(f * W - 1u, mb).blocks == mb);  // (W tiles, the last one short)
            CHECK(g4(f * (W - 1u) + 1u, mb).fpt == f);
            CHECK(g4(f * (W - 1u), mb).fpt == f / 2u);  // W - 1 tiles: halved
            CHECK(g4(f * (W - 1u), mb).blocks == mb);
        }
        CHECK(g4(4u * W, mb).fpt == 4u && g4(4u * W, mb).blocks == mb);
        CHECK(g4(4u * W - 1u, mb).fpt == 4u && g4(4u * W - 1u, mb).blocks == mb);
        CHECK(g4(4u * (W - 1u), mb).fpt == 4u && g4(4u * (W - 1u), mb).blocks == mb);  // (W - 1 tiles still need mb groups)
        if (mb > 1u) CHECK(g4(4u * (W - kWaves), mb).blocks == mb - 1u);
        CHECK(g4(1u, mb).fpt == 4u && g4(1u, mb).blocks == 1u);
        CHECK(g4(0x80000000u, mb).fpt == 16u && g4(0x80000000u, mb).blocks == mb);  // (n + 15 does not wrap)
        CHECK(g4(16u * W + 1u, mb).blocks == mb);
        // every n up to past the 16-frame boundary: the most frames per tile that leave no wave idle
        for (uint32_t n = 1; n <= 16u * W + 40u; n += (mb == 256u ? 7u : 1u)) {
            const uint32_t f = (n + 15u) / 16u >= W ? 16u : (n + 7u) / 8u >= W ? 8u : 4u;
            const uint32_t tiles = (n + f - 1u) / f, blocks = (tiles + kWaves - 1u) / kWaves;
            CHECK(g4(n, mb).fpt == f && g4(n, mb).blocks == (blocks < mb ? blocks : mb) && g4(n, mb).blocks >= 1u);
        }
        // the small-frame kernel: 256 frames per group, at most 2 groups per CU
        CHECK(grid_small(1u, mb, kSmallWaves) == 1u);
        CHECK(grid_small(256u, mb, kSmallWaves) == 1u);
        CHECK(grid_small(257u, mb, kSmallWaves) == 2u);
        CHECK(grid_small(256u * (2u * mb - 1u), mb, kSmallWaves) == 2u * mb - 1u);
        CHECK(grid_small(256u * 2u * mb, mb, kSmallWaves) == 2u * mb);
        CHECK(grid_small(256u * 2u * mb + 1u, mb, kSmallWaves) == 2u * mb);
        CHECK(grid_small(0x80000000u, mb, kSmallWaves) == 2u * mb);  // (n + 63 does not wrap)
    }
}

int main() {
    for (uint32_t late : {0u, kLate}) {
        uniform_traffic(late);
        mixed_traffic(late);
        id_wrap(late);
        giant_tiles(late);
        // the count of short launches starts with launch 4's answer: at once, the streak is 16 at
        // launch 20; kLate = 5 launches late, launch 8's answer counts too before the every-launch
        // answers (launch 10 on) arrive at launch 16, and the streak is 16 at launch 29
        short_traffic(late, late == 0u ? 20u : 29u);
        variant8(late);
        host_forces(late);
        fill_never_small(late);
    }
    no_block();
    grids();
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::puts("choice checks OK");
    return 0;
}
