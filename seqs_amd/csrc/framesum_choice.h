// Which kernel a launch runs, what it is asked to report, and how large its grid is: the policy
// of launch_digest (framesum_kernel.hip), free of HIP so that it compiles on its own. The library
// includes it; tests/csrc/test_choice.cpp builds it alone under ASan + UBSan and drives it with a
// model of what the kernels post. The choice never changes a result, only the speed.
#pragma once
#include <stdint.h>

namespace framesum {

// The kernel variants (fs_ctx_set_kernel, fs_ctx_last_kernel; the values are ABI): the automatic
// choice, the mixed-length kernel (digest_kernel_ab, pieces), the segment kernel (digest_kernel_g:
// another mixed-length decomposition, slower on C3), the one-pass kernel
// (digest_kernel_a), and the small-frame kernel (digest_kernel_s) preferred.
constexpr int kKernelAuto = 0, kKernelMixed = 2, kKernelSegment = 3, kKernelOnePass = 4, kKernelSmall = 8;
// choose()'s force values for the host-staged path, which knows every length: the small-frame
// kernel unconditionally (every frame <= kSmallMaxLen), or the automatic choice among the 4-lane
// kernels only (a frame is longer: however short the context's recent traffic, the small-frame
// kernel would stream that frame with one lane)
constexpr int kForceSmallExact = 16;
constexpr int kForceNoSmall = 17;
// ... and for a host batch whose lengths all lie within kUniformSpan bytes, the one-pass kernel from
// the context's first call: the initial mixed-kernel window (kInitialMixedLaunches) is for
// device-resident batches, whose lengths the host never sees. Mode B cannot pay inside that span
// (tile_geometry: no frame has a full piece, or the full-piece passes cost more rows than they
// save). Not because the tile's frames differ by under 4 rows: with start alignment they can (65 B
// at alignment 0 is 2 rows, 319 B at alignment 3 is 6).
constexpr int kForceUniformHost = 18;
constexpr uint32_t kUniformSpan = 256;

// The context's host-mapped report block (64 B) holds three words, all written by the device only:
// kReportLatest, the latest launch id that met mixed-length tiles, with kReportMixedGiant set when
// the posting tile held a frame longer than the mixed-length kernel's pieces cover (kMaxFullPasses
// passes of 16 pieces) beside short ones (the automatic choice then runs the segment kernel, which
// splits any frame into equal chunks); and for the short-frame choice (the
// small-frame kernel for traffic of frames <= kSmallMaxLen bytes) kReportLong, the
// latest launch id that met a frame longer than kSmallMaxLen, and kReportRan, the latest launch id
// that ran a 4-lane kernel (posted by the grid's first wave, with kReportRanLong set when its own
// tile held such a frame). What the host remembers about them is in ChoiceState.
constexpr int kReportLatest = 0, kReportLong = 5, kReportRan = 6;
constexpr uint32_t kReportRanLong = 1u << 16;
constexpr uint32_t kReportMixedGiant = 1u << 16;
constexpr uint32_t kSmallMaxLen = 128;
// the kernels' `report` argument: the report block's device address in bits 6..46 (host-mapped
// memory sits below 2^47; the block is 64-B aligned), the watch flag kReportWatch in bit 47 (the host
// is counting short launches, so every wave reports its long tiles, not only the grid's first), the
// launch id in bits 48..63, and in bits 0..1 what this launch is asked to post: kAskRan (the grid's
// first tile posts kReportRan) and kAskMixed (the mixed-length kernel posts its mixed tiles; the
// one-pass kernel always does). Each post costs the launch ~0.28 us (C2), so steady traffic is
// sampled: "ran" on every kRanSample-th launch under variant 0 (every launch while the host counts
// short launches, and every launch under variant 8), "mixed" from the mixed-length kernel on every
// kMixedSample-th launch (and until the first report).
constexpr uint64_t kReportWatch = 1ull << 47;
constexpr uint64_t kReportAddrMask = (kReportWatch - 1u) & ~63ull;
constexpr uint64_t kAskRan = 1u, kAskMixed = 2u;
constexpr uint32_t kRanSample = 4, kMixedSample = 32;
// a context's first launches run the mixed-length kernel (see choose)
constexpr uint32_t kInitialMixedLaunches = 16;
// the mixed kernel stays chosen for this many launches after the host saw the latest mixed report
constexpr uint32_t kStickyLaunches = 4096;
// launches seen to run without a long frame before variant 0 moves to the small-frame kernel, and
// before a variant-8 context that met long frames goes back to it
constexpr uint32_t kShortLaunchesAuto = 16, kShortLaunchesSmall = 2;

// What a context remembers between launches (host memory only; a context is used from one thread
// at a time, include/framesum.h).
struct ChoiceState {
    // the context's launch sequence (the counter is the context's: another context's launches
    // never shift this one's window)
    uint32_t next_seq = 1;
    uint32_t initial = kInitialMixedLaunches;  // launches left in the initial mixed-kernel window
    uint32_t chosen = 0;                       // the variant of the latest launch (fs_ctx_last_kernel)
    // kReportLatest as the host last saw it change, and the launch sequence at that moment (the
    // sticky window's clock)
    uint32_t seen = 0, seen_seq = 0;
    // kReportLong and kReportRan's id as the host last saw them, the number of launches seen to run
    // since the latest long report, and whether any long report has arrived
    uint32_t long_seen = 0, ran_seen = 0, short_streak = 0, long_ever = 0;
};

// The report block's three words as the caller read them just now.
struct Reports {
    uint32_t latest, lng, ran;
};

struct Choice {
    uint32_t variant;  // kKernelMixed, kKernelSegment, kKernelOnePass or kKernelSmall
    uint32_t id;       // the launch's 16-bit id (never 0), for bits 48..63 of `report`
    uint64_t bits;     // kAskRan | kAskMixed | kReportWatch, to OR into `report`
};

// One launch's choice. `r`: null when the context has no usable report block. `force`: a kKernel*
// value (fs_ctx_set_kernel) or one of the host-staged path's kForce* values. `is_fill`: a TX fill.
inline Choice choose(ChoiceState& s, const Reports* r, int force, bool is_fill) {
    // The report of the launches before (the latest launch id that met a mixed-length tile):
    // launches are enqueued ahead of the GPU, so a report arrives several launches late; the
    // mixed kernel stays chosen for kStickyLaunches launches after the latest report (it keeps
    // reporting while the traffic is mixed, on every kMixedSample-th launch). A heuristic only:
    // never a result.
    // Launch ids are 16-bit (they travel in the report pointer's top bits; 0 = never reported).
    // The window is timed on the host instead: `next_seq` is the context's 32-bit launch sequence,
    // and the host notes the sequence at which it first saw the report word change (seen /
    // seen_seq), so a report stays recent for kStickyLaunches of this context's launches and never
    // aliases an old one after the 16-bit ids wrap.
    const uint32_t seq = s.next_seq++;
    uint32_t id = seq & 0xFFFFu;
    if (id == 0u) id = 0x8000u;  // (0 means "never reported"; any non-zero tag will do)
    uint64_t bits = 0u;
    bool mixed = false, giant = false;
    if (r) {
        const uint32_t latest = r->latest;
        giant = (latest & kReportMixedGiant) != 0u;
        if (latest != s.seen) {
            s.seen = latest;
            s.seen_seq = seq;
        }
        mixed = latest != 0u && seq - s.seen_seq <= kStickyLaunches;
        // the mixed-length kernel's own posts only refresh the window: sampled (kMixedSample)
        if (latest == 0u || seq % kMixedSample == 0u) bits |= kAskMixed;
        // A context's first launches run the mixed-length kernel: it reports its own mode-B tiles,
        // so mixed traffic keeps it from the first batch on (the one-pass kernel's report would
        // arrive launches late, after slow first batches), and uniform traffic moves to the
        // one-pass kernel once the window ends.
        if (s.initial != 0u) {
            --s.initial;
            mixed = true;
        }
    }
    if (force == kKernelMixed || force == kKernelSegment || force == kKernelOnePass) mixed = force != kKernelOnePass;
    if (force == kForceUniformHost) mixed = false;
    // the automatic choice runs the segment kernel while the latest mixed report saw a giant tile
    const bool segments = force == kKernelSegment ||
                          (mixed && giant && (force == kKernelAuto || force == kForceNoSmall || force == kKernelSmall));
    // The small-frame kernel (RX digest and FCS verify; a TX fill keeps the 4-lane choice above).
    // The kernels report launches that met a frame longer than kSmallMaxLen (kReportLong), and the
    // 4-lane kernels, when asked (kAskRan), that a launch ran (kReportRan, with the grid's first
    // tile's own long flag in the same word, kReportRanLong); the host counts the launches it sees
    // run since the latest long report. Variant 0
    // moves to the small-frame kernel after kShortLaunchesAuto of them; variant 8 runs it until a
    // long report arrives, then the 4-lane choice until kShortLaunchesSmall launches ran short
    // again. The reports come launches late, so a long frame can still meet the small-frame kernel:
    // it stays correct there, only slower (one lane streams it). kForceSmallExact: the host-staged
    // path, which has seen every length.
    bool small = false;
    // kForceNoSmall (a host-staged batch with a long frame) reports as the automatic choice does, so
    // its long frames end a short streak; it only never picks the small-frame kernel itself
    const bool autov = force == kKernelAuto || force == kForceNoSmall || force == kForceUniformHost;
    if (r) {
        const uint32_t lng = r->lng, rw = r->ran, ran = rw & 0xFFFFu;
        const bool ran_new = ran != s.ran_seen;
        if (lng != s.long_seen || (ran_new && (rw & kReportRanLong) != 0u)) {
            s.long_seen = lng;
            s.short_streak = 0u;
            s.long_ever = 1u;
        } else if (ran_new && ran != lng && s.short_streak < (1u << 30)) {
            ++s.short_streak;
        }
        s.ran_seen = ran;
        const uint32_t streak = s.short_streak;
        if (force == kKernelAuto) small = streak >= kShortLaunchesAuto;
        if (force == kKernelSmall) small = s.long_ever == 0u || streak >= kShortLaunchesSmall;
        // every workgroup reports its long frames while the host counts short launches
        if ((autov || force == kKernelSmall) && streak > 0u) bits |= kReportWatch;
        // "ran": variant 0 samples it on long traffic and asks every launch while it counts short
        // ones; variant 8 (short traffic expected: back to the small-frame kernel after 2 short
        // launches) asks every launch
        if (force == kKernelSmall || (autov && (streak > 0u || seq % kRanSample == 0u))) bits |= kAskRan;
    } else if (force == kKernelSmall) {
        small = true;  // no report block: the caller's choice as it stands
    }
    if (force == kForceSmallExact) small = true;
    if (force == kForceNoSmall || force == kForceUniformHost || is_fill) small = false;
    if (small) mixed = false;
    s.chosen = (uint32_t)(small ? kKernelSmall : mixed ? (segments ? kKernelSegment : kKernelMixed) : kKernelOnePass);
    return Choice{s.chosen, id, bits};
}

// The host-staged digest sees the batch's lengths on the host: with the automatic choice (0) or the
// short-frame preference (8), a batch whose frames are all this short runs the small-frame kernel
// (one lane per frame; its header slot holds frames up to ~130 B), and any other batch the
// automatic choice between the 4-lane kernels. (A device-resident batch's lengths are in device
// memory: there choose() goes by the kernels' reports.)
inline int host_force(int force_kernel, uint32_t max_len, uint32_t min_len) {
    if (force_kernel != kKernelAuto && force_kernel != kKernelSmall) return force_kernel;
    if (max_len <= kSmallMaxLen) return kForceSmallExact;
    // a longer frame: the 4-lane choice, never the small-frame kernel, even after a
    // streak of short device-resident launches; lengths within kUniformSpan: the one-pass kernel from
    // the first call (a short-lived RecvEthBatch context)
    return max_len - min_len < kUniformSpan ? kForceUniformHost : kForceNoSmall;
}

// The 4-lane kernels' grid: workgroups of `waves_per_block` waves, one tile of `fpt` frames per wave
// at a time, at most `max_blocks` workgroups. Fewer frames per tile (8, then 4) while `max_fpt` (16)
// would leave waves without a tile: a small batch still spreads over every CU. The groups past a
// tile's frames stay empty in the one-pass kernel; the mixed-length kernel gives them pieces of
// the tile's long frames.
struct Grid {
    uint32_t fpt, blocks;
};
inline Grid grid_4lane(uint32_t n, uint32_t max_blocks, uint32_t waves_per_block, uint32_t max_fpt) {
    uint32_t fpt = max_fpt;
    const uint32_t waves = max_blocks * waves_per_block;
    while (fpt > 4u && (n + fpt - 1) / fpt < waves) fpt >>= 1;
    const uint32_t tiles = (n + fpt - 1) / fpt;
    const uint32_t blocks = (tiles + waves_per_block - 1) / waves_per_block;
    return Grid{fpt, blocks > max_blocks ? max_blocks : blocks};
}
// The small-frame kernel's grid: 64 frames (one per lane) per wave, `waves_per_block` waves per
// workgroup, at most two workgroups per CU.
inline uint32_t grid_small(uint32_t n, uint32_t max_blocks, uint32_t waves_per_block) {
    const uint32_t tiles = (n + 63u) / 64u;
    const uint32_t blocks = (tiles + waves_per_block - 1u) / waves_per_block;
    return blocks > 2u * max_blocks ? 2u * max_blocks : blocks;
}

}  // namespace framesum
