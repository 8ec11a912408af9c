// Host-side planning for the framesum entry points, free of HIP so that it compiles on its
// own: the chunks of a host-staged batch (fs_digest_batch_host), the byte-balanced blocks of
// fs_digest_batch_multi, the round-robin shard maps of fs_digest_batch_sharded and its
// de-interleave kernel, and the device result arrays of the RX host forms. The library includes it; tests/csrc/test_plan.cpp builds it alone
// under ASan + UBSan (sanitizers on the host code) and checks every invariant
// on random, out-of-order, overlapping and edge-case batches.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

namespace framesum {
namespace plan {

// ---------------------------------------------------------------------------------------
// Round-robin shards (eth/crc.go:12-17: CRC791 is per call, so frames are
// independent). Global frame i lives on shard i % N at local index i / N. Shards are padded
// to m = ceil(n / N) rows for the fixed-size RCCL gather; shard k's gathered slab holds its
// m 8-byte digests and then its m verdict bytes, 256-byte aligned.
constexpr uint64_t shard_count(uint64_t n, uint32_t nshards, uint32_t shard) {
    return shard < n ? (n - shard + nshards - 1) / nshards : 0;
}
constexpr uint64_t shard_rows(uint64_t n, uint32_t nshards) { return (n + nshards - 1) / nshards; }
constexpr uint64_t slab_bytes(uint64_t m) { return (9 * m + 255) / 256 * 256; }
// byte offsets, in the gathered buffer of nshards slabs, of global frame i's digest and verdict
constexpr uint64_t gathered_digest_at(uint64_t i, uint32_t nshards, uint64_t m) {
    return (i % nshards) * slab_bytes(m) + 8 * (i / nshards);
}
constexpr uint64_t gathered_status_at(uint64_t i, uint32_t nshards, uint64_t m) {
    return (i % nshards) * slab_bytes(m) + 8 * m + i / nshards;
}

// Chunks of a sharded batch (fs_digest_batch_sharded gathers chunk by chunk, so chunk c's
// transfer overlaps chunk c+1's kernels): chunk c = local rows [c*R, min((c+1)*R, m)) of every
// shard, R a multiple of 256 rows (the digest and verdict pieces stay 256-B aligned in the
// slab). Those rows hold exactly the global frames [c*R*N, min((c+1)*R*N, n)), so the
// de-interleave of a chunk needs only that chunk's pieces.
constexpr uint64_t chunk_rows(uint64_t m, uint32_t nchunks) {
    return nchunks == 0 ? m : ((m + nchunks - 1) / nchunks + 255) / 256 * 256;
}
constexpr uint32_t chunk_count(uint64_t m, uint64_t rows) { return rows == 0 ? 0 : (uint32_t)((m + rows - 1) / rows); }
// shard k's frames in local rows [lo, hi): [lo, min(hi, shard_count))
constexpr uint64_t shard_rows_in(uint64_t n, uint32_t nshards, uint32_t shard, uint64_t lo, uint64_t hi) {
    const uint64_t c = shard_count(n, nshards, shard);
    return (hi < c ? hi : c) > lo ? (hi < c ? hi : c) - lo : 0;
}

// The transfers of one chunk of fs_digest_batch_sharded: for every shard k >= 1 with rows in
// the chunk, its digest piece and its verdict piece go from its own slab (send offsets) to
// slab k of the first device's gather buffer (recv offsets); shard 0's kernel writes in place
// there. The first device then de-interleaves the global frames [g0, g1).
struct Piece {
    uint32_t shard;           // k >= 1
    uint64_t rows;            // rk = shard_rows_in(n, N, k, lo, hi) > 0
    uint64_t send_dig, send_st;  // byte offsets in shard k's slab: 8 lo, 8 m + lo
    uint64_t recv_dig, recv_st;  // byte offsets in the gather buffer: k sb + 8 lo, k sb + 8 m + lo
};
struct ChunkXfer {
    uint64_t lo, hi;   // local rows [lo, hi) of every shard
    uint64_t g0, g1;   // global frames [g0, g1) = [lo N, min(hi N, n))
    std::vector<Piece> pieces;
};
// The chunk plan of a sharded call: nchunks_max chunks at most, about target_rows rows each.
inline void chunk_plan(uint64_t n, uint32_t N, uint32_t nchunks_max, uint64_t target_rows, std::vector<ChunkXfer>& out) {
    out.clear();
    if (N == 0 || n == 0) return;
    const uint64_t m = shard_rows(n, N), sb = slab_bytes(m);
    const uint64_t want = target_rows ? (m + target_rows - 1) / target_rows : 1;
    const uint64_t R = chunk_rows(m, (uint32_t)(want < nchunks_max ? want : nchunks_max));
    const uint32_t C = chunk_count(m, R);
    for (uint32_t c = 0; c < C; ++c) {
        ChunkXfer x;
        x.lo = (uint64_t)c * R;
        x.hi = x.lo + R < m ? x.lo + R : m;
        x.g0 = x.lo * N;
        x.g1 = x.hi * N < n ? x.hi * N : n;
        for (uint32_t k = 1; k < N; ++k) {
            const uint64_t rk = shard_rows_in(n, N, k, x.lo, x.hi);
            if (rk == 0) continue;
            x.pieces.push_back(Piece{k, rk, 8 * x.lo, 8 * m + x.lo, k * sb + 8 * x.lo, k * sb + 8 * m + x.lo});
        }
        out.push_back(x);
    }
}

// ---------------------------------------------------------------------------------------
// Host-staged chunks.

// Index of the first frame that does not lie inside [0, frames_bytes) (overflow-safe), or n.
inline uint32_t first_frame_out_of_range(const uint64_t* offsets, const uint32_t* lengths, uint32_t n,
                                         uint64_t frames_bytes, uint32_t extra = 0, uint32_t* max_len = nullptr) {
    uint32_t mx = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t need = (uint64_t)lengths[i] + extra;
        if (offsets[i] > frames_bytes || need > frames_bytes - offsets[i]) return i;
        mx = lengths[i] > mx ? lengths[i] : mx;
    }
    if (max_len) *max_len = mx;  // (the batch's longest frame, when every frame is in range)
    return n;
}

// One pass over a host batch's descriptors (fs_digest_batch_host): whether every frame lies in
// [0, frames_bytes) (overflow-safe), the longest frame, and the byte span [lo, hi) of the whole
// batch. Branch-free in the loop (the compiler vectorizes it): the host-staged call of a batch of
// short frames walks 65,536 descriptors per call, and two passes of a branchy loop were a sizeable
// part of its host time. bad = the first out-of-range frame, or n. `extra`: bytes
// behind every frame that must lie in range too (the FCS a TX fill appends); hi does not count them.
struct Scan {
    uint32_t bad, max_len, min_len;
    uint64_t lo, hi;
};
// The reductions only (min offset, max offset, max end, max and min length): five independent
// min/max chains the compiler vectorizes. Every frame lies in range iff max offset <= frames_bytes and
// max end + extra <= frames_bytes, as long as no end wraps (frames_bytes < 2^64 - 2^33: a larger
// buffer falls back to the per-frame test).
struct ScanCore {
    uint64_t lo, hi_off, hi_end;
    uint32_t max_len, min_len;
};
inline ScanCore scan_core(const uint64_t* offsets, const uint32_t* lengths, uint32_t n) {
    uint64_t lo = UINT64_MAX, ho = 0, he = 0;
    uint32_t mx = 0, mn = UINT32_MAX;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t o = offsets[i];
        const uint32_t l = lengths[i];
        lo = o < lo ? o : lo;
        ho = o > ho ? o : ho;
        he = o + l > he ? o + l : he;
        mx = l > mx ? l : mx;
        mn = l < mn ? l : mn;
    }
    ScanCore c;
    c.lo = lo;
    c.hi_off = ho;
    c.hi_end = he;
    c.max_len = mx;
    c.min_len = n ? mn : 0;
    return c;
}
inline Scan scan_from(const ScanCore& c, const uint64_t* offsets, const uint32_t* lengths, uint32_t n,
                      uint64_t frames_bytes, uint32_t extra = 0) {
    Scan s;
    const bool exact = frames_bytes < UINT64_MAX - (uint64_t(1) << 33);
    const bool in_range = exact && c.hi_off <= frames_bytes && c.hi_end <= frames_bytes &&
                          frames_bytes - c.hi_end >= extra;
    s.bad = (n == 0 || in_range) ? n : first_frame_out_of_range(offsets, lengths, n, frames_bytes, extra);
    s.max_len = c.max_len;
    s.min_len = c.min_len;
    s.lo = n ? c.lo : 0;
    s.hi = c.hi_end;
    return s;
}
inline Scan scan_batch(const uint64_t* offsets, const uint32_t* lengths, uint32_t n, uint64_t frames_bytes,
                       uint32_t extra = 0) {
    return scan_from(scan_core(offsets, lengths, n), offsets, lengths, n, frames_bytes, extra);
}

// The sum of a batch's lengths: the bytes fs_digest_batch_multi balances over its contexts, and the
// most payload an RX coalesce of the batch can deliver. (Apart from scan_core, whose reductions are
// the timed loop of fs_digest_batch_host.)
inline uint64_t total_length(const uint32_t* lengths, uint32_t n) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) total += lengths[i];
    return total;
}

struct Chunk {
    uint32_t c0, c1;          // frames [c0, c1)
    uint64_t cpy_lo, cpy_hi;  // host bytes [cpy_lo, cpy_hi) staged for them
};

// The bytes a staged chunk copies for frames spanning [lo, hi): a 16-B aligned start with a
// 16-B prefix (frames under 4 bytes are read from up to 12 bytes before their start), and the
// end rounded up to the dword the engine may read, capped at the buffer.
inline void copy_span(uint64_t lo, uint64_t hi, uint64_t frames_bytes, uint64_t& cpy_lo, uint64_t& cpy_hi) {
    cpy_lo = (lo >= 16 ? lo - 16 : 0) & ~uint64_t(15);
    cpy_hi = (hi + 3) & ~uint64_t(3);
    if (cpy_hi > frames_bytes) cpy_hi = frames_bytes;
    if (cpy_hi < cpy_lo) cpy_hi = cpy_lo;
}

// Cut frames [0, n) into chunks of at most chunk_frames frames whose byte span stays within
// chunk_bytes (a single frame may exceed it). When a chunk would hold fewer than 64 frames
// because the next frame lies far away (frames not stored in index order), the chunk takes
// the rest of the batch instead of a launch per handful of frames. Every frame must already
// lie inside the buffer (first_frame_out_of_range).
inline void host_chunks(const uint64_t* offsets, const uint32_t* lengths, uint32_t n, uint64_t frames_bytes,
                        uint64_t chunk_bytes, uint32_t chunk_frames, std::vector<Chunk>& out) {
    out.clear();
    uint32_t c0 = 0;
    while (c0 < n) {
        uint64_t lo = offsets[c0], hi = offsets[c0] + lengths[c0];
        uint32_t c1 = c0 + 1;
        while (c1 < n && c1 - c0 < chunk_frames) {
            const uint64_t o = offsets[c1], e = o + lengths[c1];
            const uint64_t nlo = o < lo ? o : lo, nhi = e > hi ? e : hi;
            if (nhi - nlo > chunk_bytes) break;
            lo = nlo;
            hi = nhi;
            ++c1;
        }
        if (c1 < n && c1 - c0 < 64 && hi - lo < chunk_bytes / 4) {
            for (; c1 < n; ++c1) {
                const uint64_t o = offsets[c1], e = o + lengths[c1];
                lo = o < lo ? o : lo;
                hi = e > hi ? e : hi;
            }
        }
        Chunk c{c0, c1, 0, 0};
        copy_span(lo, hi, frames_bytes, c.cpy_lo, c.cpy_hi);
        out.push_back(c);
        c0 = c1;
    }
}

// ---------------------------------------------------------------------------------------
// The device result arrays of the first seven RX host forms (fs_coalesce_batch_host,
// fs_coalesce_flows_batch_host, fs_deliver_flows_batch_host, fs_recv_flows_batch_host and, with the
// arrays of their own in the second table below, fs_accept_flows_batch_host,
// fs_close_flows_batch_host and fs_connect_flows_batch_host), described
// once: which arrays a call kind has, what each is sized by, where each lies in the context's one
// buffer, and how much of each comes back given the totals the device reported. The host forms carve
// the buffer and copy back by walking this description (framesum_api_rx.cpp).
namespace rx {

// A kind has the arrays of the kinds before it and its own.
enum Kind : uint32_t { kPlain, kFlows, kDeliver, kRecv, kAccept, kClose, kConnect, kUdp, kArp };
enum Array : uint32_t { kTotals, kRuns, kFlowRecs, kOrder, kRunOf, kDelivered, kSocksOut, kSndOut, kCode, kArrays };
// What counts an array's entries: one record, the batch's frames, the call's sockets, or (for what
// comes back only) one of the totals.
enum Count : uint32_t { kOne, kPerFrame, kPerSock, kNRuns, kNFlows, kNAccepted };
struct Totals {
    uint64_t n_runs, n_flows, n_accepted;  // (the plain call reports runs only)
};
struct ArrayDesc {
    Kind from;             // the first kind that has the array
    uint32_t elem, align;  // bytes per entry (kTotals: see totals_bytes), and the alignment its type needs
    Count room, back;      // entries it has room for, entries that come back
};
constexpr ArrayDesc kArrayDesc[kArrays] = {
    {kPlain, 0, 8, kOne, kOne},               // fs_rx_totals / fs_rx_flow_totals
    {kPlain, 24, 8, kPerFrame, kNRuns},       // fs_rx_run
    {kFlows, 32, 8, kPerFrame, kNFlows},      // fs_rx_flow
    {kFlows, 4, 4, kPerFrame, kNAccepted},    // order
    {kPlain, 4, 4, kPerFrame, kPerFrame},     // run_of
    {kDeliver, 1, 1, kPerFrame, kPerFrame},   // delivered
    {kDeliver, 32, 8, kPerSock, kPerSock},    // fs_rx_sock_out
    {kRecv, 32, 8, kPerSock, kPerSock},       // fs_rx_snd_out
    {kRecv, 1, 1, kPerFrame, kPerFrame},      // code
};
constexpr uint64_t totals_bytes(Kind kind) { return kind == kPlain ? 16 : 24; }
constexpr uint64_t elem_bytes(Kind kind, Array a) { return a == kTotals ? totals_bytes(kind) : kArrayDesc[a].elem; }
constexpr uint64_t count_of(Count c, uint64_t n, uint64_t n_socks, const Totals& t) {
    return c == kOne ? 1 : c == kPerFrame ? n : c == kPerSock ? n_socks : c == kNRuns ? t.n_runs : c == kNFlows ? t.n_flows : t.n_accepted;
}

// Whether the totals the device reported can be a batch of n frames' (every count that sizes a copy
// back is then within its array's room).
constexpr bool consistent(Kind kind, uint64_t n, const Totals& t) {
    return kind == kPlain ? t.n_runs <= n : t.n_accepted <= n && t.n_runs <= t.n_accepted && t.n_flows <= t.n_runs;
}

// Where the arrays of a call of `kind` over n frames and n_socks sockets lie: byte offsets from an
// 8-byte aligned base (kAbsent: the kind has no such array), each aligned for its type, in the order of
// Array; `room` bytes each, `bytes` in all.
constexpr uint64_t kAbsent = ~uint64_t(0);
struct Layout {
    uint64_t at[kArrays], room[kArrays], bytes;
    bool has(Array a) const { return at[a] != kAbsent; }
};
inline Layout layout(Kind kind, uint64_t n, uint64_t n_socks) {
    Layout L;
    uint64_t at = 0;
    for (uint32_t a = 0; a < kArrays; ++a) {
        const ArrayDesc& d = kArrayDesc[a];
        L.at[a] = kAbsent;
        L.room[a] = 0;
        if (kind < d.from) continue;
        at = (at + d.align - 1) / d.align * d.align;
        L.at[a] = at;
        L.room[a] = elem_bytes(kind, (Array)a) * count_of(d.room, n, n_socks, Totals{0, 0, 0});
        at += L.room[a];
    }
    L.bytes = at;
    return L;
}
// The bytes of array `a` that come back to the caller, given consistent totals `t`.
constexpr uint64_t bytes_back(Kind kind, Array a, uint64_t n, uint64_t n_socks, const Totals& t) {
    return kind < kArrayDesc[a].from ? 0 : elem_bytes(kind, a) * count_of(kArrayDesc[a].back, n, n_socks, t);
}

// The own arrays of the fifth, the sixth and the seventh kind (fs_accept_flows_batch_host,
// fs_close_flows_batch_host, fs_connect_flows_batch_host: each has every array above, those of the kinds
// before it, and its own), described the same way in one table: which kind brings an array, what counts
// its entries, the alignment the kernels' stores want, and whether the caller's bytes go to the device
// first (the call writes only some entries of those -- the filled slots', the openers' with a reply --
// and every array comes back whole). They lie behind the arrays above in the same buffer, in this order.
enum ExtraArray : uint32_t {
    kConns, kListenersOut, kAcceptOf, kSynacks, kSynackOut, kSynackStatus,  // kAccept
    kClosersOut, kSocksClose, kCtlCode,                                      // kClose
    kOpenersOut, kReplies, kReplyOut, kReplyStatus,                          // kConnect
    kExtraArrays,
};
enum ExtraCount : uint32_t { kPerSlot, kPerListener, kPerCloser, kPerSocket, kPerOpener, kPerBatchFrame, kExtraCounts };
struct ExtraArrayDesc {
    Kind from;             // the kind that brings the array
    uint32_t elem, align;  // bytes per entry, and the alignment
    ExtraCount count;
    bool goes_in;
};
constexpr ExtraArrayDesc kExtraArrayDesc[kExtraArrays] = {
    {kAccept, 48, 4, kPerSlot, false},         // fs_accept_conn
    {kAccept, 16, 4, kPerListener, false},     // fs_listener_out
    {kAccept, 4, 4, kPerBatchFrame, false},    // accept_of
    {kAccept, 64, 1, kPerSlot, true},          // synacks (FS_ACCEPT_STRIDE)
    {kAccept, 8, 8, kPerSlot, true},           // synack_out
    {kAccept, 1, 1, kPerSlot, true},           // synack_status
    {kClose, 32, 4, kPerCloser, false},        // fs_cl_out, per closer
    {kClose, 32, 4, kPerSocket, false},        // fs_cl_out, per listed socket
    {kClose, 1, 1, kPerBatchFrame, false},     // ctl_code
    {kConnect, 48, 4, kPerOpener, false},      // fs_cn_out
    {kConnect, 64, 1, kPerOpener, true},       // replies (FS_ACCEPT_STRIDE)
    {kConnect, 8, 8, kPerOpener, true},        // reply_out
    {kConnect, 1, 1, kPerOpener, true},        // reply_status
};
struct ExtraCounts {
    uint64_t of[kExtraCounts];  // by ExtraCount
};
struct ExtraLayout {
    uint64_t at[kExtraArrays], room[kExtraArrays], bytes;  // `bytes`: `base` and the rows laid out
    bool has(ExtraArray a) const { return at[a] != kAbsent; }
};
// The rows whose kind lies in [first, last] (none when last < first), from `base` on:
// layout(kind, n, n_socks).bytes with first = kAccept and last = the call's kind; 0 with both kConnect for
// a connect call without a batch, which has these arrays alone.
inline ExtraLayout extra_layout(Kind first, Kind last, uint64_t base, const ExtraCounts& counts) {
    ExtraLayout L;
    uint64_t at = base;
    for (uint32_t a = 0; a < kExtraArrays; ++a) {
        const ExtraArrayDesc& d = kExtraArrayDesc[a];
        L.at[a] = kAbsent;
        L.room[a] = 0;
        if (d.from < first || d.from > last) continue;
        at = (at + d.align - 1) / d.align * d.align;
        L.at[a] = at;
        L.room[a] = d.elem * counts.of[d.count];
        at += L.room[a];
    }
    L.bytes = at;
    return L;
}

// The own arrays of the eighth kind (fs_udp_flows_batch_host), in a description of their own: they lie
// behind extra_layout(kAccept, kConnect, ...)'s rows in the same buffer, in this order, every entry is
// written by the call and every array comes back whole. (`cells` is no such array: the span of it that
// the listed queues cover has a buffer of its own, as the rings have.)
enum UdpArray : uint32_t { kPortsOut, kPortOf, kCellOf, kUdpArrays };
enum UdpCount : uint32_t { kPerPort, kPerUdpFrame };
struct UdpArrayDesc {
    uint32_t elem, align;  // bytes per entry, and the alignment the kernels' stores want
    UdpCount count;
};
constexpr UdpArrayDesc kUdpArrayDesc[kUdpArrays] = {
    {32, 8, kPerPort},      // fs_udp_port_out (its `bytes` is a 64-bit sum)
    {4, 4, kPerUdpFrame},   // port_of
    {4, 4, kPerUdpFrame},   // cell_of
};
struct UdpLayout {
    uint64_t at[kUdpArrays], room[kUdpArrays], bytes;  // `bytes`: `base` and the rows laid out
};
inline UdpLayout udp_layout(uint64_t base, uint64_t n, uint64_t n_ports) {
    UdpLayout L;
    uint64_t at = base;
    for (uint32_t a = 0; a < kUdpArrays; ++a) {
        const UdpArrayDesc& d = kUdpArrayDesc[a];
        at = (at + d.align - 1) / d.align * d.align;
        L.at[a] = at;
        L.room[a] = d.elem * (d.count == kPerPort ? n_ports : n);
        at += L.room[a];
    }
    L.bytes = at;
    return L;
}

// The own arrays of the ninth kind (fs_arp_flows_batch_host), described the same way: they lie behind
// udp_layout's rows in the same buffer, in this order. Of the frames, their digests and their verdicts the
// call writes only the slots that take a frame, so the caller's bytes go to the device first; every array
// comes back whole. A frame slot is a reply slot or a query's request slot.
enum ArpArray : uint32_t { kHostsOut, kQueriesOut, kArpFrames, kArpOut, kArpStatus, kArpCode, kArpOf, kArpArrays };
enum ArpCount : uint32_t { kPerHost, kPerQuery, kPerFrameSlot, kPerArpFrame, kArpCounts };
struct ArpArrayDesc {
    uint32_t elem, align;  // bytes per entry, and the alignment the kernels' stores want
    ArpCount count;
    bool goes_in;
};
constexpr ArpArrayDesc kArpArrayDesc[kArpArrays] = {
    {16, 4, kPerHost, false},       // fs_arp_host_out
    {16, 4, kPerQuery, false},      // fs_arp_query_out
    {64, 1, kPerFrameSlot, true},   // arp_frames (FS_ACCEPT_STRIDE)
    {8, 8, kPerFrameSlot, true},    // arp_out
    {1, 1, kPerFrameSlot, true},    // arp_status
    {1, 1, kPerArpFrame, false},    // arp_code
    {4, 4, kPerArpFrame, false},    // arp_of
};
struct ArpCounts {
    uint64_t of[kArpCounts];  // by ArpCount
};
struct ArpLayout {
    uint64_t at[kArpArrays], room[kArpArrays], bytes;  // `bytes`: `base` and the rows laid out
};
inline ArpLayout arp_layout(uint64_t base, const ArpCounts& counts) {
    ArpLayout L;
    uint64_t at = base;
    for (uint32_t a = 0; a < kArpArrays; ++a) {
        const ArpArrayDesc& d = kArpArrayDesc[a];
        at = (at + d.align - 1) / d.align * d.align;
        L.at[a] = at;
        L.room[a] = d.elem * counts.of[d.count];
        at += L.room[a];
    }
    L.bytes = at;
    return L;
}

}  // namespace rx

// ---------------------------------------------------------------------------------------
// fs_digest_batch_multi blocks: nctx blocks of about equal byte counts. The blocks are
// contiguous runs of the frames in buffer order, so that each context copies only its own
// bytes: `order` is empty when the offsets are already non-decreasing (block k = frames
// [cut[k], cut[k+1])), otherwise it lists the frame indices sorted by offset (stable) and
// block k = order[cut[k] .. cut[k+1]).
struct MultiPlan {
    std::vector<uint32_t> order;
    std::vector<uint32_t> cut;  // nctx + 1 positions, cut[0] = 0, cut[nctx] = n
    uint32_t frame(uint32_t pos) const { return order.empty() ? pos : order[pos]; }
};

inline void multi_blocks(const uint64_t* offsets, const uint32_t* lengths, uint32_t n, int nctx, MultiPlan& p) {
    p.order.clear();
    p.cut.assign((size_t)nctx + 1, n);
    p.cut[0] = 0;
    bool sorted = true;
    for (uint32_t i = 1; i < n && sorted; ++i) sorted = offsets[i] >= offsets[i - 1];
    if (!sorted) {
        p.order.resize(n);
        std::iota(p.order.begin(), p.order.end(), 0u);
        std::stable_sort(p.order.begin(), p.order.end(),
                         [offsets](uint32_t a, uint32_t b) { return offsets[a] < offsets[b]; });
    }
    const uint64_t total = total_length(lengths, n);
    // block k starts at the first position whose running byte count reaches k/nctx of the total
    uint64_t run = 0;
    int k = 1;
    for (uint32_t pos = 0; pos < n && k < nctx; ++pos) {
        while (k < nctx && (unsigned __int128)run * (unsigned)nctx >= (unsigned __int128)total * (unsigned)k)
            p.cut[k++] = pos;
        run += lengths[p.frame(pos)];
    }
}

}  // namespace plan
}  // namespace framesum
