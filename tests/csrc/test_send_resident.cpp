// The arithmetic of the resident ring send (seqs_amd/csrc/framesum_send_resident.h, and through it the
// rule header seqs_amd/csrc/framesum_send.h as the device path uses it) on the CPU, built alone under
// ASan + UBSan by tests/test_send_resident_host.py. For batches with idle, window-bound, FIN, ACK and
// long sockets, at ample capacity and at every frames_cap and frames_bytes that cuts them, with invalid
// sockets of every reason and with RX records handed off: the socks_out records are send::layout's for
// the list of built sockets, the block the plan writes is send::stage's byte for byte, and the totals,
// the head and the write-back are what the header states. The plan runs twice: in index order
// (plan_sequential) and cut into chunks the way the three plan kernels compute it (chunk sums, their
// exclusive prefix, the search of the cut chunk, the in-chunk prefixes), on exactly sized heap arrays.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../seqs_amd/csrc/framesum_send_resident.h"

namespace sd = framesum::send;
namespace seg = framesum::segment;
namespace res = framesum::resident;

static int g_failed = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                  \
        }                                                                \
    } while (0)

static uint32_t g_rng = 12345;
static uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % n;
}

static fs_tx_sock sock(uint32_t mss, uint64_t ring_off, uint32_t ring_size, uint32_t rpos, uint32_t buffered, uint32_t flags = 0) {
    fs_tx_sock s;
    std::memset(&s, 0, sizeof s);
    for (int i = 0; i < 54; ++i) s.hdr[i] = (uint8_t)rnd(256);
    s.hdr[12] = 0x08, s.hdr[13] = 0x00, s.hdr[14] = 0x45, s.hdr[23] = 6, s.hdr[46] = 0x50;
    s.mss = (uint16_t)mss;
    s.ring_off = ring_off;
    s.ring_size = ring_size;
    s.ring_rpos = rpos;
    s.ring_buffered = buffered;
    s.snd_una = rnd(1u << 30) * 4u + 3u;
    s.snd_nxt = s.snd_una + rnd(500);
    s.snd_wnd = 1u << 20;
    s.rcv_nxt = rnd(1u << 30), s.rcv_wnd = rnd(100000);
    s.flags = flags;
    return s;
}

// n sockets of mixed state: a third idle, some window-bound, some with FIN / ACK / PSH, one long
static std::vector<fs_tx_sock> mixed(uint32_t n, uint64_t& rings_bytes) {
    std::vector<fs_tx_sock> v;
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t size = 64 + rnd(4000), mss = 1 + rnd(300);
        uint32_t buffered = i % 3 == 0 ? 0 : 1 + rnd(size);
        static const uint32_t kFlags[6] = {0, FS_TX_ACK, FS_TX_FIN, FS_TX_PSH, FS_TX_FIN | FS_TX_PSH, 0};
        const uint32_t flags = kFlags[rnd(6)];
        fs_tx_sock s = sock(mss, at, size, rnd(size), buffered, i % 3 == 0 && i % 2 ? 0 : flags);
        if (i % 7 == 3) s.snd_wnd = s.snd_nxt - s.snd_una + rnd(50);  // little or no room
        if (i % 11 == 5) s.max_frames = 1 + rnd(3);
        if (i == n / 2) s.mss = 1, s.ring_buffered = size, s.max_frames = 0;  // many frames: several ID powers
        v.push_back(s);
        at += size;
    }
    rings_bytes = at;
    return v;
}

struct Result {
    std::vector<fs_tx_sock> table;  // after the call
    std::vector<fs_tx_sock_out> outs;
    std::vector<uint8_t> block;
    res::Head head;
    fs_tx_totals totals;
};

static res::Call call_of(std::vector<fs_tx_sock>& table, std::vector<fs_tx_sock_out>& outs, fs_tx_totals& totals,
                         uint64_t rings_bytes, uint32_t cap, uint64_t frames_bytes, uint32_t flags, uint32_t align) {
    res::Call c;
    std::memset(&c, 0, sizeof c);
    c.socks = table.data();
    c.socks_out = outs.data();
    c.totals = &totals;
    c.rings_bytes = rings_bytes;
    c.frames_bytes = frames_bytes;
    c.n_socks = (uint32_t)table.size();
    c.frames_cap = cap;
    c.flags = flags;
    c.align = align;
    c.grid_waves = 24;
    return c;
}

// The whole plan in index order: `head`, `totals`, the block, socks_out and the write-back.
static void plan_sequential(const res::Call& c, res::Head& head, uint8_t* block) {
    res::Sums all, built;
    uint32_t cut = c.n_socks;
    for (uint32_t i = 0; i < c.n_socks; ++i) {
        const res::SockPlan q = res::plan_sock(c, i);
        all = res::add(all, res::sums_of(q));
        if (cut == c.n_socks && q.p.frames && !res::fits(c, all)) cut = i;
        if (cut == c.n_socks) built = all;
    }
    head = res::head_of(c, cut, built);
    *c.totals = res::totals_of(built, all);
    res::Sums excl;
    for (uint32_t i = 0; i < c.n_socks; ++i) {
        const res::SockPlan q = res::plan_sock(c, i);
        res::write_sock(c, head, block, i, q, excl);
        excl = res::add(excl, res::sums_of(q));
    }
    res::write_prefix_end(head, block);
}

// The plan as the three kernels compute it: chunk sums; their exclusive prefix and the cut; the writes.
static void plan_chunked(const res::Call& c, res::Head& head, uint8_t* block) {
    const uint32_t chunks = (c.n_socks + res::kChunk - 1) / res::kChunk;
    std::vector<res::Sums> sums(chunks), base(chunks);
    for (uint32_t k = 0; k < chunks; ++k)
        for (uint32_t i = k * res::kChunk; i < c.n_socks && i < (k + 1) * res::kChunk; ++i)
            sums[k] = res::add(sums[k], res::sums_of(res::plan_sock(c, i)));
    res::Sums all;
    uint32_t cut_chunk = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < chunks; ++k) {
        base[k] = all;
        all = res::add(all, sums[k]);
        if (cut_chunk == 0xFFFFFFFFu && !res::fits(c, all)) cut_chunk = k;
    }
    if (cut_chunk == 0xFFFFFFFFu) {
        head = res::head_of(c, c.n_socks, all);
        *c.totals = res::totals_of(all, all);
    } else {
        res::Sums excl = base[cut_chunk];
        bool found = false;
        for (uint32_t i = cut_chunk * res::kChunk; i < c.n_socks && i < (cut_chunk + 1) * res::kChunk && !found; ++i) {
            const res::Sums s = res::sums_of(res::plan_sock(c, i));
            if (s.recs && !res::fits(c, res::add(excl, s))) {
                head = res::head_of(c, i, excl);
                *c.totals = res::totals_of(excl, all);
                found = true;
            }
            excl = res::add(excl, s);
        }
        CHECK(found);
    }
    res::write_prefix_end(head, block);
    for (uint32_t k = 0; k < chunks; ++k) {
        res::Sums excl = base[k];
        for (uint32_t i = k * res::kChunk; i < c.n_socks && i < (k + 1) * res::kChunk; ++i) {
            const res::SockPlan q = res::plan_sock(c, i);
            res::write_sock(c, head, block, i, q, excl);
            excl = res::add(excl, res::sums_of(q));
        }
    }
}

static Result run(const std::vector<fs_tx_sock>& socks, uint64_t rings_bytes, uint32_t cap, uint64_t frames_bytes, uint32_t flags,
                  uint32_t align, bool chunked, const fs_rx_sock_out* so = nullptr, const fs_rx_snd_out* sn = nullptr,
                  const uint32_t* idx = nullptr, uint32_t n_rx = 0) {
    Result r;
    r.table = socks;
    r.outs.resize(socks.size());
    const res::Scratch sl = res::scratch_of((uint32_t)socks.size(), cap);
    r.block.assign(sl.block_cap, 0);  // exactly the bytes the call's scratch has for the block
    res::Call c = call_of(r.table, r.outs, r.totals, rings_bytes, cap, frames_bytes, flags, align);
    c.rx_socks_out = so, c.rx_snd_out = sn, c.rx_index = idx, c.n_rx = n_rx;
    if (chunked) plan_chunked(c, r.head, r.block.data());
    else plan_sequential(c, r.head, r.block.data());
    return r;
}

// What fs_send_rings_batch gives for `built` (valid sockets): records and the staged block.
static void host_call(const std::vector<fs_tx_sock>& built, uint32_t flags, uint32_t align, sd::Layout& L,
                      std::vector<fs_tx_sock_out>& outs, std::vector<uint8_t>& block, seg::Block& b) {
    outs.resize(built.size());
    L = sd::layout(built.data(), (uint32_t)built.size(), flags & FS_FCS_APPEND, align, false, 0, outs.data());
    CHECK(L.bad == sd::kGood);
    b = sd::block_of(L.n_recs, L.id_entries);
    block.assign(b.bytes, 0);
    sd::stage(built.data(), (uint32_t)built.size(), flags & FS_FCS_APPEND, align, b, block.data());
}

// Everything the header states, for `r` = the call on `socks` (`handed`: the sockets behind step 1, for the
// valid ones), with `invalid[i]` the expected reason of socket i (0: valid).
static void verify(const std::vector<fs_tx_sock>& socks, const std::vector<fs_tx_sock>& handed, const std::vector<uint32_t>& invalid,
                   const Result& r, uint32_t cap, uint64_t frames_bytes, uint32_t flags, uint32_t align) {
    const uint32_t n = (uint32_t)socks.size();
    std::vector<fs_tx_sock> built;
    std::vector<uint32_t> built_at;
    uint64_t F = 0, B = 0;
    uint32_t idle = 0, deferred = 0, bad = 0;
    bool cut = false;
    for (uint32_t i = 0; i < n; ++i) {
        const fs_tx_sock_out& o = r.outs[i];
        if (invalid[i]) {
            ++bad;
            CHECK(o.sent == (FS_TX_INVALID | (invalid[i] << 16)) && o.n_frames == 0 && o.first_frame == FS_SEND_NONE);
            CHECK(o.snd_nxt == socks[i].snd_nxt && o.ring_rpos == socks[i].ring_rpos && o.ring_buffered == socks[i].ring_buffered);
            CHECK(std::memcmp(&r.table[i], &socks[i], sizeof(fs_tx_sock)) == 0);
            continue;
        }
        const sd::Plan p = sd::plan_of(handed[i]);
        if (p.frames == 0) {
            ++idle;
            CHECK(o.sent == 0 && o.n_frames == 0 && o.bytes == 0 && o.first_frame == FS_SEND_NONE);
            continue;
        }
        F += p.frames;
        B += sd::sock_bytes(handed[i], p, flags & FS_FCS_APPEND, align);
        if (F > cap || B > frames_bytes) cut = true;
        if (cut) {
            ++deferred;
            CHECK(o.sent == FS_TX_DEFERRED && o.n_frames == 0 && o.bytes == 0 && o.first_frame == FS_SEND_NONE);
            CHECK(o.snd_nxt == socks[i].snd_nxt && o.ring_rpos == socks[i].ring_rpos && o.ring_buffered == socks[i].ring_buffered);
            CHECK(o.ip_id == sd::template_id(socks[i]));
        } else {
            built.push_back(handed[i]);
            built_at.push_back(i);
        }
    }
    sd::Layout L;
    std::vector<fs_tx_sock_out> outs;
    std::vector<uint8_t> block;
    seg::Block b;
    host_call(built, flags, align, L, outs, block, b);
    for (size_t k = 0; k < built.size(); ++k) CHECK(std::memcmp(&r.outs[built_at[k]], &outs[k], sizeof(fs_tx_sock_out)) == 0);
    CHECK(r.head.n_recs == L.n_recs && r.head.n_frames == L.n_frames && r.head.recs_at == b.recs_at &&
          r.head.prefix_at == b.prefix_at && r.head.ids_at == b.ids_at && r.head.block_bytes == b.bytes);
    CHECK(r.head.tile == seg::tile_frames(L.n_frames, 24));
    CHECK(b.bytes <= r.block.size());
    CHECK(std::memcmp(r.block.data(), block.data(), b.bytes) == 0);  // send::stage's block, byte for byte
    for (size_t k = b.bytes; k < r.block.size(); ++k)
        if (r.block[k] != 0) {
            CHECK(!"a byte behind the block was written");
            break;
        }
    CHECK(r.totals.n_frames == L.n_frames && r.totals.frames_bytes == L.frames_bytes && r.totals.data_bytes == L.data);
    CHECK(r.totals.n_built == built.size() && r.totals.n_idle == idle && r.totals.n_deferred == deferred && r.totals.n_invalid == bad);
    CHECK(r.totals.n_frames <= cap && r.totals.frames_bytes <= frames_bytes);
    if (!(flags & FS_TX_WRITEBACK)) {
        CHECK(std::memcmp(r.table.data(), socks.data(), n * sizeof(fs_tx_sock)) == 0);  // the table is only read
        return;
    }
    // the write-back: the host chain through socks_out for the built, the hand-off for the other valid sockets
    size_t k = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (invalid[i]) continue;
        fs_tx_sock want = handed[i];
        if (k < built_at.size() && built_at[k] == i) {
            want.snd_nxt = outs[k].snd_nxt, want.ring_rpos = outs[k].ring_rpos, want.ring_buffered = outs[k].ring_buffered;
            want.hdr[18] = (uint8_t)(outs[k].ip_id >> 8), want.hdr[19] = (uint8_t)outs[k].ip_id;
            want.flags &= ~(FS_TX_ACK | (outs[k].sent & FS_TX_FIN));
            ++k;
        }
        CHECK(std::memcmp(&r.table[i], &want, sizeof want) == 0);
    }
}

static void both(const std::vector<fs_tx_sock>& socks, uint64_t rings_bytes, uint32_t cap, uint64_t frames_bytes, uint32_t flags,
                 uint32_t align, const std::vector<uint32_t>& invalid) {
    for (int chunked = 0; chunked < 2; ++chunked)
        verify(socks, socks, invalid, run(socks, rings_bytes, cap, frames_bytes, flags, align, chunked != 0), cap, frames_bytes,
               flags, align);
}

static void test_ample_and_cuts() {
    for (uint32_t n : {1u, 12u, 255u, 256u, 257u, 700u}) {
        uint64_t rings_bytes = 0;
        const std::vector<fs_tx_sock> socks = mixed(n, rings_bytes);
        const std::vector<uint32_t> valid(n, 0);
        sd::Layout L = sd::layout(socks.data(), n, 0, 1, true, rings_bytes, nullptr);
        CHECK(L.bad == sd::kGood && (n < 12 || L.n_frames > n / 2));
        both(socks, rings_bytes, 1u << 31, ~0ull, 0, 1, valid);
        both(socks, rings_bytes, 1u << 31, ~0ull, FS_FCS_APPEND | FS_TX_WRITEBACK, 64, valid);
        both(socks, rings_bytes, (uint32_t)L.n_frames, L.frames_bytes, 0, 1, valid);  // exactly enough
        both(socks, rings_bytes, 0, ~0ull, 0, 1, valid);
        both(socks, rings_bytes, 1u << 31, 0, FS_TX_WRITEBACK, 1, valid);
        // cut at every socket's end, one frame or one byte short of it, and inside it
        uint64_t F = 0, B = 0;
        for (uint32_t i = 0; i < n; i += n > 300 ? 37 : n > 20 ? 9 : 1) {
            F = B = 0;
            for (uint32_t j = 0; j <= i; ++j) {
                const sd::Plan p = sd::plan_of(socks[j]);
                if (p.frames) F += p.frames, B += sd::sock_bytes(socks[j], p, 0, 4);
            }
            for (uint64_t cap : {F, F - (F ? 1 : 0), F + 1})
                both(socks, rings_bytes, (uint32_t)cap, ~0ull, FS_TX_WRITEBACK, 4, valid);
            for (uint64_t bytes : {B, B - (B ? 1 : 0), B + 1}) both(socks, rings_bytes, 1u << 31, bytes, 0, 4, valid);
        }
    }
}

static void test_invalid() {
    uint64_t rings_bytes = 0;
    const std::vector<fs_tx_sock> good = mixed(40, rings_bytes);
    struct Edit {
        uint32_t reason;
        void (*apply)(fs_tx_sock&, uint64_t);
    };
    const Edit edits[] = {
        {FS_TX_BAD_ETHERTYPE, [](fs_tx_sock& s, uint64_t) { s.hdr[13] = 6; }},
        {FS_TX_BAD_IHL, [](fs_tx_sock& s, uint64_t) { s.hdr[14] = 0x46; }},
        {FS_TX_BAD_PROTO, [](fs_tx_sock& s, uint64_t) { s.hdr[23] = 17; }},
        {FS_TX_BAD_DATA_OFFSET, [](fs_tx_sock& s, uint64_t) { s.hdr[46] = 0x60; }},
        {FS_TX_BAD_MSS, [](fs_tx_sock& s, uint64_t) { s.mss = 0; }},
        {FS_TX_BAD_SOCK_FLAGS, [](fs_tx_sock& s, uint64_t) { s.flags = 8; }},
        {FS_TX_BAD_MAX_FRAMES, [](fs_tx_sock& s, uint64_t) { s.max_frames = FS_SEGMENT_MAX_FRAMES + 1; }},
        {FS_TX_BAD_RING_SIZE, [](fs_tx_sock& s, uint64_t) { s.ring_size = 0; }},
        {FS_TX_BAD_RING_POS, [](fs_tx_sock& s, uint64_t) { s.ring_rpos = s.ring_size; }},
        {FS_TX_BAD_BUFFERED, [](fs_tx_sock& s, uint64_t) { s.ring_buffered = s.ring_size + 1; }},
        {FS_TX_BAD_RING_RANGE, [](fs_tx_sock& s, uint64_t bytes) { s.ring_off = bytes - s.ring_size + 1; }},
    };
    for (const Edit& e : edits)
        for (uint32_t at : {0u, 20u, 39u}) {
            std::vector<fs_tx_sock> socks = good;
            std::vector<uint32_t> invalid(socks.size(), 0);
            e.apply(socks[at], rings_bytes);
            invalid[at] = e.reason;
            both(socks, rings_bytes, 1u << 31, ~0ull, FS_TX_WRITEBACK, 1, invalid);
            both(socks, rings_bytes, 30, ~0ull, 0, 1, invalid);
        }
}

static void test_hand_off() {
    uint64_t rings_bytes = 0;
    const uint32_t n = 300;
    const std::vector<fs_tx_sock> socks = mixed(n, rings_bytes);
    std::vector<fs_rx_sock_out> so(n);
    std::vector<fs_rx_snd_out> sn(n);
    for (uint32_t r = 0; r < n; ++r) {
        std::memset(&so[r], 0, sizeof so[r]);
        std::memset(&sn[r], 0, sizeof sn[r]);
        so[r].rcv_nxt = 0xFFFFFF00u + rnd(512), so[r].ring_free = rnd(140000);
        sn[r].snd_una = socks[r].snd_nxt - rnd(3), sn[r].snd_wnd = rnd(65536), sn[r].flags = rnd(4);
    }
    std::vector<uint32_t> idx(n);
    for (uint32_t i = 0; i < n; ++i) idx[i] = (i * 7 + 3) % n;
    idx[0] = idx[150] = FS_TX_NO_RX;
    idx[9] = n, idx[299] = 0xFFFFFFFEu;
    for (int with_snd = 0; with_snd < 2; ++with_snd)
        for (int with_idx = 0; with_idx < 2; ++with_idx) {
            std::vector<fs_tx_sock> handed = socks;
            std::vector<uint32_t> invalid(n, 0);
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t r = with_idx ? idx[i] : i;
                if (r == FS_TX_NO_RX) continue;
                if (r >= n) {
                    invalid[i] = FS_TX_BAD_RX_INDEX;
                    continue;
                }
                handed[i].rcv_nxt = so[r].rcv_nxt, handed[i].rcv_wnd = so[r].ring_free;
                if (with_snd) {
                    handed[i].snd_una = sn[r].snd_una, handed[i].snd_wnd = sn[r].snd_wnd;
                    if (sn[r].flags & FS_RECV_ACK_OWED) handed[i].flags |= FS_TX_ACK;
                }
            }
            for (int chunked = 0; chunked < 2; ++chunked)
                for (uint32_t cap : {1u << 31, 200u}) {
                    const uint32_t flags = chunked ? FS_TX_WRITEBACK : 0;
                    verify(socks, handed, invalid,
                           run(socks, rings_bytes, cap, ~0ull, flags, 1, chunked != 0, so.data(), with_snd ? sn.data() : nullptr,
                               with_idx ? idx.data() : nullptr, n),
                           cap, ~0ull, flags, 1);
                }
        }
}

static void test_scratch() {
    // the block's room covers the largest block the built sockets of a call can make
    for (uint32_t n : {1u, 256u, 65536u})
        for (uint32_t cap : {0u, 1u, 63u, 64u, 65u, 4096u, 65536u, 1u << 22, 1u << 31}) {
            const res::Scratch s = res::scratch_of(n, cap);
            const uint32_t recs = n < cap ? n : cap;
            // the worst cases: every record one frame; as few records as hold cap frames, 4,096 each
            CHECK(s.block_cap >= sd::block_of(recs, recs).bytes);
            const uint64_t full = cap / FS_SEGMENT_MAX_FRAMES < n ? cap / FS_SEGMENT_MAX_FRAMES : n;
            CHECK(s.block_cap >= sd::block_of((uint32_t)full, full * 64).bytes);
            CHECK(s.block % 64 == 0 && s.head >= s.chunk_base && s.bytes == s.block + s.block_cap);
            CHECK(s.bytes < (64ull << 20));
        }
}

int main() {
    test_ample_and_cuts();
    test_invalid();
    test_hand_off();
    test_scratch();
    if (g_failed) {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("send resident checks OK\n");
    return 0;
}
