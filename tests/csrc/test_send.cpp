// The arithmetic of the ring send (seqs_amd/csrc/framesum_send.h) on the CPU, built alone under ASan +
// UBSan by tests/test_send_host.py: every rejection of a socket, the per-socket rule at each of its
// boundaries (the window room, sequence numbers across 2^32, FIN with and without data, the max_frames
// cap), the layout, and the staged block on exactly sized heap arrays: the records, the strictly
// increasing prefix the frame -> record search needs, the ID powers, the headers, and the split of
// every chunk at the ring's end against a byte-by-byte walk of the ring.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../seqs_amd/csrc/framesum_send.h"

namespace sd = framesum::send;
namespace seg = framesum::segment;

static int g_failed = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                  \
        }                                                                \
    } while (0)

static fs_tx_sock sock(uint32_t mss, uint64_t ring_off, uint32_t ring_size, uint32_t rpos, uint32_t buffered) {
    fs_tx_sock s;
    std::memset(&s, 0, sizeof s);
    for (int i = 0; i < 54; ++i) s.hdr[i] = (uint8_t)(0xA0 + i);
    s.hdr[12] = 0x08, s.hdr[13] = 0x00, s.hdr[14] = 0x45, s.hdr[23] = 6, s.hdr[46] = 0x50;
    s.hdr[18] = 0x12, s.hdr[19] = 0x34;
    s.mss = (uint16_t)mss;
    s.ring_off = ring_off;
    s.ring_size = ring_size;
    s.ring_rpos = rpos;
    s.ring_buffered = buffered;
    s.snd_una = 1000, s.snd_nxt = 1500, s.snd_wnd = 1u << 20;
    s.rcv_nxt = 0x01020304, s.rcv_wnd = 65535;
    return s;
}

static void test_rejections() {
    const uint64_t bytes = 1u << 20;
    fs_tx_sock s = sock(100, 0, 4096, 0, 0);
    CHECK(sd::check_sock(s, true, bytes) == sd::kGood);
    fs_tx_sock b = s;
    b.hdr[13] = 0x06;
    CHECK(sd::check_sock(b, true, bytes) == sd::kBadEtherType);
    b = s, b.hdr[14] = 0x46;
    CHECK(sd::check_sock(b, true, bytes) == sd::kBadIhl);
    b = s, b.hdr[23] = 17;
    CHECK(sd::check_sock(b, true, bytes) == sd::kBadProto);
    b = s, b.hdr[46] = 0x60;
    CHECK(sd::check_sock(b, true, bytes) == sd::kBadDataOffset);
    b = s, b.mss = 0;
    CHECK(sd::check_sock(b, true, bytes) == sd::kBadMss);
    b = s, b.mss = 65496;
    CHECK(sd::check_sock(b, true, bytes) == sd::kBadMss);
    b = s, b.mss = 65495;
    CHECK(sd::check_sock(b, true, bytes) == sd::kGood);
    b = s, b.flags = 8;
    CHECK(sd::check_sock(b, true, bytes) == sd::kBadSockFlags);
    b = s, b.flags = FS_TX_ACK | FS_TX_FIN | FS_TX_PSH;
    CHECK(sd::check_sock(b, true, bytes) == sd::kGood);
    b = s, b.max_frames = FS_SEGMENT_MAX_FRAMES + 1;
    CHECK(sd::check_sock(b, true, bytes) == sd::kBadMaxFrames);
    b = s, b.max_frames = FS_SEGMENT_MAX_FRAMES;
    CHECK(sd::check_sock(b, true, bytes) == sd::kGood);
    b = s, b.ring_size = 0;
    CHECK(sd::check_sock(b, true, bytes) == sd::kBadRingSize);
    b = s, b.ring_size = 0x80000001u;
    CHECK(sd::check_sock(b, false, 0) == sd::kBadRingSize);
    b = s, b.ring_size = 0x80000000u;
    CHECK(sd::check_sock(b, false, 0) == sd::kGood);
    b = s, b.ring_rpos = 4096;
    CHECK(sd::check_sock(b, true, bytes) == sd::kBadRingPos);
    b = s, b.ring_buffered = 4097;
    CHECK(sd::check_sock(b, true, bytes) == sd::kBadBuffered);
    b = s, b.ring_buffered = 4096, b.ring_rpos = 4095;
    CHECK(sd::check_sock(b, true, bytes) == sd::kGood);
    b = s, b.ring_off = bytes - 4095;
    CHECK(sd::check_sock(b, true, bytes) == sd::kBadRingRange);
    CHECK(sd::check_sock(b, false, 0) == sd::kGood);  // (the layout call has no rings_bytes)
    b = s, b.ring_off = bytes - 4096;
    CHECK(sd::check_sock(b, true, bytes) == sd::kGood);
    b = s, b.ring_off = ~0ull - 100;  // ring_off + ring_size wraps 64 bits
    CHECK(sd::check_sock(b, true, bytes) == sd::kBadRingRange);
    // the layout names the first bad socket and writes no total
    std::vector<fs_tx_sock> v(5, sock(100, 0, 4096, 0, 10));
    v[3].mss = 0;
    v[4].ring_size = 0;
    const sd::Layout L = sd::layout(v.data(), 5, 0, 1, true, bytes, nullptr);
    CHECK(L.bad == sd::kBadMss && L.bad_sock == 3);
}

static void test_rule() {
    // 500 in flight, 1,000 buffered, mss 100
    fs_tx_sock s = sock(100, 0, 4096, 4000, 1000);
    struct Case {
        uint32_t wnd, data, frames;
    } rooms[] = {{500, 0, 0},     {501, 1, 1},      {599, 99, 1},    {600, 100, 1},    {601, 101, 2}, {1499, 999, 10},
                 {1500, 1000, 10}, {1501, 1000, 10}, {100, 0, 0} /* in_flight > snd_wnd */, {0, 0, 0}};
    for (const Case& c : rooms) {
        s.snd_wnd = c.wnd;
        const sd::Plan p = sd::plan_of(s);
        CHECK(p.data == c.data && p.frames == c.frames && !p.fin && p.tcp_flags == 0x10);
        const fs_tx_sock_out o = sd::out_of(s, p, 7);
        CHECK(o.snd_nxt == 1500 + c.data && o.ring_rpos == (4000 + c.data) % 4096 && o.ring_buffered == 1000 - c.data);
        CHECK(o.bytes == c.data && o.n_frames == c.frames && o.first_frame == (c.frames ? 7u : FS_SEND_NONE) && o.sent == 0);
        CHECK(o.ip_id == sd::advance_id(0x1234, c.frames));
        // FS_TX_ACK: a frame where there was none, nothing else
        s.flags = FS_TX_ACK;
        const sd::Plan q = sd::plan_of(s);
        CHECK(q.data == c.data && q.frames == (c.frames ? c.frames : 1u) && q.tcp_flags == 0x10);
        CHECK(sd::out_of(s, q, 0).sent == (c.data ? 0u : (uint32_t)FS_TX_ACK));
        s.flags = 0;
    }
    // FIN: with the last data, alone, held back by the window and by the cap; it takes no room
    s.snd_wnd = 1u << 20;
    s.flags = FS_TX_FIN | FS_TX_PSH;
    sd::Plan p = sd::plan_of(s);
    CHECK(p.data == 1000 && p.frames == 10 && p.fin && p.tcp_flags == 0x19);
    fs_tx_sock_out o = sd::out_of(s, p, 0);
    CHECK(o.snd_nxt == 2501 && o.sent == FS_TX_FIN && o.ring_rpos == 904 && o.ring_buffered == 0);
    s.snd_wnd = 1500;  // room == buffered
    p = sd::plan_of(s);
    CHECK(p.data == 1000 && p.fin);
    s.snd_wnd = 1499;
    p = sd::plan_of(s);
    CHECK(p.data == 999 && !p.fin && p.tcp_flags == 0x18);
    s.snd_wnd = 1u << 20, s.max_frames = 3;
    p = sd::plan_of(s);
    CHECK(p.data == 300 && p.frames == 3 && !p.fin && sd::out_of(s, p, 0).sent == 0);
    s.max_frames = 10;
    p = sd::plan_of(s);
    CHECK(p.data == 1000 && p.frames == 10 && p.fin);
    s.max_frames = 0, s.ring_buffered = 0;
    p = sd::plan_of(s);
    CHECK(p.data == 0 && p.frames == 1 && p.fin && p.tcp_flags == 0x11);  // (no data segment: no PSH)
    o = sd::out_of(s, p, 3);
    CHECK(o.snd_nxt == 1501 && o.sent == FS_TX_FIN && o.first_frame == 3 && o.ring_rpos == 4000);
    s.snd_wnd = 0;  // ... and no window room is needed
    CHECK(sd::plan_of(s).fin && sd::plan_of(s).frames == 1);
    s.flags = FS_TX_PSH;
    CHECK(sd::plan_of(s).frames == 0);
    // sequence numbers across 2^32
    s = sock(100, 0, 4096, 0, 1000);
    s.snd_una = 0xFFFFFF00u, s.snd_nxt = 0x00000010u, s.snd_wnd = 0x110 + 250;  // 0x110 in flight
    p = sd::plan_of(s);
    CHECK(sd::room_of(s) == 250 && p.data == 250 && p.frames == 3);
    s.snd_una = 0xFFFFFE00u, s.snd_nxt = 0xFFFFFFFCu, s.snd_wnd = 1u << 20, s.ring_buffered = 4, s.flags = FS_TX_FIN;
    p = sd::plan_of(s);
    CHECK(sd::out_of(s, p, 0).snd_nxt == 1);
    // the largest products
    s = sock(65495, 0, 0x80000000u, 0x7FFFFFFFu, 0x80000000u);
    s.snd_una = s.snd_nxt = 0, s.snd_wnd = 0xFFFFFFFFu;
    p = sd::plan_of(s);
    CHECK(p.data == 4096u * 65495u && p.frames == 4096);
    CHECK(sd::out_of(s, p, 0).ring_rpos == (uint32_t)((0x7FFFFFFFull + p.data) % 0x80000000ull));
    // advance_id is prand16 applied n times
    uint16_t id = 0xBEEF;
    for (uint32_t n = 0; n <= 200; ++n) {
        CHECK(sd::advance_id(0xBEEF, n) == id);
        id = seg::prand16(id);
    }
}

// The staged block of a batch against a walk of every socket by the rule, on arrays of exactly the
// block's and the rings' sizes.
static void check_batch(const std::vector<fs_tx_sock>& socks, const std::vector<uint8_t>& rings, uint32_t flags,
                        uint32_t align) {
    const uint32_t n = (uint32_t)socks.size();
    std::vector<fs_tx_sock_out> outs(n);
    const sd::Layout L = sd::layout(socks.data(), n, flags, align, true, rings.size(), outs.data());
    CHECK(L.bad == sd::kGood);
    if (L.bad != sd::kGood || L.n_frames == 0) return;
    const seg::Block b = sd::block_of(L.n_recs, L.id_entries);
    uint8_t* block = static_cast<uint8_t*>(std::malloc(b.bytes));
    sd::stage(socks.data(), n, flags, align, b, block);
    const sd::RingRec* recs = reinterpret_cast<const sd::RingRec*>(block + b.recs_at);
    const uint32_t* prefix = reinterpret_cast<const uint32_t*>(block + b.prefix_at);
    const uint16_t* ids = reinterpret_cast<const uint16_t*>(block + b.ids_at);
    CHECK(prefix[L.n_recs] == L.n_frames);
    uint64_t frame = 0, base = 0, data = 0;
    uint32_t r = 0;
    const uint32_t fcs = (flags & FS_FCS_APPEND) ? 4 : 0;
    for (uint32_t i = 0; i < n; ++i) {
        const fs_tx_sock& s = socks[i];
        const sd::Plan p = sd::plan_of(s);
        CHECK(outs[i].n_frames == p.frames && outs[i].first_frame == (p.frames ? (uint32_t)frame : FS_SEND_NONE));
        if (p.frames == 0) continue;
        const sd::RingRec& rec = recs[r];
        CHECK(prefix[r] == frame && prefix[r + 1] > prefix[r] && rec.frames == p.frames && rec.data == p.data);
        CHECK(rec.frame_base == base && rec.mss == s.mss && rec.ring_off == s.ring_off && rec.ring_size == s.ring_size);
        // the header: Seq, Ack, flags and window, every other byte the template's
        uint8_t want[54];
        std::memcpy(want, s.hdr, 54);
        for (int k = 0; k < 4; ++k) {
            want[38 + k] = (uint8_t)(s.snd_nxt >> (24 - 8 * k));
            want[42 + k] = (uint8_t)(s.rcv_nxt >> (24 - 8 * k));
        }
        want[47] = p.tcp_flags;
        const uint32_t wnd = s.rcv_wnd > 65535 ? 65535 : s.rcv_wnd;
        want[48] = (uint8_t)(wnd >> 8), want[49] = (uint8_t)wnd;
        CHECK(std::memcmp(want, rec.hdr, 54) == 0);
        uint16_t id = sd::template_id(s);
        uint64_t sent = 0;
        for (uint32_t k = 0; k < p.frames; ++k) {
            CHECK(seg::find_send(prefix, L.n_recs, (uint32_t)(frame + k)) == r);
            const uint32_t C = sd::rec_chunk(rec, k), p0 = sd::rec_pos(rec, k), w = sd::rec_before_wrap(rec, k);
            CHECK(C == sd::chunk_of(s, p, k) && (k + 1 == p.frames ? C <= s.mss : C == s.mss) && p0 < s.ring_size);
            // the split: bytes [0, min(C, w)) from p0 on, the rest from the ring's start; all inside rings
            for (uint32_t j = 0; j < C; ++j) {
                const uint64_t model = s.ring_off + ((uint64_t)s.ring_rpos + sent + j) % s.ring_size;
                const uint64_t mine = s.ring_off + (j < w ? (uint64_t)p0 + j : (uint64_t)j - w);
                CHECK(mine == model);
                (void)rings.at(mine);
            }
            sent += C;
            // the ID chain through the staged powers
            uint16_t got = ids[rec.id_at + k / seg::kIdStride];
            for (uint32_t q = 0; q < k % seg::kIdStride; ++q) got = seg::prand16(got);
            CHECK(got == id);
            id = seg::prand16(id);
            base += seg::slot_bytes(seg::kTcpHdr + C, flags, align);
        }
        CHECK(sent == p.data && outs[i].ip_id == id);
        data += p.data;
        frame += p.frames;
        ++r;
    }
    CHECK(r == L.n_recs && frame == L.n_frames && base == L.frames_bytes && data == L.data);
    CHECK(L.written == L.n_frames * (seg::kTcpHdr + fcs) + L.data);
    CHECK(L.data == 0 || (L.read_lo < L.read_hi && L.read_hi <= rings.size()));
    std::free(block);
}

static void test_batches() {
    std::vector<uint8_t> rings(5000);
    // the wrap at every position of a chunk, chunk boundaries on the wrap, rings of 1 and 2 bytes
    std::vector<fs_tx_sock> v;
    for (uint32_t rpos = 4096 - 1020; rpos < 4096; rpos += 7) v.push_back(sock(100, 904, 4096, rpos, 1000));
    v.push_back(sock(100, 904, 4096, 3096, 1000));  // rpos + data == ring_size
    v.push_back(sock(100, 904, 4096, 3196, 1000));  // a chunk boundary on the wrap
    for (uint32_t size : {1u, 2u, 15u, 16u, 17u})
        for (uint32_t rpos = 0; rpos < size; ++rpos) v.push_back(sock(5, 5000 - size, size, rpos, size));
    fs_tx_sock quiet = sock(100, 0, 64, 3, 0);
    v.insert(v.begin(), quiet);  // S == 0 first, in the middle and last
    v.insert(v.begin() + 40, quiet);
    v.push_back(quiet);
    fs_tx_sock ack = quiet;
    ack.flags = FS_TX_ACK;
    v.push_back(ack);
    v.push_back(quiet);
    for (uint32_t flags : {0u, (uint32_t)FS_FCS_APPEND})
        for (uint32_t align : {1u, 4u, 64u, 4096u}) check_batch(v, rings, flags, align);
    // a long socket: more than one staged ID power, the ring read from its last byte
    std::vector<uint8_t> big(70000);
    fs_tx_sock l = sock(16, 3, 65536, 65535, 65536);
    l.flags = FS_TX_FIN;
    check_batch({quiet, l, l}, big, 0, 1);
    // nothing to send at all
    std::vector<fs_tx_sock_out> outs(2);
    const std::vector<fs_tx_sock> none = {quiet, quiet};
    const sd::Layout L = sd::layout(none.data(), 2, 0, 1, true, 64, outs.data());
    CHECK(L.bad == sd::kGood && L.n_frames == 0 && L.frames_bytes == 0 && L.n_recs == 0 && L.read_lo == L.read_hi);
    CHECK(outs[1].first_frame == FS_SEND_NONE && outs[1].snd_nxt == 1500 && outs[1].ring_rpos == 3 && outs[1].ip_id == 0x1234);
}

// The TX frame build's helpers as the ring send uses them: the block over 96-byte records, a record's
// chunks, and its staged ID powers against segment::rec_id over a SendRec with the same id_at.
static void test_shared_helpers() {
    const seg::Block b = seg::block_of(3, sizeof(sd::RingRec), 5), s = seg::block_of(3, sizeof(seg::SendRec), 5);
    CHECK(sizeof(sd::RingRec) == 96 && b.recs_at == 0 && b.prefix_at == 288 && b.ids_at == 304 && b.bytes == 320);
    CHECK(s.prefix_at == 264 && s.ids_at == 280 && s.bytes == 320);
    CHECK(sd::block_of(3, 5).prefix_at == b.prefix_at && sd::block_of(3, 5).bytes == b.bytes && seg::block_of(3, 5).ids_at == 280);
    CHECK(seg::block_of(0, 96, 0).bytes == 64 && seg::block_of(2, 96, 26).bytes == 256 && seg::block_of(2, 96, 27).bytes == 320);
    sd::RingRec r{};
    r.mss = 100, r.data = 1000, r.id_at = 1;
    CHECK(sd::rec_chunk(r, 9) == 100 && sd::rec_chunk(r, 10) == 0 && seg::chunk_at(1000, 100, 10) == 0);  // k mss == total
    r.data = 1001;
    CHECK(sd::rec_chunk(r, 10) == 1 && sd::rec_chunk(r, 11) == 0);
    CHECK(seg::chunk_at(1001, 0, 0) == 1001 && seg::chunk_at(1001, 0, 3) == 1001);  // (mss == 0: no socket has it)
    const fs_tx_sock k = sock(100, 0, 4096, 5, 1000);
    CHECK(sd::chunk_of(k, sd::plan_of(k), 9) == 100 && sd::chunk_of(k, sd::plan_of(k), 10) == 0);
    seg::SendRec as_send{};
    as_send.id_at = r.id_at;
    for (uint32_t frames : {1u, 64u, 65u, 200u, 4096u}) {
        std::vector<uint16_t> ids(1 + (frames + 63) / 64, 0xEEEE);
        CHECK(seg::stage_ids(0x1234, frames, ids.data(), 1) == ids.size() && ids[0] == 0xEEEE);
        for (uint32_t f = 0; f < frames; ++f) CHECK(seg::rec_id(as_send, ids.data(), f) == sd::advance_id(0x1234, f));
    }
}

int main() {
    test_rejections();
    test_rule();
    test_batches();
    test_shared_helpers();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("send checks OK\n");
    return 0;
}
