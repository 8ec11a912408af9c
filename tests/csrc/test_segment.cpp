// seqs_amd/csrc/framesum_segment.h (the host arithmetic of the TX frame build) alone, under
// ASan + UBSan: frames per send, the prefix of frame indices and byte bases, the frame -> send
// search the kernel runs, the staged block, and every FS_E_INVALID case of the layout.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../seqs_amd/csrc/framesum_segment.h"

namespace seg = framesum::segment;

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

static fs_tx_send tcp_send(uint16_t mss, uint32_t len, uint64_t off = 0) {
    fs_tx_send s;
    memset(&s, 0, sizeof s);
    s.hdr[12] = 0x08;
    s.hdr[14] = 0x45;
    s.hdr[23] = 6;
    s.hdr[46] = 0x50;
    s.hdr[18] = 0x12;
    s.hdr[19] = 0x34;
    s.mss = mss;
    s.payload_len = len;
    s.payload_off = off;
    return s;
}
static fs_tx_send udp_send(uint32_t len, uint64_t off = 0) {
    fs_tx_send s = tcp_send(0, len, off);
    s.hdr[23] = 17;
    s.hdr[46] = 0;
    return s;
}

// the plain definition the header's arithmetic must agree with
static uint32_t frames_plain(const fs_tx_send& s) {
    if (s.mss == 0 || s.payload_len == 0) return 1;
    uint32_t n = 0;
    for (uint64_t at = 0; at < s.payload_len; at += s.mss) ++n;
    return n;
}

static void check_batch(const std::vector<fs_tx_send>& sends, uint32_t flags, uint32_t align) {
    const uint32_t n = (uint32_t)sends.size();
    const seg::Layout L = seg::layout(sends.data(), n, flags, align, false, 0);
    CHECK(L.bad == seg::kGood);
    const seg::Block b = seg::block_of(n, L.id_entries);
    std::vector<uint64_t> block(b.bytes / 8);  // exactly the staged bytes: ASan sees any overrun
    uint8_t* blk = reinterpret_cast<uint8_t*>(block.data());
    seg::stage(sends.data(), n, flags, align, b, blk);
    const seg::SendRec* recs = reinterpret_cast<const seg::SendRec*>(blk + b.recs_at);
    const uint32_t* prefix = reinterpret_cast<const uint32_t*>(blk + b.prefix_at);
    const uint16_t* ids = reinterpret_cast<const uint16_t*>(blk + b.ids_at);
    const uint32_t fcs = (flags & FS_FCS_APPEND) ? 4u : 0u;
    uint64_t frame = 0, at = 0, written = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const fs_tx_send& s = sends[i];
        const uint32_t S = frames_plain(s), h = seg::hdr_len(s);
        CHECK(seg::frames_of(s) == S && recs[i].frames == S);
        CHECK(prefix[i] == frame && recs[i].frame_base == at);
        uint16_t id = (uint16_t)((s.hdr[18] << 8) | s.hdr[19]);
        uint64_t carried = 0;
        for (uint32_t k = 0; k < S; ++k) {
            // frame k carries payload[k*mss, min(L, (k+1)*mss))
            const uint64_t lo = (uint64_t)k * s.mss;
            const uint64_t hi = s.mss == 0 ? s.payload_len : (lo + s.mss < s.payload_len ? lo + s.mss : s.payload_len);
            const uint32_t c = (uint32_t)(hi - (s.mss == 0 ? 0 : lo));
            CHECK(seg::chunk_of(s, k) == c && seg::rec_chunk(recs[i], k) == c);
            CHECK(seg::rec_frame_offset(recs[i], k, flags, align) == at);
            CHECK(at % align == 0);
            CHECK(seg::rec_id(recs[i], ids, k) == id);
            // frame -> send at every boundary: each frame of the batch is looked up
            CHECK(seg::find_send(prefix, n, (uint32_t)frame) == i && frame - prefix[i] == k);
            id = seg::prand16(id);
            const uint64_t slot = seg::slot_bytes(h + c, flags, align);
            CHECK(slot >= h + c + fcs && slot < h + c + fcs + align);
            at += slot;
            written += h + c + fcs;
            carried += c;
            ++frame;
        }
        CHECK(carried == s.payload_len);
    }
    CHECK(prefix[n] == frame && L.n_frames == frame && L.frames_bytes == at && L.written == written);
    if (align == 1) CHECK(L.written == L.frames_bytes);
}

static void expect_bad(fs_tx_send s, seg::Bad want, bool have_payload = false, uint64_t payload_bytes = 0) {
    const fs_tx_send good = tcp_send(100, 1000);
    const fs_tx_send sends[3] = {good, good, s};
    const seg::Layout L = seg::layout(sends, 3, 0, 4, have_payload, payload_bytes);
    CHECK(L.bad == want && L.bad_send == 2);
    CHECK(seg::bad_text(want)[0] != '?');
}

int main() {
    static_assert(seg::prand16(1) == 0x8181, "prand16(1)");
    const uint32_t aligns[] = {1, 4, 64, 4096};
    // counts and bases for L in {0, 1, mss-1, mss, mss+1, 4096 mss, 4096 mss + 1 (invalid)}
    for (uint16_t mss : {(uint16_t)1, (uint16_t)2, (uint16_t)63, (uint16_t)536, (uint16_t)1460}) {
        std::vector<fs_tx_send> sends;
        for (uint32_t len : {0u, 1u, (uint32_t)mss - 1, (uint32_t)mss, (uint32_t)mss + 1, 4096u * mss})
            sends.push_back(tcp_send(mss, len));
        sends.push_back(udp_send(0));
        sends.push_back(udp_send(1472));
        sends.push_back(tcp_send(0, 65495));
        sends.push_back(udp_send(65507));
        for (uint32_t align : aligns)
            for (uint32_t flags : {0u, (uint32_t)FS_FCS_APPEND}) check_batch(sends, flags, align);
        CHECK(seg::frames_of(tcp_send(mss, 4096u * mss)) == FS_SEGMENT_MAX_FRAMES);
        expect_bad(tcp_send(mss, 4096u * mss + 1), seg::kBadFrameCount);
    }
    // many sends: the search's rounds (more than 64, more than 4096 sends)
    {
        std::mt19937 rng(7);
        for (uint32_t n : {1u, 2u, 63u, 64u, 65u, 4095u, 4096u, 4097u, 10000u}) {
            std::vector<fs_tx_send> sends;
            for (uint32_t i = 0; i < n; ++i)
                sends.push_back(rng() % 4 == 0 ? udp_send(rng() % 1473) : tcp_send((uint16_t)(1 + rng() % 300), rng() % 1500));
            check_batch(sends, FS_FCS_APPEND, 4);
        }
    }
    // every invalid case
    {
        fs_tx_send s = tcp_send(100, 1000);
        s.reserved = 1;
        expect_bad(s, seg::kBadReserved);
        s = tcp_send(100, 1000);
        s.hdr[13] = 0x06;
        expect_bad(s, seg::kBadEtherType);
        s = tcp_send(100, 1000);
        s.hdr[14] = 0x46;
        expect_bad(s, seg::kBadIhl);
        s = tcp_send(100, 1000);
        s.hdr[23] = 1;
        expect_bad(s, seg::kBadProto);
        s = tcp_send(100, 1000);
        s.hdr[46] = 0x60;
        expect_bad(s, seg::kBadDataOffset);
        s = udp_send(100);
        s.mss = 50;
        expect_bad(s, seg::kBadUdpMss);
        expect_bad(tcp_send(0, 65496), seg::kBadChunk);
        expect_bad(tcp_send(65535, 65496), seg::kBadChunk);
        expect_bad(udp_send(65508), seg::kBadChunk);
        expect_bad(tcp_send(1, 4097), seg::kBadFrameCount);
        expect_bad(tcp_send(100, 1000, 1), seg::kBadPayloadRange, true, 1000);
        expect_bad(tcp_send(100, 1000, ~0ull), seg::kBadPayloadRange, true, 1ull << 40);
        expect_bad(tcp_send(100, 0, 1001), seg::kBadPayloadRange, true, 1000);
        // ... and their valid neighbours
        const fs_tx_send ok[] = {tcp_send(0, 65495), udp_send(65507), tcp_send(1, 4096), tcp_send(100, 1000, 0)};
        CHECK(seg::layout(ok, 4, 0, 4, true, 65507).bad == seg::kGood);
        CHECK(!seg::valid_align(0) && !seg::valid_align(3) && !seg::valid_align(8192) && seg::valid_align(1) &&
              seg::valid_align(4096));
        CHECK(seg::valid_flags(0) && seg::valid_flags(FS_FCS_APPEND) && !seg::valid_flags(FS_FILL_CSUM) && !seg::valid_flags(4));
    }
    // more than 2^31 frames in all: 2^19 + 1 sends of 4096 frames (the layout only, nothing staged)
    {
        std::vector<fs_tx_send> sends((1u << 19) + 1, tcp_send(1, 4096));
        seg::Layout L = seg::layout(sends.data(), 1u << 19, 0, 1, false, 0);
        CHECK(L.bad == seg::kGood && L.n_frames == seg::kMaxFrames);
        L = seg::layout(sends.data(), (1u << 19) + 1, 0, 1, false, 0);
        CHECK(L.bad == seg::kBadTotalFrames && L.bad_send == (1u << 19));
    }
    CHECK(seg::tile_frames(65536, 4096) == 16 && seg::tile_frames(1, 16) == 1 && seg::tile_frames(1u << 31, 4096) == 16 &&
          seg::tile_frames(100, 64) == 2);
    // the helpers the ring send shares. A block: the records, n + 1 prefix entries, the ID powers, up to 64
    {
        const seg::Block b = seg::block_of(3, sizeof(seg::SendRec), 5), e = seg::block_of(0, sizeof(seg::SendRec), 0);
        CHECK(b.recs_at == 0 && b.prefix_at == 3 * 88 && b.ids_at == 3 * 88 + 16 && b.bytes == 320);
        CHECK(e.prefix_at == 0 && e.ids_at == 4 && e.bytes == 64);
        CHECK(seg::block_of(3, 5).prefix_at == b.prefix_at && seg::block_of(3, 5).ids_at == b.ids_at && seg::block_of(3, 5).bytes == b.bytes);
        CHECK(seg::block_of(3, 96, 5).prefix_at == 288 && seg::block_of(3, 96, 5).bytes == 320);
        CHECK(seg::block_of(1, 88, 14).bytes == 128 && seg::block_of(1, 88, 15).bytes == 128 && seg::block_of(1, 88, 17).bytes == 192);
        // a chunk: whole, the rest, nothing at k mss == total and behind; mss == 0: everything, for any k
        CHECK(seg::chunk_at(1000, 100, 0) == 100 && seg::chunk_at(1000, 100, 9) == 100 && seg::chunk_at(1000, 100, 10) == 0);
        CHECK(seg::chunk_at(1001, 100, 10) == 1 && seg::chunk_at(1001, 100, 11) == 0 && seg::chunk_at(0, 100, 0) == 0);
        CHECK(seg::chunk_at(1000, 0, 0) == 1000 && seg::chunk_at(1000, 0, 7) == 1000 && seg::chunk_at(0, 0, 0) == 0);
        CHECK(seg::chunk_at(0xFFFFFFFFu, 65535, 65536) == 65535 && seg::chunk_at(0xFFFFFFFFu, 65535, 65537) == 0);
        // the staged ID powers: ceil(frames / 64) entries from id_at on, and rec_id walks from them
        for (uint32_t frames : {1u, 63u, 64u, 65u, 128u, 129u, 4096u}) {
            std::vector<uint16_t> ids(2 + (frames + 63) / 64 + 1, 0xEEEE);
            const uint64_t end = seg::stage_ids(0xBEEF, frames, ids.data(), 2);
            CHECK(end == 2 + (frames + 63) / 64 && ids[0] == 0xEEEE && ids[1] == 0xEEEE && ids[end] == 0xEEEE);
            seg::SendRec r{};
            r.id_at = 2;
            uint16_t id = 0xBEEF;
            for (uint32_t k = 0; k < frames; ++k, id = seg::prand16(id)) CHECK(seg::rec_id(r, ids.data(), k) == id);
        }
        uint16_t none = 0xEEEE;
        CHECK(seg::stage_ids(1, 0, &none, 0) == 0 && none == 0xEEEE);
    }
    std::puts("segment checks OK");
    return 0;
}
