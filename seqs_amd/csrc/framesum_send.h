// Host-side arithmetic of the ring send (fs_send_rings_layout / fs_send_rings_batch), free of HIP so
// that it compiles on its own, like framesum_segment.h and framesum_deliver.h: the checks of a socket,
// the per-socket rule (how much goes out, in how many frames, with which flags, and the state after),
// the layout, and the block of per-socket records a call stages for the kernel (framesum_send.hip
// reads exactly these structs). The slots, the chunks, the block's layout, the ID powers and the
// frame -> record search are the TX frame build's (framesum_segment.h). tests/csrc/test_send.cpp builds
// it alone under ASan + UBSan. The checks, the rule and the records are marked FS_HD: the plan kernels of
// the resident ring send (framesum_send_resident.h, framesum_send_resident.hip) run them per socket on
// the device, so the rule stays written once.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/framesum_send.h"
#include "framesum_segment.h"

namespace framesum {
namespace send {

constexpr uint32_t kSockFlags = FS_TX_ACK | FS_TX_FIN | FS_TX_PSH;
constexpr uint32_t kMaxRing = 1u << 31;
constexpr uint8_t kTcpFin = 0x01, kTcpPsh = 0x08, kTcpAck = 0x10;

static_assert(sizeof(fs_tx_sock) == 104 && offsetof(fs_tx_sock, mss) == 54 && offsetof(fs_tx_sock, ring_off) == 56 &&
                  offsetof(fs_tx_sock, ring_size) == 64 && offsetof(fs_tx_sock, snd_una) == 76 &&
                  offsetof(fs_tx_sock, rcv_nxt) == 88 && offsetof(fs_tx_sock, flags) == 100,
              "fs_tx_sock is 104 bytes with no padding");
static_assert(sizeof(fs_tx_sock_out) == 32 && offsetof(fs_tx_sock_out, ip_id) == 24, "fs_tx_sock_out is 32 bytes");

enum Bad : int {
    kGood = 0,
    kBadEtherType,
    kBadIhl,
    kBadProto,
    kBadDataOffset,
    kBadMss,
    kBadSockFlags,
    kBadMaxFrames,
    kBadRingSize,
    kBadRingPos,
    kBadBuffered,
    kBadRingRange,
    kBadTotalFrames,
};
inline const char* bad_text(Bad b) {
    switch (b) {
    case kGood: return "valid";
    case kBadEtherType: return "EtherType is not 0x0800";
    case kBadIhl: return "IPv4 IHL is not 5";
    case kBadProto: return "IPv4 protocol is not TCP (6)";
    case kBadDataOffset: return "TCP data offset is not 5";
    case kBadMss: return "mss is 0 or above 65495";
    case kBadSockFlags: return "unknown bits in flags";
    case kBadMaxFrames: return "max_frames above FS_SEGMENT_MAX_FRAMES";
    case kBadRingSize: return "ring_size is 0 or above 2^31";
    case kBadRingPos: return "ring_rpos is not below ring_size";
    case kBadBuffered: return "ring_buffered above ring_size";
    case kBadRingRange: return "ring outside rings_bytes";
    case kBadTotalFrames: return "more than 2^31 frames in the batch";
    }
    return "?";
}

// One socket's checks. `have_rings` false: fs_send_rings_layout has no rings_bytes to bound the ring with.
FS_HD inline Bad check_sock(const fs_tx_sock& s, bool have_rings, uint64_t rings_bytes) {
    if (s.hdr[12] != 0x08 || s.hdr[13] != 0x00) return kBadEtherType;
    if ((s.hdr[14] & 0x0F) != 5) return kBadIhl;
    if (s.hdr[23] != 6) return kBadProto;
    if ((s.hdr[46] >> 4) != 5) return kBadDataOffset;
    if (s.mss == 0 || s.mss > segment::kMaxTcpChunk) return kBadMss;
    if (s.flags & ~kSockFlags) return kBadSockFlags;
    if (s.max_frames > FS_SEGMENT_MAX_FRAMES) return kBadMaxFrames;
    if (s.ring_size == 0 || s.ring_size > kMaxRing) return kBadRingSize;
    if (s.ring_rpos >= s.ring_size) return kBadRingPos;
    if (s.ring_buffered > s.ring_size) return kBadBuffered;
    if (have_rings && (s.ring_off > rings_bytes || s.ring_size > rings_bytes - s.ring_off)) return kBadRingRange;
    return kGood;
}

// ---------------------------------------------------------------------------------------
// The per-socket rule (include/framesum_send.h) for a socket check_sock found valid.
struct Plan {
    uint32_t data = 0;    // ring bytes that go out
    uint32_t frames = 0;  // S
    bool fin = false;
    uint8_t tcp_flags = 0;  // of the socket's LAST frame (the kernel clears FIN and PSH on the others)
};
FS_HD inline uint32_t room_of(const fs_tx_sock& s) {
    const uint32_t in_flight = s.snd_nxt - s.snd_una;
    return s.snd_wnd > in_flight ? s.snd_wnd - in_flight : 0u;  // (the reference panics when in_flight > snd_wnd)
}
FS_HD inline Plan plan_of(const fs_tx_sock& s) {
    Plan p;
    const uint32_t cap = (s.max_frames ? s.max_frames : FS_SEGMENT_MAX_FRAMES) * (uint32_t)s.mss;  // <= 4096 * 65495
    const uint32_t room = room_of(s);
    p.data = s.ring_buffered;
    if (room < p.data) p.data = room;
    if (cap < p.data) p.data = cap;
    p.fin = (s.flags & FS_TX_FIN) && p.data == s.ring_buffered;
    p.frames = (p.data + s.mss - 1u) / s.mss;
    if (p.frames == 0 && (p.fin || (s.flags & FS_TX_ACK))) p.frames = 1;
    p.tcp_flags = (uint8_t)(kTcpAck | ((s.flags & FS_TX_PSH) && p.data ? kTcpPsh : 0) | (p.fin ? kTcpFin : 0));
    return p;
}
FS_HD inline uint32_t chunk_of(const fs_tx_sock& s, const Plan& p, uint32_t k) { return segment::chunk_at(p.data, s.mss, k); }
// prand16 applied n times (n <= FS_SEGMENT_MAX_FRAMES): kIdStride steps at once, then the rest
FS_HD inline uint16_t advance_id(uint16_t id, uint32_t n) {
    for (; n >= segment::kIdStride; n -= segment::kIdStride) id = segment::prand16_stride(id);
    for (; n > 0; --n) id = segment::prand16(id);
    return id;
}
FS_HD inline uint16_t template_id(const fs_tx_sock& s) { return (uint16_t)((s.hdr[18] << 8) | s.hdr[19]); }
FS_HD inline fs_tx_sock_out out_of(const fs_tx_sock& s, const Plan& p, uint64_t first_frame) {
    fs_tx_sock_out o;
    o.snd_nxt = s.snd_nxt + p.data + (p.fin ? 1u : 0u);
    o.ring_rpos = (uint32_t)(((uint64_t)s.ring_rpos + p.data) % s.ring_size);
    o.ring_buffered = s.ring_buffered - p.data;
    o.bytes = p.data;
    o.n_frames = p.frames;
    o.first_frame = p.frames ? (uint32_t)first_frame : FS_SEND_NONE;
    o.ip_id = advance_id(template_id(s), p.frames);
    o.sent = p.fin ? FS_TX_FIN : (p.frames && p.data == 0 ? FS_TX_ACK : 0u);
    return o;
}
// bytes of `frames` a socket's S > 0 frames own: S - 1 full frames and the last one
FS_HD inline uint64_t sock_bytes(const fs_tx_sock& s, const Plan& p, uint32_t flags, uint32_t align) {
    return (uint64_t)(p.frames - 1) * segment::slot_bytes(segment::kTcpHdr + s.mss, flags, align) +
           segment::slot_bytes(segment::kTcpHdr + chunk_of(s, p, p.frames - 1), flags, align);
}

struct Layout {
    Bad bad = kGood;
    uint32_t bad_sock = 0;      // the first invalid socket (when bad != kGood)
    uint64_t n_frames = 0;
    uint64_t frames_bytes = 0;  // the sum of the slots
    uint64_t written = 0;       // the frame and FCS bytes among them
    uint64_t data = 0;          // ring bytes the frames carry
    uint32_t n_recs = 0;        // sockets with S > 0: the records staged
    uint64_t id_entries = 0;    // staged ID powers: the sum of ceil(S / kIdStride)
    uint64_t read_lo = 0, read_hi = 0;  // the span of `rings` the call reads (empty when data == 0)
};
// The checks, the totals and (socks_out not null) every socket's record, in one pass.
inline Layout layout(const fs_tx_sock* socks, uint32_t n_socks, uint32_t flags, uint32_t align, bool have_rings,
                     uint64_t rings_bytes, fs_tx_sock_out* socks_out) {
    Layout L;
    const uint32_t fcs = (flags & FS_FCS_APPEND) ? 4u : 0u;
    uint64_t lo = UINT64_MAX, hi = 0;
    for (uint32_t i = 0; i < n_socks; ++i) {
        const fs_tx_sock& s = socks[i];
        L.bad = check_sock(s, have_rings, rings_bytes);
        const Plan p = L.bad == kGood ? plan_of(s) : Plan();
        if (L.bad == kGood && L.n_frames + p.frames > segment::kMaxFrames) L.bad = kBadTotalFrames;
        if (L.bad != kGood) {
            L.bad_sock = i;
            return L;
        }
        if (socks_out) socks_out[i] = out_of(s, p, L.n_frames);
        if (p.frames == 0) continue;
        L.n_frames += p.frames;
        L.frames_bytes += sock_bytes(s, p, flags, align);
        L.written += (uint64_t)p.frames * (segment::kTcpHdr + fcs) + p.data;
        L.data += p.data;
        L.n_recs += 1;
        L.id_entries += (p.frames + segment::kIdStride - 1) / segment::kIdStride;
        if (p.data) {  // the sent range, or the whole ring when it wraps
            const bool wraps = p.data > s.ring_size - s.ring_rpos;
            const uint64_t a = s.ring_off + (wraps ? 0u : s.ring_rpos);
            const uint64_t b = wraps ? s.ring_off + s.ring_size : a + p.data;
            lo = a < lo ? a : lo;
            hi = b > hi ? b : hi;
        }
    }
    if (hi > lo) L.read_lo = lo, L.read_hi = hi;
    return L;
}

// ---------------------------------------------------------------------------------------
// What a call stages for its kernel, in one block laid out as the TX frame build's (segment::Block):
// one record per socket with S > 0, so that the prefix of frame indices is strictly increasing as
// segment::find_send needs it, the prefix (n_recs + 1 entries) and the ID powers. Seq, Ack, Window and
// the flags are already in the record's header: the kernel varies per frame what the TX frame build
// varies (Seq + k mss, FIN and PSH on the last frame only, ID, lengths, checksums).
struct RingRec {
    uint8_t hdr[54];
    uint16_t mss;
    uint64_t ring_off;
    uint32_t data;
    uint32_t frames;      // S
    uint64_t frame_base;  // byte offset of the socket's first frame in `frames`
    uint32_t id_at;       // index of the socket's first staged ID power
    uint32_t ring_size;
    uint32_t ring_rpos;
    uint32_t pad;
};
static_assert(sizeof(RingRec) == 96 && offsetof(RingRec, ring_off) == 56 && offsetof(RingRec, frame_base) == 72 &&
                  offsetof(RingRec, ring_size) == 84,
              "RingRec layout (the kernel reads it)");
// What the frame body both kernels share (framesum_tx_dev.h) reads of a record lies where
// segment::SendRec has it: the header, mss, the byte offset, the byte count, frames, frame_base, id_at.
static_assert(offsetof(RingRec, hdr) == offsetof(segment::SendRec, hdr) &&
                  offsetof(RingRec, mss) == offsetof(segment::SendRec, mss) &&
                  offsetof(RingRec, ring_off) == offsetof(segment::SendRec, payload_off) &&
                  offsetof(RingRec, data) == offsetof(segment::SendRec, payload_len) &&
                  offsetof(RingRec, frames) == offsetof(segment::SendRec, frames) &&
                  offsetof(RingRec, frame_base) == offsetof(segment::SendRec, frame_base) &&
                  offsetof(RingRec, id_at) == offsetof(segment::SendRec, id_at),
              "RingRec and SendRec agree in what the shared frame body reads");

FS_HD inline segment::Block block_of(uint32_t n_recs, uint64_t id_entries) {
    return segment::block_of(n_recs, sizeof(RingRec), id_entries);
}

FS_HD inline void put32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}
// The header of a socket's frames as the kernel takes it: the template with Seq, Ack, the flags of the
// last frame and the window.
FS_HD inline void put_state(const fs_tx_sock& s, const Plan& p, uint8_t hdr[54]) {
    memcpy(hdr, s.hdr, 54);
    put32(hdr + 38, s.snd_nxt);
    put32(hdr + 42, s.rcv_nxt);
    hdr[47] = p.tcp_flags;
    const uint32_t wnd = s.rcv_wnd > 65535u ? 65535u : s.rcv_wnd;  // (the reference: uint16(rcv.WND))
    hdr[48] = (uint8_t)(wnd >> 8);
    hdr[49] = (uint8_t)wnd;
}
// Fill a block of block_of(L.n_recs, L.id_entries).bytes bytes at `dst` from a batch layout() found valid.
inline void stage(const fs_tx_sock* socks, uint32_t n_socks, uint32_t flags, uint32_t align, const segment::Block& b,
                  uint8_t* dst) {
    RingRec* recs = reinterpret_cast<RingRec*>(dst + b.recs_at);
    uint32_t* prefix = reinterpret_cast<uint32_t*>(dst + b.prefix_at);
    uint16_t* ids = reinterpret_cast<uint16_t*>(dst + b.ids_at);
    uint64_t frame = 0, base = 0, id_at = 0;
    uint32_t n = 0;
    for (uint32_t i = 0; i < n_socks; ++i) {
        const fs_tx_sock& s = socks[i];
        const Plan p = plan_of(s);
        if (p.frames == 0) continue;
        RingRec r;
        memset(&r, 0, sizeof r);
        put_state(s, p, r.hdr);
        r.mss = s.mss;
        r.ring_off = s.ring_off;
        r.data = p.data;
        r.frames = p.frames;
        r.frame_base = base;
        r.id_at = (uint32_t)id_at;
        r.ring_size = s.ring_size;
        r.ring_rpos = s.ring_rpos;
        memcpy(&recs[n], &r, sizeof r);
        prefix[n++] = (uint32_t)frame;
        id_at = segment::stage_ids(template_id(s), p.frames, ids, id_at);
        frame += p.frames;
        base += sock_bytes(s, p, flags, align);
    }
    prefix[n] = (uint32_t)frame;
}

// Where frame k of a staged record reads: its chunk, the ring position of the chunk's first byte and
// the chunk bytes that lie before the ring's end (>= chunk: the chunk does not wrap).
inline uint32_t rec_chunk(const RingRec& r, uint32_t k) { return segment::chunk_at(r.data, r.mss, k); }
inline uint32_t rec_pos(const RingRec& r, uint32_t k) {
    return (uint32_t)(((uint64_t)r.ring_rpos + (uint64_t)k * r.mss) % r.ring_size);
}
inline uint32_t rec_before_wrap(const RingRec& r, uint32_t k) { return r.ring_size - rec_pos(r, k); }

}  // namespace send
}  // namespace framesum
