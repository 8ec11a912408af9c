// Host-side arithmetic of the TX frame build (fs_segment_layout / fs_segment_batch), free of HIP
// so that it compiles on its own, like framesum_plan.h and framesum_choice.h: the validation of a
// send, the frames a send makes, the prefix of frame indices and byte bases per send, the map from
// a frame index back to (send, k), and the block of per-send records a call stages for the kernel
// (the kernel reads exactly these structs). The ring send's arithmetic (framesum_send.h) takes the
// chunk of a byte count, the block's layout and the staged ID powers from here.
// tests/csrc/test_segment.cpp builds it alone under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/framesum.h"

// The arithmetic the device plan of the resident ring send (framesum_send_resident.hip) runs too is
// marked FS_HD: callable from device code in a HIP translation unit, plain inline functions elsewhere.
#if defined(__HIP__)
#define FS_HD __host__ __device__
#else
#define FS_HD
#endif

namespace framesum {
namespace segment {

constexpr uint32_t kTcpHdr = 54, kUdpHdr = 42;  // Ethernet 14 + IPv4 20 + TCP 20 / UDP 8
// the largest chunk whose IPv4 TotalLength (20 + 20 or 8 + chunk) still fits 16 bits
constexpr uint32_t kMaxTcpChunk = 65495, kMaxUdpChunk = 65507;
constexpr uint64_t kMaxFrames = 1ull << 31;  // frame indices are 32-bit in the kernel
constexpr uint32_t kIdStride = 64;           // every 64th power of prand16 is staged per send (Prand16Stride)
constexpr uint32_t kLanes = 64;              // probes per round of the kernel's frame -> send search

// The reference's IPv4 ID generator (stacks/port_tcp.go:197-203), stepped once per CalculateHeaders.
constexpr uint16_t prand16(uint16_t x) {
    x = (uint16_t)(x ^ (uint16_t)(x << 7));
    x = (uint16_t)(x ^ (uint16_t)(x >> 9));
    x = (uint16_t)(x ^ (uint16_t)(x << 8));
    return x;
}
static_assert(prand16(1) == 0x8181, "prand16");

// kIdStride steps at once: prand16 is linear over GF(2) (XORs of shifts), so its 64th power is the
// XOR of the images of x's bits.
struct Prand16Stride {
    uint16_t image[16] = {};
    constexpr Prand16Stride() {
        for (int b = 0; b < 16; ++b) {
            uint16_t v = (uint16_t)(1u << b);
            for (uint32_t i = 0; i < kIdStride; ++i) v = prand16(v);
            image[b] = v;
        }
    }
};
FS_HD inline uint16_t prand16_stride(uint16_t x) {
    constexpr Prand16Stride t;  // (16 constants: the same on the host and in a kernel)
    uint16_t r = 0;
    for (int b = 0; b < 16; ++b)
        if ((x >> b) & 1u) r = (uint16_t)(r ^ t.image[b]);
    return r;
}

constexpr bool valid_align(uint32_t a) { return a >= 1 && a <= 4096 && (a & (a - 1)) == 0; }
constexpr bool valid_flags(uint32_t f) { return (f & ~(uint32_t)FS_FCS_APPEND) == 0; }
// bytes of `frames` one frame of `len` bytes owns
constexpr uint64_t slot_bytes(uint32_t len, uint32_t flags, uint32_t align) {
    return ((uint64_t)len + ((flags & FS_FCS_APPEND) ? 4u : 0u) + (align - 1)) & ~(uint64_t)(align - 1);
}

inline bool is_udp(const fs_tx_send& s) { return s.hdr[23] == 17; }
inline uint32_t hdr_len(const fs_tx_send& s) { return is_udp(s) ? kUdpHdr : kTcpHdr; }
// frames a (valid) send makes, and the payload bytes frame k carries
inline uint32_t frames_of(const fs_tx_send& s) {
    if (s.mss == 0 || s.payload_len == 0) return 1;
    return (uint32_t)(((uint64_t)s.payload_len + s.mss - 1) / s.mss);
}
// bytes [k mss, (k + 1) mss) of `total` (none behind its end); mss == 0: all of them
FS_HD inline uint32_t chunk_at(uint32_t total, uint32_t mss, uint32_t k) {
    if (mss == 0) return total;
    const uint64_t lo = (uint64_t)k * mss;
    return lo >= total ? 0u : (uint32_t)(total - lo < mss ? total - lo : mss);
}
inline uint32_t chunk_of(const fs_tx_send& s, uint32_t k) { return chunk_at(s.payload_len, s.mss, k); }

enum Bad : int {
    kGood = 0,
    kBadReserved,
    kBadEtherType,
    kBadIhl,
    kBadProto,
    kBadDataOffset,
    kBadUdpMss,
    kBadChunk,
    kBadFrameCount,
    kBadPayloadRange,
    kBadTotalFrames,
};
inline const char* bad_text(Bad b) {
    switch (b) {
    case kGood: return "valid";
    case kBadReserved: return "reserved is not 0";
    case kBadEtherType: return "EtherType is not 0x0800";
    case kBadIhl: return "IPv4 IHL is not 5";
    case kBadProto: return "IPv4 protocol is neither TCP (6) nor UDP (17)";
    case kBadDataOffset: return "TCP data offset is not 5";
    case kBadUdpMss: return "a UDP send has mss != 0";
    case kBadChunk: return "a frame's payload exceeds what IPv4 TotalLength can hold";
    case kBadFrameCount: return "more than FS_SEGMENT_MAX_FRAMES frames";
    case kBadPayloadRange: return "payload range outside payload_bytes";
    case kBadTotalFrames: return "more than 2^31 frames in the batch";
    }
    return "?";
}

// One send's checks. `payload_bytes` < 0 in the sense of have_payload == false: fs_segment_layout
// has no payload to bound the range with.
inline Bad check_send(const fs_tx_send& s, bool have_payload, uint64_t payload_bytes) {
    if (s.reserved != 0) return kBadReserved;
    if (s.hdr[12] != 0x08 || s.hdr[13] != 0x00) return kBadEtherType;
    if ((s.hdr[14] & 0x0F) != 5) return kBadIhl;
    if (s.hdr[23] != 6 && s.hdr[23] != 17) return kBadProto;
    const bool udp = is_udp(s);
    if (!udp && (s.hdr[46] >> 4) != 5) return kBadDataOffset;
    if (udp && s.mss != 0) return kBadUdpMss;
    const uint32_t chunk = s.mss == 0 || s.payload_len < s.mss ? s.payload_len : s.mss;
    if (chunk > (udp ? kMaxUdpChunk : kMaxTcpChunk)) return kBadChunk;
    if (s.mss != 0 && ((uint64_t)s.payload_len + s.mss - 1) / s.mss > FS_SEGMENT_MAX_FRAMES) return kBadFrameCount;
    if (have_payload && (s.payload_off > payload_bytes || s.payload_len > payload_bytes - s.payload_off))
        return kBadPayloadRange;
    return kGood;
}

// bytes of `frames` a (valid) send's S frames own: S - 1 full frames and the last one
inline uint64_t send_bytes(const fs_tx_send& s, uint32_t flags, uint32_t align) {
    const uint32_t S = frames_of(s), h = hdr_len(s);
    return (uint64_t)(S - 1) * slot_bytes(h + s.mss, flags, align) + slot_bytes(h + chunk_of(s, S - 1), flags, align);
}

struct Layout {
    Bad bad = kGood;
    uint32_t bad_send = 0;      // the first invalid send (when bad != kGood)
    uint64_t n_frames = 0;
    uint64_t frames_bytes = 0;  // the sum of the slots
    uint64_t written = 0;       // the frame and FCS bytes among them (== frames_bytes: no gaps)
    uint64_t payload = 0;       // payload bytes the sends carry
    uint64_t id_entries = 0;    // staged ID powers: the sum of ceil(S / kIdStride)
};
inline Layout layout(const fs_tx_send* sends, uint32_t n_sends, uint32_t flags, uint32_t align, bool have_payload,
                     uint64_t payload_bytes) {
    Layout L;
    const uint32_t fcs = (flags & FS_FCS_APPEND) ? 4u : 0u;
    for (uint32_t i = 0; i < n_sends; ++i) {
        const fs_tx_send& s = sends[i];
        L.bad = check_send(s, have_payload, payload_bytes);
        if (L.bad == kGood && L.n_frames + frames_of(s) > kMaxFrames) L.bad = kBadTotalFrames;
        if (L.bad != kGood) {
            L.bad_send = i;
            return L;
        }
        const uint32_t S = frames_of(s);
        L.n_frames += S;
        L.frames_bytes += send_bytes(s, flags, align);
        L.written += (uint64_t)S * (hdr_len(s) + fcs) + s.payload_len;
        L.payload += s.payload_len;
        L.id_entries += (S + kIdStride - 1) / kIdStride;
    }
    return L;
}

// ---------------------------------------------------------------------------------------
// What a call stages for its kernel, in one block: n_sends records, the prefix of frame indices
// (n_sends + 1 entries: prefix[i] = send i's first frame, prefix[n_sends] = n_frames) and the ID
// powers. No per-frame array crosses PCIe: the kernel finds a frame's send in the prefix.
struct SendRec {
    uint8_t hdr[54];
    uint16_t mss;
    uint64_t payload_off;
    uint32_t payload_len;
    uint32_t frames;      // S
    uint64_t frame_base;  // byte offset of the send's first frame in `frames`
    uint32_t id_at;       // index of the send's first staged ID power
    uint32_t pad;
};
static_assert(sizeof(SendRec) == 88 && offsetof(SendRec, payload_off) == 56 && offsetof(SendRec, frame_base) == 72,
              "SendRec layout (the kernel reads it)");
static_assert(sizeof(fs_tx_send) == 72 && offsetof(fs_tx_send, mss) == 54 && offsetof(fs_tx_send, payload_off) == 56 &&
                  offsetof(fs_tx_send, payload_len) == 64 && offsetof(fs_tx_send, reserved) == 68,
              "fs_tx_send is 72 bytes with no padding");

struct Block {
    uint64_t recs_at = 0, prefix_at = 0, ids_at = 0, bytes = 0;
};
// n_recs records of rec_bytes each: the layout of this call's block and of the ring send's
FS_HD inline Block block_of(uint32_t n_recs, uint64_t rec_bytes, uint64_t id_entries) {
    Block b;
    b.recs_at = 0;
    b.prefix_at = (uint64_t)n_recs * rec_bytes;
    b.ids_at = b.prefix_at + ((uint64_t)n_recs + 1) * 4;
    b.bytes = (b.ids_at + id_entries * 2 + 63) & ~63ull;
    return b;
}
inline Block block_of(uint32_t n_sends, uint64_t id_entries) { return block_of(n_sends, sizeof(SendRec), id_entries); }
// A record's staged ID powers, ceil(frames / kIdStride) of them from ids[id_at] on: the IDs of its
// frames 0, kIdStride, 2 kIdStride, ... Returns the index behind them.
FS_HD inline uint64_t stage_ids(uint16_t id, uint32_t frames, uint16_t* ids, uint64_t id_at) {
    for (uint32_t k = 0; k < frames; k += kIdStride) {
        ids[id_at++] = id;
        id = prand16_stride(id);
    }
    return id_at;
}
// Fill a block of block_of(...).bytes bytes at `dst` from a batch layout() found valid.
inline void stage(const fs_tx_send* sends, uint32_t n_sends, uint32_t flags, uint32_t align, const Block& b, uint8_t* dst) {
    SendRec* recs = reinterpret_cast<SendRec*>(dst + b.recs_at);
    uint32_t* prefix = reinterpret_cast<uint32_t*>(dst + b.prefix_at);
    uint16_t* ids = reinterpret_cast<uint16_t*>(dst + b.ids_at);
    uint64_t frame = 0, base = 0, id_at = 0;
    for (uint32_t i = 0; i < n_sends; ++i) {
        const fs_tx_send& s = sends[i];
        SendRec r;
        memset(&r, 0, sizeof r);
        memcpy(r.hdr, s.hdr, 54);
        r.mss = s.mss;
        r.payload_off = s.payload_off;
        r.payload_len = s.payload_len;
        r.frames = frames_of(s);
        r.frame_base = base;
        r.id_at = (uint32_t)id_at;
        memcpy(&recs[i], &r, sizeof r);
        prefix[i] = (uint32_t)frame;
        id_at = stage_ids((uint16_t)((s.hdr[18] << 8) | s.hdr[19]), r.frames, ids, id_at);
        frame += r.frames;
        base += send_bytes(s, flags, align);
    }
    prefix[n_sends] = (uint32_t)frame;
}

// Frame k of a staged send: its payload bytes, byte offset in `frames` and IPv4 ID.
inline uint32_t rec_chunk(const SendRec& r, uint32_t k) { return chunk_at(r.payload_len, r.mss, k); }
inline uint64_t rec_frame_offset(const SendRec& r, uint32_t k, uint32_t flags, uint32_t align) {
    const uint32_t h = r.hdr[23] == 17 ? kUdpHdr : kTcpHdr;
    return r.frame_base + (uint64_t)k * slot_bytes(h + r.mss, flags, align);  // frames before k are full ones
}
inline uint16_t rec_id(const SendRec& r, const uint16_t* ids, uint32_t k) {
    uint16_t id = ids[r.id_at + k / kIdStride];
    for (uint32_t j = 0; j < k % kIdStride; ++j) id = prand16(id);
    return id;
}

// frame index -> send: the largest s with prefix[s] <= frame (frame < prefix[n_sends]). The kernel
// runs this same search with one probe per lane: each round cuts [lo, hi) into kLanes steps and
// keeps the step whose first entry is the last one <= frame. Every send has at least one frame, so
// the prefix is strictly increasing.
inline uint32_t find_send(const uint32_t* prefix, uint32_t n_sends, uint32_t frame) {
    uint32_t lo = 0, hi = n_sends;
    while (hi - lo > 1) {
        const uint32_t step = (hi - lo + kLanes - 1) / kLanes;
        uint32_t cnt = 0;
        for (uint32_t l = 0; l < kLanes; ++l) {
            const uint64_t idx = (uint64_t)lo + (uint64_t)l * step;
            if (idx < hi && prefix[idx] <= frame) ++cnt;
        }
        lo += (cnt - 1) * step;
        hi = hi - lo < step ? hi : lo + step;
    }
    return lo;
}

// Frames a wave builds back to back before it looks its next frame's send up again: enough that
// the lookups are few, few enough that a small batch still spreads over the waves.
FS_HD inline uint32_t tile_frames(uint64_t n_frames, uint32_t waves) {
    const uint64_t t = (n_frames + waves - 1) / (waves ? waves : 1);
    return t < 1 ? 1u : t > 16 ? 16u : (uint32_t)t;
}

}  // namespace segment
}  // namespace framesum
