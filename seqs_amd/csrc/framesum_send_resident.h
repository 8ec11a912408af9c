// Arithmetic of the resident ring send (fs_send_rings_resident, include/framesum_send_resident.h), free
// of HIP so that it compiles on its own like framesum_send.h, whose checks, rule, records and block it
// uses unchanged: what one socket contributes to the scans (plan_sock), what the call writes for one
// socket once the scans are known (write_sock), the capacity cut, the totals, and the layout of the
// call's scratch. The plan kernels (framesum_send_resident.hip) run exactly these functions, one lane
// per socket; tests/csrc/test_send_resident.cpp runs them on the host, in index order and cut into chunks
// as the kernels do, and compares what they leave with send::layout and send::stage under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/framesum_send_resident.h"
#include "framesum_send.h"

namespace framesum {
namespace resident {

constexpr uint32_t kChunk = 256;  // sockets per scan chunk: one lane each of a plan workgroup
constexpr uint32_t kMaxChunks = (FS_SEND_MAX_SOCKS + kChunk - 1) / kChunk;  // 256: one lane each of the middle kernel
constexpr uint32_t kCallFlags = FS_FCS_APPEND | FS_TX_WRITEBACK;
constexpr uint64_t kMaxFramesCap = 1ull << 31;

static_assert(sizeof(fs_tx_totals) == 40 && offsetof(fs_tx_totals, n_built) == 24, "fs_tx_totals is 40 bytes with no padding");
static_assert(sizeof(fs_rx_sock_out) == 32 && sizeof(fs_rx_snd_out) == 32, "the RX records the hand-off reads");
static_assert(FS_TX_BAD_ETHERTYPE == send::kBadEtherType && FS_TX_BAD_IHL == send::kBadIhl &&
                  FS_TX_BAD_PROTO == send::kBadProto && FS_TX_BAD_DATA_OFFSET == send::kBadDataOffset &&
                  FS_TX_BAD_MSS == send::kBadMss && FS_TX_BAD_SOCK_FLAGS == send::kBadSockFlags &&
                  FS_TX_BAD_MAX_FRAMES == send::kBadMaxFrames && FS_TX_BAD_RING_SIZE == send::kBadRingSize &&
                  FS_TX_BAD_RING_POS == send::kBadRingPos && FS_TX_BAD_BUFFERED == send::kBadBuffered &&
                  FS_TX_BAD_RING_RANGE == send::kBadRingRange,
              "the FS_TX_BAD_* reasons are check_sock's, in its order");
static_assert((FS_TX_DEFERRED & send::kSockFlags) == 0 && (FS_TX_INVALID & send::kSockFlags) == 0 &&
                  (FS_TX_WRITEBACK & FS_FCS_APPEND) == 0,
              "the new bits are free");

// What the plan reads and writes of a call: every pointer is device memory.
struct Call {
    fs_tx_sock* socks;
    const fs_rx_sock_out* rx_socks_out;
    const fs_rx_snd_out* rx_snd_out;
    const uint32_t* rx_index;
    fs_tx_sock_out* socks_out;
    fs_tx_totals* totals;
    uint64_t rings_bytes, frames_bytes;
    uint32_t n_socks, n_rx, frames_cap, flags, align;
    uint32_t grid_waves;  // the waves of the frame kernel's grid: the tile follows from them
};

// One socket as the scans see it: the record behind the hand-off, why it is invalid (0: valid), the rule,
// and what it adds to the four scans.
struct SockPlan {
    fs_tx_sock s;
    send::Plan p;
    uint32_t reason;  // FS_TX_BAD_*
    bool handed;      // an RX record was applied
    uint64_t bytes;   // send::sock_bytes (0 when S == 0)
    uint32_t ids;     // ceil(S / kIdStride)
};
FS_HD inline SockPlan plan_sock(const Call& c, uint32_t i) {
    SockPlan q;
    q.s = c.socks[i];
    q.reason = 0;
    q.handed = false;
    q.bytes = 0;
    q.ids = 0;
    if (c.rx_socks_out) {  // step 1, the hand-off: tx_sock_from
        const uint32_t r = c.rx_index ? c.rx_index[i] : i;
        if (r != FS_TX_NO_RX) {
            if (r >= c.n_rx) {
                q.reason = FS_TX_BAD_RX_INDEX;
            } else {
                q.handed = true;
                q.s.rcv_nxt = c.rx_socks_out[r].rcv_nxt;
                q.s.rcv_wnd = c.rx_socks_out[r].ring_free;
                if (c.rx_snd_out) {
                    q.s.snd_una = c.rx_snd_out[r].snd_una;
                    q.s.snd_wnd = c.rx_snd_out[r].snd_wnd;
                    if (c.rx_snd_out[r].flags & FS_RECV_ACK_OWED) q.s.flags |= FS_TX_ACK;
                }
            }
        }
    }
    if (q.reason == 0) q.reason = (uint32_t)send::check_sock(q.s, true, c.rings_bytes);  // step 2
    if (q.reason != 0) {
        q.p = send::Plan();
        q.handed = false;
        q.s = c.socks[i];  // an invalid socket reports its own state
        return q;
    }
    q.p = send::plan_of(q.s);  // step 3
    if (q.p.frames) {
        q.bytes = send::sock_bytes(q.s, q.p, c.flags & FS_FCS_APPEND, c.align);
        q.ids = (q.p.frames + segment::kIdStride - 1) / segment::kIdStride;
    }
    return q;
}

// The sums of the scans, over a range of sockets.
struct Sums {
    uint64_t frames = 0, bytes = 0, data = 0, ids = 0;
    uint32_t recs = 0, idle = 0, invalid = 0, pad = 0;
};
static_assert(sizeof(Sums) == 48, "Sums is 48 bytes (the kernels keep one per chunk)");
FS_HD inline Sums sums_of(const SockPlan& q) {
    Sums s;
    s.frames = q.p.frames;
    s.bytes = q.bytes;
    s.data = q.p.data;
    s.ids = q.ids;
    s.recs = q.p.frames ? 1u : 0u;
    s.idle = q.reason == 0 && q.p.frames == 0 ? 1u : 0u;
    s.invalid = q.reason != 0 ? 1u : 0u;
    return s;
}
FS_HD inline Sums add(const Sums& a, const Sums& b) {
    Sums s;
    s.frames = a.frames + b.frames;
    s.bytes = a.bytes + b.bytes;
    s.data = a.data + b.data;
    s.ids = a.ids + b.ids;
    s.recs = a.recs + b.recs;
    s.idle = a.idle + b.idle;
    s.invalid = a.invalid + b.invalid;
    return s;
}
// Step 4 for one socket with frames: does it still fit, `incl` being the sums over the sockets 0..i?
FS_HD inline bool fits(const Call& c, const Sums& incl) { return incl.frames <= c.frames_cap && incl.bytes <= c.frames_bytes; }

// What the middle kernel leaves for the writing kernel and the frame kernel: the cut (the first socket
// with frames that does not fit; n_socks when all fit), the built counts, and where the three arrays of
// send::stage's block lie behind the scratch's `block`.
struct Head {
    uint32_t cut, n_recs, n_frames, tile;
    uint64_t recs_at, prefix_at, ids_at, block_bytes;
};
static_assert(sizeof(Head) == 48, "Head is 48 bytes");
// `built`: the sums over the sockets before the cut; `all`: over every socket.
FS_HD inline Head head_of(const Call& c, uint32_t cut, const Sums& built) {
    Head h;
    const segment::Block b = send::block_of(built.recs, built.ids);
    h.cut = cut;
    h.n_recs = built.recs;
    h.n_frames = (uint32_t)built.frames;
    h.tile = segment::tile_frames(built.frames, c.grid_waves);
    h.recs_at = b.recs_at;
    h.prefix_at = b.prefix_at;
    h.ids_at = b.ids_at;
    h.block_bytes = b.bytes;
    return h;
}
FS_HD inline fs_tx_totals totals_of(const Sums& built, const Sums& all) {
    fs_tx_totals t;
    t.n_frames = built.frames;
    t.frames_bytes = built.bytes;
    t.data_bytes = built.data;
    t.n_built = built.recs;
    t.n_idle = all.idle;
    t.n_deferred = all.recs - built.recs;
    t.n_invalid = all.invalid;
    return t;
}

// Everything the call writes for socket i: its socks_out record; when it is built, its record, prefix
// entry and ID powers in the block at `block` (laid out as `h` says); with FS_TX_WRITEBACK its state in
// `socks`. `excl`: the sums over the sockets before i.
FS_HD inline void write_sock(const Call& c, const Head& h, uint8_t* block, uint32_t i, const SockPlan& q, const Sums& excl) {
    fs_tx_sock_out o;
    const bool built = q.p.frames != 0 && i < h.cut;
    if (built) {
        o = send::out_of(q.s, q.p, excl.frames);
    } else {  // idle, deferred, invalid: the state as it is (no arithmetic on an invalid socket's fields)
        o.snd_nxt = q.s.snd_nxt;
        o.ring_rpos = q.s.ring_rpos;
        o.ring_buffered = q.s.ring_buffered;
        o.bytes = 0;
        o.n_frames = 0;
        o.first_frame = FS_SEND_NONE;
        o.ip_id = send::template_id(q.s);
        o.sent = q.reason ? FS_TX_INVALID | (q.reason << 16) : q.p.frames ? FS_TX_DEFERRED : 0u;
    }
    c.socks_out[i] = o;
    if (built) {
        send::RingRec r;
        memset(&r, 0, sizeof r);
        send::put_state(q.s, q.p, r.hdr);
        r.mss = q.s.mss;
        r.ring_off = q.s.ring_off;
        r.data = q.p.data;
        r.frames = q.p.frames;
        r.frame_base = excl.bytes;
        r.id_at = (uint32_t)excl.ids;
        r.ring_size = q.s.ring_size;
        r.ring_rpos = q.s.ring_rpos;
        memcpy(block + h.recs_at + (uint64_t)excl.recs * sizeof r, &r, sizeof r);
        reinterpret_cast<uint32_t*>(block + h.prefix_at)[excl.recs] = (uint32_t)excl.frames;
        segment::stage_ids(send::template_id(q.s), q.p.frames, reinterpret_cast<uint16_t*>(block + h.ids_at), excl.ids);
    }
    if ((c.flags & FS_TX_WRITEBACK) && q.reason == 0) {
        fs_tx_sock& t = c.socks[i];
        if (q.handed) {
            t.rcv_nxt = q.s.rcv_nxt;
            t.rcv_wnd = q.s.rcv_wnd;
            if (c.rx_snd_out) {
                t.snd_una = q.s.snd_una;
                t.snd_wnd = q.s.snd_wnd;
            }
        }
        uint32_t flags = q.s.flags;  // (with the hand-off's FS_TX_ACK: a deferred socket keeps it)
        if (built) {
            t.snd_nxt = o.snd_nxt;
            t.ring_rpos = o.ring_rpos;
            t.ring_buffered = o.ring_buffered;
            t.hdr[18] = (uint8_t)(o.ip_id >> 8);
            t.hdr[19] = (uint8_t)o.ip_id;
            flags &= ~(FS_TX_ACK | (o.sent & FS_TX_FIN));
        }
        if (flags != t.flags) t.flags = flags;
    }
}
// The one entry behind the last record's: the prefix ends with the frame count.
FS_HD inline void write_prefix_end(const Head& h, uint8_t* block) {
    reinterpret_cast<uint32_t*>(block + h.prefix_at)[h.n_recs] = h.n_frames;
}

// The scratch of a call: the per-chunk sums, their exclusive prefix, the head, then the block, which is
// as large as the built sockets of a call with this n_socks and frames_cap can make it (every record has
// a frame, a record has at most FS_SEGMENT_MAX_FRAMES / kIdStride ID powers).
struct Scratch {
    uint64_t chunk_sums, chunk_base, head, block, block_cap, bytes;
};
inline Scratch scratch_of(uint32_t n_socks, uint32_t frames_cap) {
    Scratch s;
    const uint64_t chunks = ((uint64_t)n_socks + kChunk - 1) / kChunk;
    const uint32_t recs = n_socks < frames_cap ? n_socks : frames_cap;
    const uint64_t per_rec = (uint64_t)recs * (FS_SEGMENT_MAX_FRAMES / segment::kIdStride);
    const uint64_t by_frames = (uint64_t)recs + frames_cap / segment::kIdStride;
    s.chunk_sums = 0;
    s.chunk_base = chunks * sizeof(Sums);
    s.head = s.chunk_base + chunks * sizeof(Sums);
    s.block = (s.head + sizeof(Head) + 63) & ~63ull;
    s.block_cap = send::block_of(recs, per_rec < by_frames ? per_rec : by_frames).bytes;
    s.bytes = s.block + s.block_cap;
    return s;
}

}  // namespace resident
}  // namespace framesum
