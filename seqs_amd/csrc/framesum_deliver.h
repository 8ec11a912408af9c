// Arithmetic of the in-order TCP delivery (fs_deliver_flows_batch, include/framesum_deliver.h), free
// of HIP like framesum_flows.h, on which it builds: the checks of the socket list (which build the
// socket table: flows::build_table, staged with the records), the
// admission rule of one segment and the split of a ring write at the wrap. framesum_deliver.hip runs
// exactly this code per frame, and tests/csrc/test_deliver.cpp builds it alone under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/framesum_deliver.h"
#include "framesum_flows.h"

namespace framesum {
namespace deliver {

using namespace flows;

constexpr uint32_t kNone = FS_DELIVER_NONE;
constexpr uint32_t kMaxSocks = FS_DELIVER_MAX_SOCKS;
constexpr uint32_t kMaxRing = 1u << 31;
constexpr uint32_t kAck = 0x10;

static_assert(sizeof(fs_rx_sock) == 48 && sizeof(fs_rx_sock_out) == 32, "fs_rx_sock / fs_rx_sock_out layout");

static_assert(kNone == kEmpty, "the socket table's empty slot (framesum_flows.h) is the ABI's \"none\"");

// ---- The checks of the socket list, none of which needs a device.
enum Bad {
    kGood = 0, kNullPointer, kTooManySocks, kKeyNotTcp, kReservedNotZero, kEqualKeys, kRingSize, kRingState,
    kRingOutside, kRingsOverlap,
};
inline const char* bad_text(Bad b) {
    switch (b) {
    case kNullPointer: return "null socks, rings or socks_out";
    case kTooManySocks: return "n_socks above 65,536";
    case kKeyNotTcp: return "key[0] must be 6 (TCP)";
    case kReservedNotZero: return "reserved must be 0";
    case kEqualKeys: return "its key equals an earlier socket's";
    case kRingSize: return "ring_size must be 1 .. 2^31";
    case kRingState: return "ring_wpos must be below ring_size and ring_free at most ring_size";
    case kRingOutside: return "its ring ends past rings_bytes";
    case kRingsOverlap: return "its ring overlaps another socket's";
    default: return "";
    }
}
struct Check {
    Bad bad;
    uint32_t sock;    // the socket `bad` is about
    uint64_t lo, hi;  // the span of `rings` the listed rings cover
};
// `table`: resized and filled for the staged block when the list is good.
inline Check check_socks(const fs_rx_sock* socks, uint32_t n_socks, bool have_rings, bool have_out, uint64_t rings_bytes,
                         uint32_t hash_mask, std::vector<uint32_t>& table) {
    Check c{kGood, 0u, 0u, 0u};
    if (n_socks == 0) return c;
    if (!socks || !have_rings || !have_out) return Check{kNullPointer, 0u, 0u, 0u};
    if (n_socks > kMaxSocks) return Check{kTooManySocks, 0u, 0u, 0u};
    c.lo = UINT64_MAX;
    for (uint32_t i = 0; i < n_socks; ++i) {
        const fs_rx_sock& s = socks[i];
        if (s.key[0] != 6) return Check{kKeyNotTcp, i, 0u, 0u};
        if (s.reserved[0] | s.reserved[1] | s.reserved[2]) return Check{kReservedNotZero, i, 0u, 0u};
        if (s.ring_size == 0 || s.ring_size > kMaxRing) return Check{kRingSize, i, 0u, 0u};
        if (s.ring_wpos >= s.ring_size || s.ring_free > s.ring_size) return Check{kRingState, i, 0u, 0u};
        if (s.ring_off > rings_bytes || s.ring_size > rings_bytes - s.ring_off) return Check{kRingOutside, i, 0u, 0u};
        c.lo = std::min(c.lo, s.ring_off);
        c.hi = std::max(c.hi, s.ring_off + s.ring_size);
    }
    table.resize(table_slots(n_socks));
    const uint32_t dup = build_table(socks, n_socks, hash_mask, table.data());
    if (dup != kNone) return Check{kEqualKeys, dup, 0u, 0u};
    std::vector<uint32_t> by_off(n_socks);
    for (uint32_t i = 0; i < n_socks; ++i) by_off[i] = i;
    std::sort(by_off.begin(), by_off.end(), [&](uint32_t a, uint32_t b) {
        return socks[a].ring_off != socks[b].ring_off ? socks[a].ring_off < socks[b].ring_off : a < b;
    });
    for (uint32_t k = 1; k < n_socks; ++k) {
        const fs_rx_sock& p = socks[by_off[k - 1]];
        if (p.ring_off + p.ring_size > socks[by_off[k]].ring_off) return Check{kRingsOverlap, by_off[k], 0u, 0u};
    }
    return c;
}

// The staged block of a call: the records, then the table.
struct Block {
    uint64_t table, bytes;
};
inline Block block_of(uint32_t n_socks) {
    Block b;
    b.table = (uint64_t)n_socks * sizeof(fs_rx_sock);
    b.bytes = b.table + 4ull * table_slots(n_socks);
    return b;
}

// ---- The admission rule (include/framesum_deliver.h) of one segment against a socket's state.
struct State {
    uint32_t nxt, wpos, free;
};
FS_CO_HD bool stops_walk(uint32_t tcp_flags) { return (tcp_flags & (kSyn | kRst)) != 0; }
FS_CO_HD bool considered(uint32_t len, uint32_t tcp_flags) { return len != 0 || (tcp_flags & kFin) != 0; }
// (b) and (c): what does not depend on the frames before
FS_CO_HD bool window_and_ack_ok(uint32_t len, uint32_t tcp_flags, uint32_t ack, uint32_t rcv_wnd, uint32_t snd_nxt) {
    const uint32_t fin = tcp_flags & kFin ? 1u : 0u;
    if (len + fin > rcv_wnd) return false;  // (len < 2^16: no wrap; a zero window admits nothing)
    // Ack - snd_nxt as a signed 32-bit difference: above 0 acknowledges unsent data
    if ((tcp_flags & kAck) && (ack - snd_nxt) - 1u < 0x7FFFFFFFu) return false;
    return true;
}
// (a) and (d): what does
FS_CO_HD bool in_order_and_fits(const State& st, uint32_t seq, uint32_t len) { return seq == st.nxt && len <= st.free; }
FS_CO_HD bool admitted(const State& st, uint32_t seq, uint32_t ack, uint32_t len, uint32_t tcp_flags, uint32_t rcv_wnd,
                       uint32_t snd_nxt) {
    return considered(len, tcp_flags) && !stops_walk(tcp_flags) &&
           window_and_ack_ok(len, tcp_flags, ack, rcv_wnd, snd_nxt) && in_order_and_fits(st, seq, len);
}
// The state behind an admitted segment (len <= free <= ring_size and wpos < ring_size <= 2^31: no wrap of the sum).
FS_CO_HD State advance(const State& st, uint32_t len, bool fin, uint32_t ring_size) {
    State n;
    const uint32_t end = st.wpos + len;
    n.wpos = end >= ring_size ? end - ring_size : end;
    n.free = st.free - len;
    n.nxt = st.nxt + len + (fin ? 1u : 0u);
    return n;
}

// A ring write of `len` bytes at wpos (stacks/ring.go:17-40): `first` bytes up to the ring's end, the
// `second` rest from the ring's start.
struct Split {
    uint32_t first, second;
};
FS_CO_HD Split split_at_wrap(uint32_t wpos, uint32_t len, uint32_t ring_size) {
    const uint32_t room = ring_size - wpos;
    Split s;
    s.first = len < room ? len : room;
    s.second = len - s.first;
    return s;
}

// The per-slot word the mark step leaves for the walk beside the slot's Seq: the payload length and
// what of the rule does not depend on the chain.
constexpr uint32_t kMkConsidered = 1u << 16, kMkFixedOk = 1u << 17, kMkStop = 1u << 18, kMkFin = 1u << 19;
FS_CO_HD uint32_t mark_word(uint32_t len, uint32_t tcp_flags, uint32_t ack, uint32_t rcv_wnd, uint32_t snd_nxt) {
    return (len & 0xFFFFu) | (considered(len, tcp_flags) ? kMkConsidered : 0u) |
           (window_and_ack_ok(len, tcp_flags, ack, rcv_wnd, snd_nxt) ? kMkFixedOk : 0u) |
           (stops_walk(tcp_flags) ? kMkStop : 0u) | ((tcp_flags & kFin) ? kMkFin : 0u);
}

// What socks_out[s] holds for a socket whose flow is not in the batch (and for every socket when n is 0).
FS_CO_HD fs_rx_sock_out untouched(const fs_rx_sock& s) {
    fs_rx_sock_out o;
    o.rcv_nxt = s.rcv_nxt, o.ring_wpos = s.ring_wpos, o.ring_free = s.ring_free;
    o.bytes = o.n_delivered = o.n_dropped = 0;
    o.flow = o.stop = kNone;
    return o;
}

}  // namespace deliver
}  // namespace framesum
