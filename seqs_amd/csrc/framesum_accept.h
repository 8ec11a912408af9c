// Arithmetic of the accept call (fs_accept_flows_batch, include/framesum_accept.h), free of HIP like
// framesum_recv.h, on which it builds: the candidate test of a flow's first frame, the walk over a SYN's
// TCP options, the listener table (open addressing over a hash of `local`, built on the host and staged
// with the listeners and the slots), the checks of the listener and slot lists, the connection record
// and the SYN-ACK's header template of a filled slot, and the sort key that ranks a listener's
// candidates. framesum_accept.hip runs exactly this code per flow, and tests/csrc/test_accept.cpp builds
// it alone under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/framesum_accept.h"
#include "framesum_recv.h"

namespace framesum {
namespace accept {

using namespace recv;

static_assert(sizeof(fs_listener) == 24 && offsetof(fs_listener, mac) == 6 && offsetof(fs_listener, slot_first) == 12,
              "fs_listener is 24 bytes with no padding");
static_assert(sizeof(fs_accept_slot) == 12 && offsetof(fs_accept_slot, ip_id) == 8, "fs_accept_slot is 12 bytes");
static_assert(sizeof(fs_accept_conn) == 48 && offsetof(fs_accept_conn, used) == 13 &&
                  offsetof(fs_accept_conn, remote_mac) == 14 && offsetof(fs_accept_conn, peer_mss) == 20 &&
                  offsetof(fs_accept_conn, frame) == 24 && offsetof(fs_accept_conn, snd_wnd) == 44,
              "fs_accept_conn is 48 bytes with no padding");
static_assert(sizeof(fs_listener_out) == 16, "fs_listener_out is 16 bytes");

constexpr uint32_t kNoSlot = FS_ACCEPT_NONE, kFull = FS_ACCEPT_FULL;
constexpr uint32_t kMaxListeners = FS_ACCEPT_MAX_LISTENERS, kMaxSlots = FS_ACCEPT_MAX_SLOTS;
constexpr uint32_t kStride = FS_ACCEPT_STRIDE;
constexpr uint32_t kMaxOptionSteps = 40;
constexpr uint32_t kSynAck = kSyn | kAck;

// ---- The first frame of a flow as the candidate test reads it, from the 20 bytes at L4.
struct Syn {
    uint32_t seq, ack, window, flags9, doff;
};
FS_CO_HD Syn syn_of(const uint8_t* l4) {
    Syn s;
    s.seq = ((uint32_t)l4[4] << 24) | ((uint32_t)l4[5] << 16) | ((uint32_t)l4[6] << 8) | l4[7];
    s.ack = ((uint32_t)l4[8] << 24) | ((uint32_t)l4[9] << 16) | ((uint32_t)l4[10] << 8) | l4[11];
    s.doff = l4[12] >> 4;
    s.flags9 = (((uint32_t)l4[12] & 1u) << 8) | l4[13];
    s.window = ((uint32_t)l4[14] << 8) | l4[15];
    return s;
}
// Rule 2 without the socket and the listener: protocol 6, the nine flag bits SYN alone
// (tcplistener.go:133), Ack 0 (:137), no payload.
FS_CO_HD bool first_syn(uint32_t proto, const Syn& s, uint32_t payload_len) {
    return proto == 6u && s.flags9 == kSyn && s.ack == 0u && payload_len == 0u;
}

// The value of the first well-formed MSS option (kind 2, length 4) among the `n` option bytes at `opt`
// (n = 4 dataoff - 20 <= 40), or 0.
FS_CO_HD uint32_t peer_mss(const uint8_t* opt, uint32_t n) {
    uint32_t at = 0;
    for (uint32_t step = 0; step < kMaxOptionSteps && at < n; ++step) {
        const uint32_t kind = opt[at];
        if (kind == 0u) break;
        if (kind == 1u) {
            ++at;
            continue;
        }
        if (at + 1u >= n) break;  // the length byte lies outside
        const uint32_t len = opt[at + 1u];
        if (len < 2u || len > n - at) break;
        if (kind == 2u && len == 4u) return ((uint32_t)opt[at + 2u] << 8) | opt[at + 3u];
        at += len;
    }
    return 0u;
}

// ---- The listener table: table_slots(n_listeners) slots, each a listener's index or kNone; a `local`
// starts probing at its hash & hash_mask (all ones in the product) and goes on linearly. The result of
// a lookup does not depend on the hash, only the number of probes does.
// `local` as two words: the address (key bytes 5..8) and the port (11..12), both as a little-endian load
// of the wire bytes sees them.
struct Local {
    uint32_t addr, port;
};
FS_CO_HD Local local_of(const uint8_t local[6]) {
    return Local{local[0] | ((uint32_t)local[1] << 8) | ((uint32_t)local[2] << 16) | ((uint32_t)local[3] << 24),
                 local[4] | ((uint32_t)local[5] << 8)};
}
FS_CO_HD Local local_of_key(const Key& k) {
    return Local{key_byte(k, 5) | (key_byte(k, 6) << 8) | (key_byte(k, 7) << 16) | (key_byte(k, 8) << 24),
                 key_byte(k, 11) | (key_byte(k, 12) << 8)};
}
FS_CO_HD bool same_local(const Local& a, const Local& b) { return a.addr == b.addr && a.port == b.port; }
FS_CO_HD uint32_t local_hash(const Local& l) { return mix32(mix32(l.addr ^ 0x9E3779B9u) ^ l.port); }
FS_CO_HD uint32_t listener_start(const Local& l, uint32_t hash_mask, uint32_t tmask) { return local_hash(l) & hash_mask & tmask; }

// The listener whose `local` equals `l`, or kNone. At most every slot once.
FS_CO_HD uint32_t lookup_listener(const Local& l, const fs_listener* listeners, const uint32_t* table, uint32_t tmask,
                                  uint32_t hash_mask) {
    uint32_t s = listener_start(l, hash_mask, tmask);
    for (uint32_t probe = 0; probe <= tmask; ++probe) {
        const uint32_t owner = table[s];
        if (owner == kNone) return kNone;
        if (same_local(l, local_of(listeners[owner].local))) return owner;
        s = (s + 1u) & tmask;
    }
    return kNone;
}
// Fills `table` (table_slots(n_listeners) entries). Returns kNone, or the first listener whose `local`
// an earlier listener has already.
inline uint32_t build_listener_table(const fs_listener* listeners, uint32_t n_listeners, uint32_t hash_mask, uint32_t* table) {
    const uint32_t slots = table_slots(n_listeners), tmask = slots - 1u;
    for (uint32_t i = 0; i < slots; ++i) table[i] = kNone;
    for (uint32_t i = 0; i < n_listeners; ++i) {
        const Local l = local_of(listeners[i].local);
        uint32_t s = listener_start(l, hash_mask, tmask);
        for (uint32_t probe = 0; probe <= tmask; ++probe) {
            if (table[s] == kNone) {
                table[s] = i;
                break;
            }
            if (same_local(l, local_of(listeners[table[s]].local))) return i;
            s = (s + 1u) & tmask;
        }
    }
    return kNone;
}

// ---- The checks of the listener and slot lists (rule 7), none of which needs a device.
enum BadAccept {
    kAcceptGood = 0, kAcceptNull, kTooManyListeners, kTooManySlots, kSynackFlags, kListenerReserved, kSlotReserved,
    kEqualLocal, kZeroPort, kSlotRange, kSlotsOverlap,
};
inline const char* bad_accept_text(BadAccept b) {
    switch (b) {
    case kAcceptNull: return "null listeners, listeners_out, slots, conns or synacks";
    case kTooManyListeners: return "n_listeners above 65,536";
    case kTooManySlots: return "n_slots above 65,536";
    case kSynackFlags: return "synack_flags must be 0 or FS_FCS_APPEND";
    case kListenerReserved: return "a listener's reserved must be 0";
    case kSlotReserved: return "a slot's reserved must be 0";
    case kEqualLocal: return "its local equals an earlier listener's";
    case kZeroPort: return "its local has port 0";
    case kSlotRange: return "its slot range ends past n_slots";
    case kSlotsOverlap: return "its slot range overlaps another listener's";
    default: return "";
    }
}
struct CheckAccept {
    BadAccept bad;
    uint32_t index;  // the listener or the slot `bad` is about
};
// `table`: resized and filled for the staged block when the lists are good.
inline CheckAccept check_accept(const fs_listener* listeners, uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots,
                                uint32_t synack_flags, bool have_conns, bool have_listeners_out, bool have_synacks,
                                uint32_t hash_mask, std::vector<uint32_t>& table) {
    if (n_listeners > kMaxListeners) return CheckAccept{kTooManyListeners, 0u};
    if (n_slots > kMaxSlots) return CheckAccept{kTooManySlots, 0u};
    if (synack_flags & ~(uint32_t)FS_FCS_APPEND) return CheckAccept{kSynackFlags, 0u};
    if (n_listeners != 0 && (!listeners || !have_listeners_out)) return CheckAccept{kAcceptNull, 0u};
    if (n_slots != 0 && (!slots || !have_conns || !have_synacks)) return CheckAccept{kAcceptNull, 0u};
    for (uint32_t i = 0; i < n_slots; ++i)
        if (slots[i].reserved != 0) return CheckAccept{kSlotReserved, i};
    for (uint32_t i = 0; i < n_listeners; ++i) {
        const fs_listener& l = listeners[i];
        if (l.reserved != 0) return CheckAccept{kListenerReserved, i};
        if ((l.local[4] | l.local[5]) == 0) return CheckAccept{kZeroPort, i};
        if (l.slot_first > n_slots || l.n_slots > n_slots - l.slot_first) return CheckAccept{kSlotRange, i};
    }
    table.resize(table_slots(n_listeners));
    const uint32_t dup = build_listener_table(listeners, n_listeners, hash_mask, table.data());
    if (dup != kNone) return CheckAccept{kEqualLocal, dup};
    // the ranges that hold a slot, by their start: each must end before the next starts
    std::vector<uint32_t> by_first;
    for (uint32_t i = 0; i < n_listeners; ++i)
        if (listeners[i].n_slots != 0) by_first.push_back(i);
    std::sort(by_first.begin(), by_first.end(), [&](uint32_t a, uint32_t b) {
        return listeners[a].slot_first != listeners[b].slot_first ? listeners[a].slot_first < listeners[b].slot_first : a < b;
    });
    for (size_t k = 1; k < by_first.size(); ++k) {
        const fs_listener& p = listeners[by_first[k - 1]];
        if (p.slot_first + p.n_slots > listeners[by_first[k]].slot_first) return CheckAccept{kSlotsOverlap, by_first[k]};
    }
    return CheckAccept{kAcceptGood, 0u};
}

// The staged block of a call: the listeners, then their table, then the slots.
struct Block {
    uint64_t table, slots, bytes;
};
inline Block block_of(uint32_t n_listeners, uint32_t n_slots) {
    Block b;
    b.table = (uint64_t)n_listeners * sizeof(fs_listener);
    b.slots = b.table + 4ull * table_slots(n_listeners);
    b.bytes = b.slots + (uint64_t)n_slots * sizeof(fs_accept_slot);
    return b;
}
inline void stage(const fs_listener* listeners, uint32_t n_listeners, const uint32_t* table, const fs_accept_slot* slots,
                  uint32_t n_slots, const Block& b, uint8_t* dst) {
    if (n_listeners) memcpy(dst, listeners, b.table);
    memcpy(dst + b.table, table, b.slots - b.table);
    if (n_slots) memcpy(dst + b.slots, slots, b.bytes - b.slots);
}

// ---- The rank of a listener's candidates: the keys listener << b | flow (b = index_bits(n), as
// flows::sort_key) sorted over their low b + index_bits(n_listeners) bits put every listener's
// candidates together in ascending flow order; every other entry of the sorted array is all ones, above
// them all (a listener's index is at most n_listeners - 1 < 2^index_bits(n_listeners) - 1).
constexpr uint64_t kNoCandidate = ~(uint64_t)0;
FS_CO_HD uint64_t rank_key(uint32_t listener, uint32_t flow, uint32_t b) { return ((uint64_t)listener << b) | flow; }
FS_CO_HD uint32_t rank_bits(uint32_t b, uint32_t n_listeners) { return b + index_bits(n_listeners); }
// the key's listener as the sort saw it: the bits [b, b + lb)
FS_CO_HD uint32_t rank_listener(uint64_t key, uint32_t b, uint32_t lb) { return (uint32_t)((key >> b) & (((uint64_t)1 << lb) - 1u)); }
FS_CO_HD uint32_t rank_flow(uint64_t key, uint32_t b) { return (uint32_t)(key & (((uint64_t)1 << b) - 1u)); }
// The first position p in sorted[0, n) whose key, over the sorted bits, is at least `key`: at most 32 steps.
FS_CO_HD uint32_t lower_bound(const uint64_t* sorted, uint32_t n, uint64_t key, uint64_t mask) {
    uint32_t lo = 0, hi = n;
    for (uint32_t step = 0; step < 32u && lo < hi; ++step) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if ((sorted[mid] & mask) < key) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// ---- What a filled slot gets.
FS_CO_HD void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}
// The connection record (include/framesum_accept.h) from the slot, the flow's key and the SYN's fields.
FS_CO_HD fs_accept_conn conn_of(const fs_accept_slot& slot, const Key& key, const uint8_t remote_mac[6], const Syn& syn,
                                uint32_t mss, uint32_t frame, uint32_t flow) {
    fs_accept_conn c;
    for (uint32_t i = 0; i < kKeyBytes; ++i) c.key[i] = (uint8_t)key_byte(key, i);
    c.used = 1;
    for (uint32_t i = 0; i < 6; ++i) c.remote_mac[i] = remote_mac[i];
    c.peer_mss = (uint16_t)mss;
    c.reserved = 0;
    c.frame = frame, c.flow = flow;
    c.irs = syn.seq;
    c.rcv_nxt = syn.seq + 1u;  // rcv.NXT += LEN() of a SYN (control_user.go:216-217)
    c.snd_nxt = slot.iss + 1u;
    c.snd_wnd = syn.window;
    return c;
}
// The SYN-ACK's 54 header bytes as the frame body takes a template (framesum_tx_dev.h): everything but
// TotalLength, the ID and the two checksums, which the body writes. Bytes 18, 19 carry the ID seed.
FS_CO_HD void synack_template(const fs_listener& l, const fs_accept_slot& slot, const fs_accept_conn& c, uint8_t h[54]) {
    for (uint32_t i = 0; i < 54; ++i) h[i] = 0;
    for (uint32_t i = 0; i < 6; ++i) h[i] = c.remote_mac[i], h[6 + i] = l.mac[i];
    h[12] = 0x08, h[13] = 0x00;
    h[14] = 0x45;
    h[18] = (uint8_t)(slot.ip_id >> 8), h[19] = (uint8_t)slot.ip_id;
    h[22] = 64, h[23] = 6;
    for (uint32_t i = 0; i < 4; ++i) h[26 + i] = l.local[i], h[30 + i] = c.key[1 + i];
    h[34] = l.local[4], h[35] = l.local[5];  // ports swapped
    h[36] = c.key[9], h[37] = c.key[10];
    put_be32(h + 38, slot.iss);
    put_be32(h + 42, c.rcv_nxt);
    h[46] = 0x50;
    h[47] = (uint8_t)kSynAck;
    const uint32_t wnd = slot.rcv_wnd > kMaxWnd ? kMaxWnd : slot.rcv_wnd;  // (the reference: uint16(rcv.WND))
    h[48] = (uint8_t)(wnd >> 8), h[49] = (uint8_t)wnd;
}

}  // namespace accept
}  // namespace framesum
