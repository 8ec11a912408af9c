// Arithmetic of the ARP call (fs_arp_flows_batch, include/framesum_arp.h), free of HIP like
// framesum_udp.h, whose rank key and search it reuses: the ARP header's fields from a frame's bytes, the
// support check, the MAC filter, the two lookup tables (hosts by IP, queries by host IP and target, both
// the keyed table of framesum_flows.h over 13-byte key records, so both honour the hash mask), the
// classification of one frame, a built frame's words and its IPv4-style digest sum, the checks of the two
// lists with their texts, and the staged block's layout. framesum_arp.hip runs exactly this code per
// frame, and tests/csrc/test_arp.cpp builds it alone under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/framesum_arp.h"
#include "framesum_udp.h"

namespace framesum {
namespace arp {

using namespace udp;

static_assert(sizeof(fs_arp_host) == 20 && offsetof(fs_arp_host, mac) == 4 && offsetof(fs_arp_host, reserved) == 10 &&
                  offsetof(fs_arp_host, slot0) == 12 && offsetof(fs_arp_host, free) == 16,
              "fs_arp_host is 20 bytes with no padding");
static_assert(sizeof(fs_arp_query) == 12 && offsetof(fs_arp_query, target) == 4 && offsetof(fs_arp_query, flags) == 8,
              "fs_arp_query is 12 bytes with no padding");
static_assert(sizeof(fs_arp_host_out) == 16 && offsetof(fs_arp_host_out, first) == 8, "fs_arp_host_out is 16 bytes");
static_assert(sizeof(fs_arp_query_out) == 16 && offsetof(fs_arp_query_out, mac) == 2 && offsetof(fs_arp_query_out, frame) == 8 &&
                  offsetof(fs_arp_query_out, n_replies) == 12,
              "fs_arp_query_out is 16 bytes with no padding");

constexpr uint32_t kNoArp = FS_ARP_NONE;
constexpr uint32_t kMaxHosts = FS_ARP_MAX_HOSTS, kMaxQueries = FS_ARP_MAX_QUERIES, kMaxReplySlots = FS_ARP_MAX_REPLY_SLOTS;
constexpr uint32_t kFrame = FS_ARP_FRAME, kFramePadded = FS_ARP_FRAME_PADDED, kFrameWords = 15;
constexpr uint32_t kArpFlags = FS_ARP_PAD | FS_FCS_APPEND;
constexpr uint32_t kArpVerdict = FS_ARP;

// ---- A six-byte address as two words (bytes 0..3 and 4..5 as a little-endian load sees them), a
// four-byte one as one.
struct Mac {
    uint32_t lo, hi;
};
FS_CO_HD uint32_t le32(const uint8_t* p) { return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
FS_CO_HD Mac mac_of(const uint8_t* p) { return Mac{le32(p), p[4] | ((uint32_t)p[5] << 8)}; }
FS_CO_HD bool same_mac(const Mac& a, const Mac& b) { return a.lo == b.lo && a.hi == b.hi; }
FS_CO_HD bool broadcast(const Mac& a) { return a.lo == 0xFFFFFFFFu && a.hi == 0xFFFFu; }

// ---- Rule 2: what is read of a candidate, frame[0:6) and frame[14:42), byte by byte (any alignment).
struct Pkt {
    Mac dst, sha;
    uint32_t htype, ptype, hlen, plen, op, spa, tpa;
};
FS_CO_HD Pkt parse(const uint8_t* p) {
    Pkt k;
    k.dst = mac_of(p);
    k.htype = ((uint32_t)p[14] << 8) | p[15];
    k.ptype = ((uint32_t)p[16] << 8) | p[17];
    k.hlen = p[18], k.plen = p[19];
    k.op = ((uint32_t)p[20] << 8) | p[21];
    k.sha = mac_of(p + 22);
    k.spa = le32(p + 28);
    k.tpa = le32(p + 38);
    return k;
}
// Rule 3 (arp.go:135-137, 159-160).
FS_CO_HD bool supported(const Pkt& k) {
    return k.htype == 1u && k.ptype == 0x0800u && k.hlen == 6u && k.plen == 4u && (k.op == 1u || k.op == 2u);
}
// The MAC filter of portstack.go:185 for one host.
FS_CO_HD bool hears(const fs_arp_host& h, const Mac& dst) { return broadcast(dst) || same_mac(dst, mac_of(h.mac)); }

// ---- The two tables: the keyed table of framesum_flows.h over key records that carry a host's IP, or a
// query's host's IP and its target, in their first bytes and zeros behind.
struct KeyRec {
    uint8_t key[kKeyBytes];
};
static_assert(sizeof(KeyRec) == 13, "a key record is its 13 bytes");
FS_CO_HD Key host_key(uint32_t ip) { return Key{{ip, 0u, 0u, kKeyAccepted}}; }
FS_CO_HD Key query_key(uint32_t host_ip, uint32_t target) { return Key{{host_ip, target, 0u, kKeyAccepted}}; }
inline KeyRec key_rec(const uint8_t ip[4], const uint8_t* target) {
    KeyRec r;
    memset(r.key, 0, sizeof r.key);
    memcpy(r.key, ip, 4);
    if (target) memcpy(r.key + 4, target, 4);
    return r;
}
struct Tables {
    const fs_arp_host* hosts;
    const fs_arp_query* queries;
    const KeyRec* hkeys;
    const KeyRec* qkeys;
    const uint32_t* htable;
    const uint32_t* qtable;
    uint32_t n_hosts, n_queries, htmask, qtmask, hash_mask;
};
FS_CO_HD uint32_t lookup_host(const Tables& t, uint32_t ip) {
    if (t.n_hosts == 0u) return kNoArp;
    const uint32_t h = lookup(host_key(ip), t.hkeys, t.htable, t.htmask, t.hash_mask);
    return h < t.n_hosts ? h : kNoArp;
}
FS_CO_HD uint32_t lookup_query(const Tables& t, uint32_t host_ip, uint32_t target) {
    if (t.n_queries == 0u) return kNoArp;
    const uint32_t q = lookup(query_key(host_ip, target), t.qkeys, t.qtable, t.qtmask, t.hash_mask);
    return q < t.n_queries ? q : kNoArp;
}

// ---- Rules 2 to 5 for one frame, as far as one frame alone decides them: `code` is final but for a
// matched request (FS_ARP_ANSWERED here; the rank decides between it and FS_ARP_FULL, and gives the slot)
// and a matched reply (FS_ARP_STALE here; the lowest batch index becomes FS_ARP_RESOLVED). `host`: the
// matched request's host; `of`: the matched reply's query.
struct Class {
    uint32_t code, host, of;
};
FS_CO_HD Class classify(const Tables& t, const uint8_t* frame, bool candidate) {
    Class c{FS_ARP_NOT_ARP, kNoArp, kNoArp};
    if (!candidate) return c;
    const Pkt k = parse(frame);
    c.code = FS_ARP_UNSUPPORTED;
    if (!supported(k)) return c;
    c.code = FS_ARP_IGNORED;
    const uint32_t h = lookup_host(t, k.tpa);
    if (h == kNoArp || !hears(t.hosts[h], k.dst)) return c;
    if (k.op == 1u) {
        c.code = FS_ARP_ANSWERED, c.host = h;
        return c;
    }
    const uint32_t q = lookup_query(t, k.tpa, k.spa);
    if (q == kNoArp || (t.queries[q].flags & FS_ARP_SEND_REQUEST)) return c;
    c.code = FS_ARP_STALE, c.of = q;
    return c;
}

// Rule 4: the slot of the host's r-th matched request, or kNoArp (FS_ARP_FULL).
FS_CO_HD uint32_t slot_of_rank(const fs_arp_host& h, uint32_t r) { return r < h.free ? h.slot0 + r : kNoArp; }
FS_CO_HD fs_arp_host_out host_out(const fs_arp_host& h, uint32_t n_requests, uint32_t first) {
    fs_arp_host_out o;
    o.n_requests = n_requests;
    o.n_answered = n_requests < h.free ? n_requests : h.free;
    o.first = first;
    o.free = h.free - o.n_answered;
    return o;
}
// Rules 5 and 6: a query's out record. `frame`: the resolving reply's batch index or kNoArp; `sha`: its
// HardwareSender.
FS_CO_HD fs_arp_query_out query_out(const fs_arp_query& q, uint32_t frame, const Mac& sha, uint32_t n_replies) {
    fs_arp_query_out o;
    const bool sent = (q.flags & FS_ARP_SEND_REQUEST) != 0, done = !sent && frame != kNoArp;
    o.state = (uint8_t)(sent ? FS_ARP_Q_SENT : done ? FS_ARP_Q_DONE : FS_ARP_Q_WAIT);
    o.reserved = 0;
    for (uint32_t i = 0; i < 6; ++i) o.mac[i] = done ? (uint8_t)((i < 4 ? sha.lo >> (8 * i) : sha.hi >> (8 * (i - 4))) & 0xFFu) : 0;
    o.frame = done ? frame : kNoArp;
    o.n_replies = sent ? 0u : n_replies;
    return o;
}

// ---- A built frame (rule 9) as fifteen little-endian words, the last 18 bytes zero (the padding).
struct Fields {
    Mac eth_dst, sha, tha;
    uint32_t op, spa, tpa;
};
// The reply to a request whose header is `k` (rule 4), and the who-has frame of a query (rule 6).
FS_CO_HD Fields reply_fields(const fs_arp_host& h, const Pkt& k) { return Fields{k.sha, mac_of(h.mac), k.sha, 2u, le32(h.ip), k.spa}; }
FS_CO_HD Fields request_fields(const fs_arp_host& h, const fs_arp_query& q) {
    return Fields{Mac{0xFFFFFFFFu, 0xFFFFu}, mac_of(h.mac), Mac{0u, 0u}, 1u, le32(h.ip), le32(q.target)};
}
FS_CO_HD void frame_words(const Fields& f, uint32_t w[kFrameWords]) {
    w[0] = f.eth_dst.lo;
    w[1] = f.eth_dst.hi | (f.sha.lo << 16);
    w[2] = (f.sha.lo >> 16) | (f.sha.hi << 16);
    w[3] = 0x01000608u;  // EtherType 0x0806, HardwareType 1
    w[4] = 0x04060008u;  // ProtoType 0x0800, HardwareLength 6, ProtoLength 4
    w[5] = (f.op << 8) | (f.sha.lo << 16);
    w[6] = (f.sha.lo >> 16) | (f.sha.hi << 16);
    w[7] = f.spa;
    w[8] = f.tha.lo;
    w[9] = f.tha.hi | (f.tpa << 16);
    w[10] = f.tpa >> 16;
    w[11] = w[12] = w[13] = w[14] = 0u;
}
FS_CO_HD uint32_t frame_len(uint32_t arp_flags) { return (arp_flags & FS_ARP_PAD) ? kFramePadded : kFrame; }
// fs_digest.ip_csum of a built frame: IPv4Header.CalculateChecksum() of frame[14:34) as the digest kernels
// have it (the version nibble forced to 4, the checksum field's bytes 24, 25 left out), as a number.
FS_CO_HD uint32_t ip_csum_of(const uint32_t w[kFrameWords]) {
    uint32_t s = 0;
    for (uint32_t hw = 7; hw < 17; ++hw) {  // the halfwords at bytes 14 .. 33
        uint32_t v = (w[hw >> 1] >> (16u * (hw & 1u))) & 0xFFFFu;
        if (hw == 7u) v = (v & 0xFF0Fu) | 0x40u;
        if (hw == 12u) v = 0u;
        s += ((v & 0xFFu) << 8) | (v >> 8);
    }
    s = (s & 0xFFFFu) + (s >> 16);
    s = (s & 0xFFFFu) + (s >> 16);
    return ~s & 0xFFFFu;
}
// The verdict of a built frame of `len` bytes under the call's mtu (RecvEth's gates: only the MTU's can refuse it).
FS_CO_HD uint32_t built_verdict(uint32_t len, uint32_t mtu) { return mtu != 0u && len > mtu ? (uint32_t)FS_ERR_EXCEEDS_MTU : kArpVerdict; }

// ---- The checks of the two lists (section 11 of the header), none of which needs a device.
enum BadArp {
    kArpGood = 0, kArpNullHosts, kArpNullQueries, kTooManyHosts, kTooManyQueries, kTooManyReplySlots, kArpFlagsBad, kHostReserved,
    kQueryReserved, kEqualIp, kArpSlotRange, kArpSlotsOverlap, kQueryHost, kEqualQuery, kQueryFlags,
};
inline const char* bad_arp_text(BadArp b) {
    switch (b) {
    case kArpNullHosts: return "null hosts, hosts_out or arp_frames";
    case kArpNullQueries: return "null queries, queries_out or arp_frames";
    case kTooManyHosts: return "n_hosts above 65,536";
    case kTooManyQueries: return "n_queries above 65,536";
    case kTooManyReplySlots: return "n_reply_slots above 65,536";
    case kArpFlagsBad: return "arp_flags must lie in FS_ARP_PAD | FS_FCS_APPEND";
    case kHostReserved: return "a host's reserved must be 0";
    case kQueryReserved: return "a query's reserved must be 0";
    case kEqualIp: return "its ip equals an earlier host's";
    case kArpSlotRange: return "its slot range ends past n_reply_slots";
    case kArpSlotsOverlap: return "its slot range overlaps another host's";
    case kQueryHost: return "its host is not below n_hosts";
    case kEqualQuery: return "its host and target equal an earlier query's";
    case kQueryFlags: return "its flags must be 0 or FS_ARP_SEND_REQUEST";
    default: return "";
    }
}
struct CheckArp {
    BadArp bad;
    uint32_t index;  // the host or the query `bad` is about
};
// What a good pair of lists leaves for the staged block: the key records and the tables.
struct Built {
    std::vector<KeyRec> hkeys, qkeys;
    std::vector<uint32_t> htable, qtable;
};
inline CheckArp check_arp(const fs_arp_host* hosts, uint32_t n_hosts, const fs_arp_query* queries, uint32_t n_queries,
                          uint32_t n_reply_slots, uint32_t arp_flags, bool have_hosts_out, bool have_queries_out,
                          bool have_frames, uint32_t hash_mask, Built& built) {
    if (n_hosts > kMaxHosts) return CheckArp{kTooManyHosts, 0u};
    if (n_queries > kMaxQueries) return CheckArp{kTooManyQueries, 0u};
    if (n_reply_slots > kMaxReplySlots) return CheckArp{kTooManyReplySlots, 0u};
    if (arp_flags & ~kArpFlags) return CheckArp{kArpFlagsBad, 0u};
    if (n_hosts != 0 && (!hosts || !have_hosts_out || !have_frames)) return CheckArp{kArpNullHosts, 0u};
    if (n_queries != 0 && (!queries || !have_queries_out || !have_frames)) return CheckArp{kArpNullQueries, 0u};
    built.hkeys.resize(n_hosts), built.qkeys.resize(n_queries);
    for (uint32_t i = 0; i < n_hosts; ++i) {
        const fs_arp_host& h = hosts[i];
        if (h.reserved != 0) return CheckArp{kHostReserved, i};
        if (h.slot0 > n_reply_slots || h.free > n_reply_slots - h.slot0) return CheckArp{kArpSlotRange, i};
        built.hkeys[i] = key_rec(h.ip, nullptr);
    }
    built.htable.resize(table_slots(n_hosts));
    uint32_t dup = build_table(built.hkeys.data(), n_hosts, hash_mask, built.htable.data());
    if (dup != kEmpty) return CheckArp{kEqualIp, dup};
    // the ranges that hold a slot, by their start: each must end before the next starts
    std::vector<uint32_t> by_first;
    for (uint32_t i = 0; i < n_hosts; ++i)
        if (hosts[i].free != 0) by_first.push_back(i);
    std::sort(by_first.begin(), by_first.end(),
              [&](uint32_t a, uint32_t b) { return hosts[a].slot0 != hosts[b].slot0 ? hosts[a].slot0 < hosts[b].slot0 : a < b; });
    for (size_t k = 1; k < by_first.size(); ++k) {
        const fs_arp_host& p = hosts[by_first[k - 1]];
        if (p.slot0 + p.free > hosts[by_first[k]].slot0) return CheckArp{kArpSlotsOverlap, by_first[k]};
    }
    for (uint32_t i = 0; i < n_queries; ++i) {
        const fs_arp_query& q = queries[i];
        if (q.reserved != 0) return CheckArp{kQueryReserved, i};
        if (q.flags & ~(uint32_t)FS_ARP_SEND_REQUEST) return CheckArp{kQueryFlags, i};
        if (q.host >= n_hosts) return CheckArp{kQueryHost, i};
        built.qkeys[i] = key_rec(hosts[q.host].ip, q.target);
    }
    built.qtable.resize(table_slots(n_queries));
    dup = build_table(built.qkeys.data(), n_queries, hash_mask, built.qtable.data());
    if (dup != kEmpty) return CheckArp{kEqualQuery, dup};
    return CheckArp{kArpGood, 0u};
}

// The staged block of a call: the hosts, the queries, the two tables, then the key records (byte records
// last: everything in front of them stays 4-byte aligned).
struct Block {
    uint64_t queries, htable, qtable, hkeys, qkeys, bytes;
};
inline Block block_of(uint32_t n_hosts, uint32_t n_queries) {
    Block b;
    b.queries = (uint64_t)n_hosts * sizeof(fs_arp_host);
    b.htable = b.queries + (uint64_t)n_queries * sizeof(fs_arp_query);
    b.qtable = b.htable + 4ull * table_slots(n_hosts);
    b.hkeys = b.qtable + 4ull * table_slots(n_queries);
    b.qkeys = b.hkeys + (uint64_t)n_hosts * sizeof(KeyRec);
    b.bytes = b.qkeys + (uint64_t)n_queries * sizeof(KeyRec);
    return b;
}
inline void stage(const fs_arp_host* hosts, uint32_t n_hosts, const fs_arp_query* queries, uint32_t n_queries, const Built& built,
                  const Block& b, uint8_t* dst) {
    if (n_hosts) memcpy(dst, hosts, b.queries);
    if (n_queries) memcpy(dst + b.queries, queries, b.htable - b.queries);
    memcpy(dst + b.htable, built.htable.data(), b.qtable - b.htable);
    memcpy(dst + b.qtable, built.qtable.data(), b.hkeys - b.qtable);
    if (n_hosts) memcpy(dst + b.hkeys, built.hkeys.data(), b.qkeys - b.hkeys);
    if (n_queries) memcpy(dst + b.qkeys, built.qkeys.data(), b.bytes - b.qkeys);
}
FS_CO_HD Tables tables_of(const uint8_t* block, const Block& b, uint32_t n_hosts, uint32_t n_queries, uint32_t hash_mask) {
    Tables t;
    t.hosts = reinterpret_cast<const fs_arp_host*>(block);
    t.queries = reinterpret_cast<const fs_arp_query*>(block + b.queries);
    t.htable = reinterpret_cast<const uint32_t*>(block + b.htable);
    t.qtable = reinterpret_cast<const uint32_t*>(block + b.qtable);
    t.hkeys = reinterpret_cast<const KeyRec*>(block + b.hkeys);
    t.qkeys = reinterpret_cast<const KeyRec*>(block + b.qkeys);
    t.n_hosts = n_hosts, t.n_queries = n_queries;
    t.htmask = table_slots(n_hosts) - 1u, t.qtmask = table_slots(n_queries) - 1u;
    t.hash_mask = hash_mask;
    return t;
}

}  // namespace arp
}  // namespace framesum
