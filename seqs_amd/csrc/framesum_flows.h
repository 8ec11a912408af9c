// Arithmetic of the flow-aware RX coalesce (fs_coalesce_flows_batch), free of HIP like
// framesum_coalesce.h, on which it builds: a frame's 13-byte flow key, key equality and hash, the
// flow table's size and the 64-bit sort key that puts the accepted frames into delivery order; and the
// keyed table of a connection list, which the calls behind the flow launches build and probe
// (framesum_deliver.h, framesum_close.h, framesum_connect.h and their kernels). framesum_flows.hip runs
// exactly this code per frame, and tests/csrc/test_flows.cpp and test_deliver.cpp build it alone under
// ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "framesum_coalesce.h"

namespace framesum {
namespace flows {

using namespace coalesce;

constexpr uint32_t kMaxFrames = 1u << 30;  // the flow table (at most 2^31 slots) keeps a 32-bit index
constexpr uint32_t kEmpty = 0xFFFFFFFFu;   // an unclaimed table slot; a flow without a first frame yet
constexpr uint32_t kKeyBytes = 13;

// The 16-byte key record of one frame: bytes 0 .. 12 the flow key -- protocol frame[23], source and
// destination address frame[26 : 34), source and destination port frame[L4 : L4 + 4) with L4 = 14 +
// 4 IHL -- bytes 13, 14 zero, byte 15 the accepted bit. A frame that is not accepted has a zero record.
struct Key {
    uint32_t w[4];
};
constexpr uint32_t kKeyAccepted = 1u << 24;  // byte 15, in w[3]

FS_CO_HD uint32_t l4_of(const Hdr& h) { return 14u + 4u * ihl_of(h); }

// The key record of an accepted frame whose first 54 bytes are `h` (bytes the frame does not have
// are zero there) and whose `avail` bytes lie at `frame`. With IHL 5 the ports are bytes 34 .. 37 of
// `h` (every index into `h` is a constant: it stays in registers in the kernel); with IP options they
// come from the frame. An accepted frame holds its whole L4 header, so the bound on `avail` only
// guards a caller's mistake.
FS_CO_HD Key key_of(const Hdr& h, const uint8_t* frame, uint32_t avail) {
    uint32_t p0 = byte_of(h, 34), p1 = byte_of(h, 35), p2 = byte_of(h, 36), p3 = byte_of(h, 37);
    const uint32_t l4 = l4_of(h);
    if (l4 != 34u) {
        p0 = p1 = p2 = p3 = 0;
        if (l4 + 4u <= avail) p0 = frame[l4], p1 = frame[l4 + 1], p2 = frame[l4 + 2], p3 = frame[l4 + 3];
    }
    Key key;
    key.w[0] = byte_of(h, 23) | (byte_of(h, 26) << 8) | (byte_of(h, 27) << 16) | (byte_of(h, 28) << 24);
    key.w[1] = byte_of(h, 29) | (byte_of(h, 30) << 8) | (byte_of(h, 31) << 16) | (byte_of(h, 32) << 24);
    key.w[2] = byte_of(h, 33) | (p0 << 8) | (p1 << 16) | (p2 << 24);
    key.w[3] = p3 | kKeyAccepted;
    return key;
}
FS_CO_HD Key no_key() { return Key{{0u, 0u, 0u, 0u}}; }
FS_CO_HD bool key_accepted(const Key& k) { return (k.w[3] & kKeyAccepted) != 0; }
FS_CO_HD uint32_t key_byte(const Key& k, uint32_t i) { return (k.w[i >> 2] >> (8u * (i & 3u))) & 0xFFu; }
FS_CO_HD bool same_key(const Key& a, const Key& b) {  // the 13 key bytes
    return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && ((a.w[3] ^ b.w[3]) & 0xFFu) == 0;
}

// Where a key starts probing. Any function of the 13 key bytes will do: the result of the call
// does not depend on it, only the number of probes does.
FS_CO_HD uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}
FS_CO_HD uint32_t key_hash(const Key& k) {
    uint32_t x = mix32(k.w[0] ^ 0x9E3779B9u);
    x = mix32(x ^ k.w[1]);
    x = mix32(x ^ k.w[2]);
    return mix32(x ^ (k.w[3] & 0xFFu));
}

// The flow table: a power of two of at least 2 n slots, so that it is at most half full.
FS_CO_HD uint32_t table_slots(uint32_t n) {
    uint32_t t = 2;
    while (t < 2u * n) t <<= 1;  // (n <= 2^30: t <= 2^31)
    return t;
}

// ---- The keyed table of a connection list (the delivery's sockets, the close call's closers, the
// connect call's openers): table_slots(n) slots, each a record's index or kEmpty, built on the host and
// staged with the records. A key starts probing at its hash & hash_mask (all ones in the product) and
// goes on linearly; the result of a lookup does not depend on the hash. Rec: a record that begins with
// the 13 key bytes as `uint8_t key[13]` (fs_rx_sock, fs_cl_sock, fs_cn_sock).
// The 13 bytes as the key record of the connection's frames: same_key() compares the two.
FS_CO_HD Key wire_key(const uint8_t key[kKeyBytes]) {
    Key k;
    k.w[0] = key[0] | ((uint32_t)key[1] << 8) | ((uint32_t)key[2] << 16) | ((uint32_t)key[3] << 24);
    k.w[1] = key[4] | ((uint32_t)key[5] << 8) | ((uint32_t)key[6] << 16) | ((uint32_t)key[7] << 24);
    k.w[2] = key[8] | ((uint32_t)key[9] << 8) | ((uint32_t)key[10] << 16) | ((uint32_t)key[11] << 24);
    k.w[3] = key[12] | kKeyAccepted;
    return k;
}
FS_CO_HD uint32_t table_start(const Key& k, uint32_t hash_mask, uint32_t tmask) { return key_hash(k) & hash_mask & tmask; }
// The record whose key equals `key`, or kEmpty. At most every slot once.
template <class Rec>
FS_CO_HD uint32_t lookup(const Key& key, const Rec* recs, const uint32_t* table, uint32_t tmask, uint32_t hash_mask) {
    uint32_t s = table_start(key, hash_mask, tmask);
    for (uint32_t probe = 0; probe <= tmask; ++probe) {
        const uint32_t owner = table[s];
        if (owner == kEmpty) return kEmpty;
        if (same_key(key, wire_key(recs[owner].key))) return owner;
        s = (s + 1u) & tmask;
    }
    return kEmpty;
}
// Fills `table` (table_slots(n) entries). Returns kEmpty, or the first record whose key an earlier
// record has already.
template <class Rec>
inline uint32_t build_table(const Rec* recs, uint32_t n, uint32_t hash_mask, uint32_t* table) {
    const uint32_t slots = table_slots(n), tmask = slots - 1u;
    for (uint32_t i = 0; i < slots; ++i) table[i] = kEmpty;
    for (uint32_t i = 0; i < n; ++i) {
        const Key key = wire_key(recs[i].key);
        uint32_t s = table_start(key, hash_mask, tmask);
        for (uint32_t probe = 0; probe <= tmask; ++probe) {
            if (table[s] == kEmpty) {
                table[s] = i;
                break;
            }
            if (same_key(key, wire_key(recs[table[s]].key))) return i;
            s = (s + 1u) & tmask;
        }
    }
    return kEmpty;
}

// The sort key. b = bit_width(n) bits hold a frame index; an accepted frame's key is the batch
// index of its flow's first frame above its own, a frame that is not accepted lies above all of
// them. The keys of a batch are distinct, and sorting them over their low 2 b + 1 bits (at most 63)
// gives the delivery order followed by the frames that are not accepted.
FS_CO_HD uint32_t index_bits(uint32_t n) {
    uint32_t b = 0;
    while (b < 32 && ((uint64_t)n >> b) != 0) ++b;
    return b;
}
FS_CO_HD uint64_t sort_key(uint32_t rep, uint32_t i, uint32_t b) { return ((uint64_t)rep << b) | i; }
FS_CO_HD uint64_t sort_key_rejected(uint32_t i, uint32_t b) { return ((uint64_t)1 << (2u * b)) | i; }
FS_CO_HD uint32_t sort_bits(uint32_t b) { return 2u * b + 1u; }
FS_CO_HD uint32_t sort_index(uint64_t key, uint32_t b) { return (uint32_t)(key & (((uint64_t)1 << b) - 1u)); }
FS_CO_HD uint32_t sort_rep(uint64_t key, uint32_t b) { return (uint32_t)(key >> b); }

// The per-slot record's y bits beside kAccepted and kHead (framesum_coalesce.h): the slot opens a flow.
constexpr uint32_t kFlowHead = 4u;

}  // namespace flows
}  // namespace framesum
