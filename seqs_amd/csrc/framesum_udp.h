// Arithmetic of the UDP call (fs_udp_flows_batch, include/framesum_udp.h), free of HIP like
// framesum_accept.h, whose six-byte `local` hash and probe it reuses: the match rule over a frame's key
// record, the port table (open addressing over the hash of `local`; the wildcard address is a second
// probe), the rank key that orders a port's datagrams, a datagram's numbers and the cell header, the
// checks of the port list with their texts, and the staged block's layout. framesum_udp.hip runs exactly
// this code per frame, and tests/csrc/test_udp.cpp builds it alone under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/framesum_udp.h"
#include "framesum_accept.h"

namespace framesum {
namespace udp {

using namespace accept;

static_assert(sizeof(fs_udp_port) == 32 && offsetof(fs_udp_port, n_cells) == 8 && offsetof(fs_udp_port, cells_off) == 16 &&
                  offsetof(fs_udp_port, wcell) == 24,
              "fs_udp_port is 32 bytes with no padding");
static_assert(sizeof(fs_udp_cell) == 32 && offsetof(fs_udp_cell, len) == 4 && offsetof(fs_udp_cell, src_port) == 10 &&
                  offsetof(fs_udp_cell, src_ip) == 12 && offsetof(fs_udp_cell, src_mac) == 20 &&
                  offsetof(fs_udp_cell, dst_mac) == 26,
              "fs_udp_cell is 32 bytes with no padding");
static_assert(sizeof(fs_udp_port_out) == 32 && offsetof(fs_udp_port_out, first) == 20 && offsetof(fs_udp_port_out, bytes) == 24,
              "fs_udp_port_out is 32 bytes with no padding");

constexpr uint32_t kNoPort = FS_UDP_NONE, kCellFull = FS_UDP_FULL;
constexpr uint32_t kMaxPorts = FS_UDP_MAX_PORTS;
constexpr uint32_t kCellHeader = FS_UDP_CELL_HEADER;
constexpr uint32_t kMinCell = 40, kMaxCell = 65568;
constexpr uint32_t kMaxCells = 1u << 31;
constexpr uint32_t kProtoUdp = 17;

// ---- The match (rule 3). A frame's key record (framesum_flows.h) carries all of it: the accepted bit
// is the verdict FS_OK, byte 0 the protocol, bytes 5..8 and 11..12 the destination.
FS_CO_HD bool is_datagram(const Key& k) { return key_accepted(k) && key_byte(k, 0) == kProtoUdp; }
// The same record from the frame's own bytes, for a call whose flow stage has left none: `ok` is the
// verdict FS_OK, which says the frame holds its UDP header.
FS_CO_HD Key key_of_frame(const uint8_t* p, bool ok) {
    if (!ok) return no_key();
    const uint32_t l4 = 14u + 4u * (p[14] & 15u);
    Key k;
    k.w[0] = p[23] | ((uint32_t)p[26] << 8) | ((uint32_t)p[27] << 16) | ((uint32_t)p[28] << 24);
    k.w[1] = p[29] | ((uint32_t)p[30] << 8) | ((uint32_t)p[31] << 16) | ((uint32_t)p[32] << 24);
    k.w[2] = p[33] | ((uint32_t)p[l4] << 8) | ((uint32_t)p[l4 + 1] << 16) | ((uint32_t)p[l4 + 2] << 24);
    k.w[3] = p[l4 + 3] | kKeyAccepted;
    return k;
}

// ---- The port table: table_slots(n_ports) slots, each a port's index or kNone, probed as the
// listener table is. The result of a lookup does not depend on the hash.
FS_CO_HD uint32_t lookup_local(const Local& l, const fs_udp_port* ports, const uint32_t* table, uint32_t tmask, uint32_t hash_mask) {
    uint32_t s = listener_start(l, hash_mask, tmask);
    for (uint32_t probe = 0; probe <= tmask; ++probe) {
        const uint32_t owner = table[s];
        if (owner == kNone) return kNone;
        if (same_local(l, local_of(ports[owner].local))) return owner;
        s = (s + 1u) & tmask;
    }
    return kNone;
}
// The port of a frame whose key record is `k`, or kNoPort: the exact destination first, then the
// wildcard address with the same port.
FS_CO_HD uint32_t match_port(const Key& k, const fs_udp_port* ports, const uint32_t* table, uint32_t n_ports, uint32_t tmask,
                             uint32_t hash_mask) {
    if (n_ports == 0u || !is_datagram(k)) return kNoPort;
    const Local l = local_of_key(k);
    uint32_t p = lookup_local(l, ports, table, tmask, hash_mask);
    if (p == kNone && l.addr != 0u) p = lookup_local(Local{0u, l.port}, ports, table, tmask, hash_mask);
    return p < n_ports ? p : kNoPort;
}
// Fills `table` (table_slots(n_ports) entries). Returns kNone, or the first port whose `local` an
// earlier port has already.
inline uint32_t build_port_table(const fs_udp_port* ports, uint32_t n_ports, uint32_t hash_mask, uint32_t* table) {
    const uint32_t slots = table_slots(n_ports), tmask = slots - 1u;
    for (uint32_t i = 0; i < slots; ++i) table[i] = kNone;
    for (uint32_t i = 0; i < n_ports; ++i) {
        const Local l = local_of(ports[i].local);
        uint32_t s = listener_start(l, hash_mask, tmask);
        for (uint32_t probe = 0; probe <= tmask; ++probe) {
            if (table[s] == kNone) {
                table[s] = i;
                break;
            }
            if (same_local(l, local_of(ports[table[s]].local))) return i;
            s = (s + 1u) & tmask;
        }
    }
    return kNone;
}

// ---- The rank of a port's datagrams: the keys port << b | frame (b = index_bits(n)) sorted over their
// low b + index_bits(n_ports) bits put every port's frames together in ascending batch index; an
// unmatched frame's key is all ones, above them all (accept::rank_key, rank_bits and lower_bound).
constexpr uint64_t kUnmatched = ~(uint64_t)0;
FS_CO_HD uint32_t rank_port(uint64_t key, uint32_t b) { return (uint32_t)(key >> b); }
FS_CO_HD uint32_t rank_frame(uint64_t key, uint32_t b) { return (uint32_t)(key & (((uint64_t)1 << b) - 1u)); }
// Rule 4: the cell of the port's r-th matched frame, or kCellFull.
FS_CO_HD uint32_t cell_of_rank(const fs_udp_port& p, uint32_t r) {
    if (r >= p.free) return kCellFull;
    const uint64_t c = (uint64_t)p.wcell + r;  // (wcell < n_cells and r < free <= n_cells: below 2 n_cells)
    return (uint32_t)(c >= p.n_cells ? c - p.n_cells : c);
}
// The out record of a port with n_matched frames (`first`, `n_truncated` and `bytes` are the caller's).
FS_CO_HD fs_udp_port_out port_out(const fs_udp_port& p, uint32_t n_matched) {
    fs_udp_port_out o;
    o.n_matched = n_matched;
    o.n_admitted = n_matched < p.free ? n_matched : p.free;
    const uint64_t c = (uint64_t)p.wcell + o.n_admitted;  // (below 2 n_cells)
    o.wcell = (uint32_t)(c >= p.n_cells ? c - p.n_cells : c);
    o.free = p.free - o.n_admitted;
    o.n_truncated = 0u, o.first = kNoPort, o.bytes = 0u;
    return o;
}

// ---- A datagram's numbers from its frame (`avail` bytes at `p`, the FCS not counted) for a cell of
// `cell_size` bytes. An accepted frame holds TotalLength bytes behind its Ethernet header, so the bounds
// on `avail` only guard a caller's mistake.
struct Dgram {
    uint32_t start, len, stored, udp_length, src_port;
};
FS_CO_HD Dgram dgram_of(const uint8_t* p, uint32_t avail, uint32_t cell_size) {
    Dgram d;
    const uint32_t ihl4 = 4u * (p[14] & 15u), l4 = 14u + ihl4;
    const uint32_t total = ((uint32_t)p[16] << 8) | p[17];
    d.start = l4 + 8u;
    d.len = total >= ihl4 + 8u ? total - ihl4 - 8u : 0u;
    d.udp_length = d.src_port = 0u;
    if (l4 + 8u <= avail) {
        d.src_port = ((uint32_t)p[l4] << 8) | p[l4 + 1u];
        d.udp_length = ((uint32_t)p[l4 + 4u] << 8) | p[l4 + 5u];
    }
    const uint32_t room = cell_size - kCellHeader, held = avail > d.start ? avail - d.start : 0u;
    d.stored = d.len < room ? d.len : room;
    if (d.stored > held) d.stored = held;
    return d;
}
// The cell header as eight little-endian words (what a store of the struct writes).
FS_CO_HD void cell_words(const uint8_t* p, uint32_t frame, const Dgram& d, uint32_t w[8]) {
    w[0] = frame;
    w[1] = (d.len & 0xFFFFu) | (d.stored << 16);
    w[2] = (d.udp_length & 0xFFFFu) | (d.src_port << 16);
    w[3] = p[26] | ((uint32_t)p[27] << 8) | ((uint32_t)p[28] << 16) | ((uint32_t)p[29] << 24);
    w[4] = p[30] | ((uint32_t)p[31] << 8) | ((uint32_t)p[32] << 16) | ((uint32_t)p[33] << 24);
    w[5] = p[6] | ((uint32_t)p[7] << 8) | ((uint32_t)p[8] << 16) | ((uint32_t)p[9] << 24);
    w[6] = p[10] | ((uint32_t)p[11] << 8) | ((uint32_t)p[0] << 16) | ((uint32_t)p[1] << 24);
    w[7] = p[2] | ((uint32_t)p[3] << 8) | ((uint32_t)p[4] << 16) | ((uint32_t)p[5] << 24);
}

// ---- The lanes per datagram of the copy, decided per call from the port list's largest cell: 4 where no
// cell has room for more than 64 payload bytes (each lane has at most one 16-byte piece), else 16.
constexpr uint32_t kNarrowLanes = 4, kWideLanes = 16, kNarrowRoom = 16 * kNarrowLanes;
FS_CO_HD uint32_t copy_lanes(uint32_t max_cell_size) { return max_cell_size <= kCellHeader + kNarrowRoom ? kNarrowLanes : kWideLanes; }
inline uint32_t max_cell_size(const fs_udp_port* ports, uint32_t n_ports) {
    uint32_t m = 0;
    for (uint32_t i = 0; i < n_ports; ++i) m = ports[i].cell_size > m ? ports[i].cell_size : m;
    return m;
}

// ---- The checks of the port list (section 8 of the header), none of which needs a device.
enum BadUdp {
    kUdpGood = 0, kUdpNull, kTooManyPorts, kUdpReserved, kUdpZeroPort, kUdpEqualLocal, kUdpCellSize, kUdpCellsOff, kUdpNCells,
    kUdpWcell, kUdpFree, kUdpOutside, kUdpOverlap,
};
inline const char* bad_udp_text(BadUdp b) {
    switch (b) {
    case kUdpNull: return "null ports, cells or ports_out";
    case kTooManyPorts: return "n_ports above 65,536";
    case kUdpReserved: return "reserved must be 0";
    case kUdpZeroPort: return "its local has port 0";
    case kUdpEqualLocal: return "its local equals an earlier port's";
    case kUdpCellSize: return "cell_size must be a multiple of 8 from 40 to 65,568";
    case kUdpCellsOff: return "cells_off must be a multiple of 8";
    case kUdpNCells: return "n_cells must be from 1 to 2^31";
    case kUdpWcell: return "wcell must be below n_cells";
    case kUdpFree: return "free must be at most n_cells";
    case kUdpOutside: return "its queue ends past cells_bytes";
    case kUdpOverlap: return "its queue overlaps another port's";
    default: return "";
    }
}
struct CheckUdp {
    BadUdp bad;
    uint32_t index;   // the port `bad` is about
    uint64_t lo, hi;  // the span of `cells` the queues cover (0, 0 without a port)
};
FS_CO_HD uint64_t queue_bytes(const fs_udp_port& p) { return (uint64_t)p.n_cells * p.cell_size; }
// `table`: resized and filled for the staged block when the list is good.
inline CheckUdp check_ports(const fs_udp_port* ports, uint32_t n_ports, bool have_cells, bool have_out, uint64_t cells_bytes,
                            uint32_t hash_mask, std::vector<uint32_t>& table) {
    if (n_ports > kMaxPorts) return CheckUdp{kTooManyPorts, 0u, 0u, 0u};
    if (n_ports != 0 && (!ports || !have_cells || !have_out)) return CheckUdp{kUdpNull, 0u, 0u, 0u};
    uint64_t lo = ~(uint64_t)0, hi = 0;
    for (uint32_t i = 0; i < n_ports; ++i) {
        const fs_udp_port& p = ports[i];
        if (p.reserved[0] | p.reserved[1]) return CheckUdp{kUdpReserved, i, 0u, 0u};
        if ((p.local[4] | p.local[5]) == 0) return CheckUdp{kUdpZeroPort, i, 0u, 0u};
        if (p.cell_size < kMinCell || p.cell_size > kMaxCell || (p.cell_size & 7u)) return CheckUdp{kUdpCellSize, i, 0u, 0u};
        if (p.cells_off & 7u) return CheckUdp{kUdpCellsOff, i, 0u, 0u};
        if (p.n_cells == 0u || p.n_cells > kMaxCells) return CheckUdp{kUdpNCells, i, 0u, 0u};
        if (p.wcell >= p.n_cells) return CheckUdp{kUdpWcell, i, 0u, 0u};
        if (p.free > p.n_cells) return CheckUdp{kUdpFree, i, 0u, 0u};
        // (n_cells * cell_size < 2^48: the sum cannot wrap unless cells_off is huge, which the first test catches)
        if (p.cells_off > cells_bytes || queue_bytes(p) > cells_bytes - p.cells_off) return CheckUdp{kUdpOutside, i, 0u, 0u};
        lo = std::min(lo, p.cells_off), hi = std::max(hi, p.cells_off + queue_bytes(p));
    }
    table.resize(table_slots(n_ports));
    const uint32_t dup = build_port_table(ports, n_ports, hash_mask, table.data());
    if (dup != kNone) return CheckUdp{kUdpEqualLocal, dup, 0u, 0u};
    // the queues by their start: each must end before the next starts
    std::vector<uint32_t> by_off(n_ports);
    for (uint32_t i = 0; i < n_ports; ++i) by_off[i] = i;
    std::sort(by_off.begin(), by_off.end(),
              [&](uint32_t a, uint32_t b) { return ports[a].cells_off != ports[b].cells_off ? ports[a].cells_off < ports[b].cells_off : a < b; });
    for (size_t k = 1; k < by_off.size(); ++k) {
        const fs_udp_port& p = ports[by_off[k - 1]];
        if (p.cells_off + queue_bytes(p) > ports[by_off[k]].cells_off) return CheckUdp{kUdpOverlap, by_off[k], 0u, 0u};
    }
    return n_ports ? CheckUdp{kUdpGood, 0u, lo, hi} : CheckUdp{kUdpGood, 0u, 0u, 0u};
}

// The staged block of a call: the port records as the caller gave them, then their table.
struct Block {
    uint64_t table, bytes;
};
inline Block block_of(uint32_t n_ports) {
    Block b;
    b.table = (uint64_t)n_ports * sizeof(fs_udp_port);
    b.bytes = b.table + 4ull * table_slots(n_ports);
    return b;
}
inline void stage(const fs_udp_port* ports, uint32_t n_ports, const uint32_t* table, const Block& b, uint8_t* dst) {
    if (n_ports) memcpy(dst, ports, b.table);
    memcpy(dst + b.table, table, b.bytes - b.table);
}

}  // namespace udp
}  // namespace framesum
