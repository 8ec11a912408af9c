// Arithmetic of the RX coalesce (fs_coalesce_batch), free of HIP so that it compiles on its own, like
// framesum_segment.h and framesum_choice.h: the payload range RecvEth hands to the port for an
// accepted frame, and the rule by which a TCP segment continues the frame before it. The functions
// are __host__ __device__ under hipcc and plain inline functions elsewhere: framesum_coalesce.hip
// runs exactly this code per frame, and tests/csrc/test_coalesce.cpp builds it alone under ASan +
// UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FS_CO_HD __host__ __device__ inline
#define FS_CO_UNROLL _Pragma("unroll")
#else
#define FS_CO_HD inline
#define FS_CO_UNROLL
#endif

namespace framesum {
namespace coalesce {

constexpr uint32_t kHdr = 54;         // Ethernet 14 + IPv4 20 (IHL 5) + TCP 20 (data offset 5)
constexpr uint32_t kHdrWords = 14;    // ... as little-endian dwords, the last two bytes zero
constexpr uint32_t kScanBlock = 256;  // frames per workgroup of the scan kernels (tests read it)
constexpr uint32_t kNoRun = 0xFFFFFFFFu;
constexpr uint32_t kMaxFrames = 1u << 31;

constexpr uint32_t kFin = 0x01, kSyn = 0x02, kRst = 0x04, kPsh = 0x08, kUrg = 0x20;

// A frame's first 54 bytes as 14 little-endian dwords (word k = bytes 4k .. 4k + 3); bytes the frame
// does not have (a UDP frame may be as short as 42 bytes) are zero.
struct Hdr {
    uint32_t w[kHdrWords];
};
FS_CO_HD uint32_t byte_of(const Hdr& h, uint32_t i) { return (h.w[i >> 2] >> (8u * (i & 3u))) & 0xFFu; }
FS_CO_HD uint32_t be16_of(const Hdr& h, uint32_t i) { return (byte_of(h, i) << 8) | byte_of(h, i + 1); }
FS_CO_HD uint32_t be32_of(const Hdr& h, uint32_t i) { return (be16_of(h, i) << 16) | be16_of(h, i + 2); }

// The header of a frame of `avail` bytes at `p` (any alignment), read byte by byte: the host form,
// and the kernel's form for frames shorter than 54 bytes.
FS_CO_HD Hdr load_hdr_bytes(const uint8_t* p, uint32_t avail) {
    Hdr h;
    FS_CO_UNROLL
    for (uint32_t k = 0; k < kHdrWords; ++k) h.w[k] = 0;
    FS_CO_UNROLL
    for (uint32_t i = 0; i < kHdr; ++i)  // (constant bounds: the words stay in registers in the kernel)
        if (i < avail) h.w[i >> 2] |= (uint32_t)p[i] << (8u * (i & 3u));
    return h;
}

// Where an accepted frame's TCP data-offset and flags bytes lie: frame[tcp_bytes_at(h) + {0, 1}].
// With IHL 5 they are bytes 46 and 47 of the header; with IP options they lie beyond its 54 bytes
// and the caller fetches them from the frame (an accepted frame holds its whole TCP header).
FS_CO_HD uint32_t ihl_of(const Hdr& h) { return byte_of(h, 14) & 15u; }
FS_CO_HD bool is_tcp(const Hdr& h) { return byte_of(h, 23) == 6; }
FS_CO_HD uint32_t tcp_bytes_at(const Hdr& h) { return 14u + 4u * ihl_of(h) + 12u; }

// What the classify step keeps of one frame.
struct Info {
    uint32_t start;      // the payload is frame[start : start + len)
    uint32_t len;
    uint32_t tcp_flags;  // TCP: the flags byte; UDP: 0
    bool accepted;       // verdict FS_OK
    bool plain_tcp;      // TCP with IHL 5 and data offset 5: only such frames join
};
FS_CO_HD Info rejected() { return Info{0u, 0u, 0u, false, false}; }

// The payload RecvEth hands to the port (stacks/portstack.go:217, :239, :301-303) of a frame whose
// verdict is FS_OK: UDP frame[14 + IHL*4 + 8 : 14 + TotalLength), TCP frame[14 + IHL*4 + dataoff*4 :
// 14 + TotalLength). `doff_byte` / `flags_byte`: the two bytes at tcp_bytes_at(h) (ignored for UDP).
// FS_OK guarantees start <= 14 + TotalLength <= the frame's length (the verdict's gates), so len
// cannot wrap; it is still clamped, so that a caller's mistake cannot turn into a huge copy.
FS_CO_HD Info payload_range(const Hdr& h, uint32_t doff_byte, uint32_t flags_byte) {
    Info f;
    const uint32_t l4 = 14u + 4u * ihl_of(h);
    const uint32_t end = 14u + be16_of(h, 16);
    const bool tcp = is_tcp(h);
    const uint32_t doff = doff_byte >> 4;
    f.start = l4 + (tcp ? 4u * doff : 8u);
    f.len = end > f.start ? end - f.start : 0u;
    f.tcp_flags = tcp ? (flags_byte & 0xFFu) : 0u;
    f.accepted = true;
    f.plain_tcp = tcp && ihl_of(h) == 5u && doff == 5u;
    return f;
}

// The header bytes two frames of one run must share: every byte but the fields fs_segment_batch
// varies per segment -- IPv4 TotalLength (16, 17), ID (18, 19) and checksum (24, 25), TCP Seq
// (38 .. 41), the FIN and PSH bits of the flags byte (47) and the TCP checksum (50, 51). The
// fragment fields (20, 21) are compared as bytes, as RecvEth does not interpret them.
FS_CO_HD uint32_t compare_mask(uint32_t word) {
    switch (word) {
    case 4: return 0u;                                       // 16 .. 19: TotalLength, ID out
    case 6: return 0xFFFF0000u;                              // 24, 25: IPv4 checksum out
    case 9: return 0x0000FFFFu;                              // 38, 39: Seq out
    case 10: return 0xFFFF0000u;                             // 40, 41: Seq out
    case 11: return 0xFFFFFFFFu & ~((kFin | kPsh) << 24);    // 47: FIN, PSH out
    case 12: return 0x0000FFFFu;                             // 50, 51: TCP checksum out
    case 13: return 0x0000FFFFu;                             // 54, 55 are not header bytes
    default: return 0xFFFFFFFFu;
    }
}
FS_CO_HD bool same_flow_header(const Hdr& a, const Hdr& b) {
    uint32_t diff = 0;
    FS_CO_UNROLL
    for (uint32_t k = 0; k < kHdrWords; ++k) diff |= (a.w[k] ^ b.w[k]) & compare_mask(k);
    return diff == 0;
}

// Does the frame (cur, c) continue the frame before it (prev, p)? Both accepted plain TCP with
// payload, no SYN, RST or URG on either, no FIN or PSH on the earlier one, Seq continuing mod 2^32
// (the arithmetic of TCPConn.recv's in-order check, stacks/tcpconn.go:347-369), the same flow header.
FS_CO_HD bool joins(const Hdr& prev, const Info& p, const Hdr& cur, const Info& c) {
    if (!p.accepted || !c.accepted || !p.plain_tcp || !c.plain_tcp) return false;
    if (p.len == 0 || c.len == 0) return false;
    if ((p.tcp_flags | c.tcp_flags) & (kSyn | kRst | kUrg)) return false;
    if (p.tcp_flags & (kFin | kPsh)) return false;
    if (be32_of(cur, 38) != (uint32_t)(be32_of(prev, 38) + p.len)) return false;
    return same_flow_header(prev, cur);
}

// A run's flags: the first frame's flags byte and the last frame's FIN and PSH.
FS_CO_HD uint32_t run_flags(uint32_t first, uint32_t last) { return (first | (last & (kFin | kPsh))) & 0xFFu; }

// The per-frame record the classify kernel leaves for the scan and the copy: x = payload length
// (16 bits) | payload start (8 bits: at most 14 + 60 + 60) << 16 | flags byte << 24, y = kAccepted |
// kHead (an accepted frame that joins nothing opens a run).
constexpr uint32_t kAccepted = 1u, kHead = 2u;
FS_CO_HD uint32_t pack_info(const Info& f) { return (f.len & 0xFFFFu) | ((f.start & 0xFFu) << 16) | (f.tcp_flags << 24); }
FS_CO_HD uint32_t rec_len(uint32_t x) { return x & 0xFFFFu; }
FS_CO_HD uint32_t rec_start(uint32_t x) { return (x >> 16) & 0xFFu; }
FS_CO_HD uint32_t rec_flags(uint32_t x) { return x >> 24; }

// The copy of `len` bytes to a destination whose address is `dst_addr`: `head` bytes up to the next
// 16-byte boundary of the destination (as 1-, 2-, 4- and 8-byte accesses, the set bits of head),
// `body` whole 16-byte pieces stored aligned, `tail` bytes (8, 4, 2, 1).
struct CopyPlan {
    uint32_t head, body, tail;
};
FS_CO_HD CopyPlan copy_plan(uint64_t dst_addr, uint32_t len) {
    CopyPlan c;
    const uint32_t to_boundary = (uint32_t)((0u - dst_addr) & 15u);
    c.head = len < to_boundary ? len : to_boundary;
    c.body = (len - c.head) >> 4;
    c.tail = (len - c.head) & 15u;
    return c;
}

}  // namespace coalesce
}  // namespace framesum
