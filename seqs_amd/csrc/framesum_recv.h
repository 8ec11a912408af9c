// Arithmetic of the receive call (fs_recv_flows_batch, include/framesum_recv.h), free of HIP like
// framesum_deliver.h, on which it builds: the checks of the send-side list, the per-frame rule
// (code_of, step), the record staged per socket, and the operator under which the walk scans snd.UNA
// over 64 frames at once. framesum_recv.hip runs exactly this code per frame, and
// tests/csrc/test_recv.cpp builds it alone under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/framesum_recv.h"
#include "framesum_deliver.h"

namespace framesum {
namespace recv {

using namespace deliver;

static_assert(sizeof(fs_rx_snd) == 8 && sizeof(fs_rx_snd_out) == 32, "fs_rx_snd / fs_rx_snd_out layout");

constexpr uint32_t kMaxWnd = 65535u;
constexpr uint32_t kNs = 0x100u;      // the ninth flag bit (bit 0 of byte L4 + 12)
constexpr uint32_t kHalf = 1u << 31;  // the distance at which LessThan stops being an order
enum Code : uint32_t { kNoCode = 0, kTaken = 1, kDuplicate = 2, kUnsent = 3, kRejected = 4, kKeepalive = 5, kRingFull = 6 };

// ---- The checks of the send-side list, none of which needs a device.
enum BadSnd { kSndGood = 0, kSndNull, kSndWnd, kSndUnaAhead };
inline const char* bad_snd_text(BadSnd b) {
    switch (b) {
    case kSndNull: return "null snd or snd_out";
    case kSndWnd: return "snd_wnd above 65,535";
    case kSndUnaAhead: return "snd_una is ahead of snd_nxt";
    default: return "";
    }
}
struct CheckSnd {
    BadSnd bad;
    uint32_t sock;  // the socket `bad` is about
};
// (`socks` has passed deliver::check_socks.)
inline CheckSnd check_snd(const fs_rx_sock* socks, const fs_rx_snd* snd, uint32_t n_socks, bool have_out) {
    if (n_socks == 0) return CheckSnd{kSndGood, 0u};
    if (!snd || !have_out) return CheckSnd{kSndNull, 0u};
    for (uint32_t i = 0; i < n_socks; ++i) {
        if (snd[i].snd_wnd > kMaxWnd) return CheckSnd{kSndWnd, i};
        // snd_una - snd_nxt as a signed 32-bit difference: above 0 is ahead (2^31 behind passes)
        if ((snd[i].snd_una - socks[i].snd_nxt) - 1u < 0x7FFFFFFFu) return CheckSnd{kSndUnaAhead, i};
    }
    return CheckSnd{kSndGood, 0u};
}

// What the walk reads of a socket: staged per call, n_socks records.
struct Sock {
    uint32_t snd_una, snd_wnd, snd_nxt, rcv_wnd, rcv_nxt;
};
inline void stage(const fs_rx_sock* socks, const fs_rx_snd* snd, uint32_t n_socks, Sock* out) {
    for (uint32_t i = 0; i < n_socks; ++i)
        out[i] = Sock{snd[i].snd_una, snd[i].snd_wnd, socks[i].snd_nxt, socks[i].rcv_wnd, socks[i].rcv_nxt};
}

// ---- The reference's modular comparisons (valuesize.go:27-34).
FS_CO_HD bool less_than(uint32_t v, uint32_t w) { return (int32_t)(v - w) < 0; }
FS_CO_HD bool less_than_eq(uint32_t v, uint32_t w) { return v == w || less_than(v, w); }

// ---- One frame as the walk reads it. The dword at L4 + 12, loaded little-endian, holds the data
// offset and NS, the flags byte and the big-endian window.
struct Frame {
    uint32_t seq, ack, window, flags9, len;
    bool admitted;  // by the delivery
};
FS_CO_HD uint32_t flags9_of(uint32_t dword12) { return ((dword12 & 1u) << 8) | ((dword12 >> 8) & 0xFFu); }
FS_CO_HD uint32_t window_of(uint32_t dword12) { return ((dword12 >> 8) & 0xFF00u) | (dword12 >> 24); }
FS_CO_HD bool pure(const Frame& f) { return f.len == 0 && !(f.flags9 & kFin); }

// The code of a frame before `stop` (include/framesum_recv.h) that meets snd.UNA = una and rcv.NXT = nxt_k.
FS_CO_HD uint32_t code_of(uint32_t una, uint32_t nxt_k, uint32_t snd_nxt, uint32_t rcv_wnd, const Frame& f) {
    const bool ack = (f.flags9 & kAck) != 0;
    if (pure(f)) {
        if (f.seq == nxt_k - 1u && f.flags9 == kAck && f.ack == snd_nxt) return kKeepalive;
        if (f.seq != nxt_k) return kRejected;
        if (ack && !less_than(una, f.ack)) return kDuplicate;
        if (ack && !less_than_eq(f.ack, snd_nxt)) return kUnsent;
        return kTaken;
    }
    if (f.admitted) return kTaken;
    const uint32_t fin = (f.flags9 & kFin) ? 1u : 0u;
    if (f.seq != nxt_k || f.len + fin > rcv_wnd) return kRejected;  // (a), (b)
    if (ack && !less_than_eq(f.ack, snd_nxt)) return kUnsent;       // (c)
    return kRingFull;                                               // (d)
}

// The send state behind a frame of code `code`.
struct Snd {
    uint32_t una, wnd;
};
FS_CO_HD Snd step(Snd s, uint32_t code, const Frame& f) {
    if (code == kTaken) {
        s.wnd = f.window;
        if (f.flags9 & kAck) s.una = f.ack;
    }
    return s;
}
FS_CO_HD bool owes_ack(uint32_t code, const Frame& f) { return code == kUnsent || (code == kTaken && !pure(f)); }

// ---- The scan operator. snd.UNA is measured as the distance d = snd_nxt - una, in [0, 2^31] (the
// check above, and every Ack that is taken lies in that range). What a frame does to d does not depend
// on the frames before it, since rcv.NXT comes from the delivery:
//   a pure frame that passes the Seq test and whose Ack is no newer than snd_nxt:  d -> min(d, d_ack)
//   an admitted frame with ACK:                                                    d -> d_ack
//   every other frame:                                                             d -> d
// Fn{set, v} stands for d -> set ? v : min(d, v); the family is closed under composition: a later
// constant wins, otherwise the mins combine.
struct Fn {
    uint32_t set, v;
};
FS_CO_HD Fn identity() { return Fn{0u, 0xFFFFFFFFu}; }
FS_CO_HD uint32_t apply(const Fn& f, uint32_t d) { return f.set ? f.v : (d < f.v ? d : f.v); }
// f first, then g
FS_CO_HD Fn compose(const Fn& f, const Fn& g) { return g.set ? g : Fn{f.set, f.v < g.v ? f.v : g.v}; }
FS_CO_HD Fn fn_of(uint32_t nxt_k, uint32_t snd_nxt, const Frame& f) {
    if (!(f.flags9 & kAck)) return identity();
    const uint32_t d_ack = snd_nxt - f.ack;
    if (pure(f)) return (f.seq == nxt_k && d_ack <= kHalf) ? Fn{0u, d_ack} : identity();
    return f.admitted ? Fn{1u, d_ack} : identity();
}
// The same scan as a plain minimum, which any wave scan computes in any operand order: a lane's key
// is (64 - the count of constants among the lanes up to and including it) above its v. The smallest
// key up to a lane then comes from behind the latest constant, and its low word is the minimum of the
// v's from that constant on: the composition's {set, v}.
constexpr uint64_t kKeyIdentity = (64ull << 32) | 0xFFFFFFFFull;
FS_CO_HD uint64_t scan_key(const Fn& f, uint32_t constants) { return ((uint64_t)(64u - constants) << 32) | f.v; }
FS_CO_HD Fn fn_of_key(uint64_t key) { return Fn{(uint32_t)(key >> 32) != 64u ? 1u : 0u, (uint32_t)key}; }
// The one point at which min() is not the literal rule: an Ack exactly 2^31 behind snd_nxt compares as
// NEWER than una == snd_nxt (LessThan is an order only strictly inside half the number space). The
// walk steps through a chunk that holds such a frame one frame at a time.
FS_CO_HD bool at_half(uint32_t nxt_k, uint32_t snd_nxt, const Frame& f) {
    return pure(f) && (f.flags9 & kAck) && f.seq == nxt_k && snd_nxt - f.ack == kHalf;
}

// What snd_out[s] holds for a socket whose flow is not in the batch (and for every socket when n is 0).
FS_CO_HD fs_rx_snd_out untouched(uint32_t snd_una, uint32_t snd_wnd) {
    fs_rx_snd_out o;
    o.snd_una = snd_una, o.snd_wnd = snd_wnd;
    o.n_taken = o.n_dup = o.n_unsent = o.n_rejected = o.n_keepalive = o.flags = 0;
    return o;
}

}  // namespace recv
}  // namespace framesum
