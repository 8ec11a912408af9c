// Arithmetic of the close call (fs_close_flows_batch, include/framesum_close.h), free of HIP like
// framesum_recv.h and framesum_accept.h, on which it builds: the checks of the closer list (which build
// the closer table: flows::build_table, staged with the records), the rule
// of one frame under one state (code_of, step), what makes a frame an event of the walk, and the out
// records. framesum_close.hip runs exactly this code per frame, and tests/csrc/test_close.cpp builds it
// alone under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/framesum_close.h"
#include "framesum_accept.h"

namespace framesum {
namespace closing {

using namespace recv;

static_assert(sizeof(fs_cl_sock) == 40 && offsetof(fs_cl_sock, state) == 13 && offsetof(fs_cl_sock, rcv_nxt) == 16 &&
                  offsetof(fs_cl_sock, reserved2) == 36,
              "fs_cl_sock is 40 bytes with no padding");
static_assert(sizeof(fs_cl_out) == 32 && offsetof(fs_cl_out, flags) == 28, "fs_cl_out is 32 bytes with no padding");

constexpr uint32_t kMaxClosers = FS_CLOSE_MAX_CLOSERS;
enum State : uint32_t {
    kClosed = FS_ST_CLOSED, kEstablished = FS_ST_ESTABLISHED, kFinWait1 = FS_ST_FIN_WAIT_1, kFinWait2 = FS_ST_FIN_WAIT_2,
    kClosing = FS_ST_CLOSING, kTimeWait = FS_ST_TIME_WAIT, kCloseWait = FS_ST_CLOSE_WAIT, kLastAck = FS_ST_LAST_ACK,
};
// The codes of ctl_code (1, 4 and 5 are the receive call's), and what code_of gives a frame with SYN:
// no code of the ABI, the walk ends in front of that frame.
constexpr uint32_t kCodeData = FS_CL_DATA, kCodeIgnored = FS_CL_IGNORED, kCodeRst = FS_CL_RST, kCodeExpected = FS_CL_EXPECTED;
constexpr uint32_t kEnds = 0xFFu;

// ---- The checks of the closer list (rule 7 of the header), none of which needs a device.
enum BadClose {
    kCloseGood = 0, kCloseNull, kTooManyClosers, kCloseState, kCloseKeyNotTcp, kCloseReserved, kCloseEqualKeys,
    kCloseKeyListed, kCloseSndWnd,
};
inline const char* bad_close_text(BadClose b) {
    switch (b) {
    case kCloseNull: return "null closers, closers_out or socks_close";
    case kTooManyClosers: return "n_closers above 65,536";
    case kCloseState: return "state must be 5 .. 10";
    case kCloseKeyNotTcp: return "key[0] must be 6 (TCP)";
    case kCloseReserved: return "reserved must be 0";
    case kCloseEqualKeys: return "its key equals an earlier closer's";
    case kCloseKeyListed: return "its key equals a listed socket's";
    case kCloseSndWnd: return "snd_wnd above 65,535";
    default: return "";
    }
}
struct CheckClose {
    BadClose bad;
    uint32_t index;  // the closer `bad` is about
};
// `socks`, `n_socks`, `sock_table`: the socket list, which has passed deliver::check_socks (its table
// built under the same hash_mask). `table`: resized and filled for the staged block when the list is good.
inline CheckClose check_closers(const fs_cl_sock* closers, uint32_t n_closers, bool have_out, bool have_socks_close,
                                const fs_rx_sock* socks, uint32_t n_socks, const uint32_t* sock_table, uint32_t hash_mask,
                                std::vector<uint32_t>& table) {
    if (n_closers > kMaxClosers) return CheckClose{kTooManyClosers, 0u};
    if (n_closers != 0 && (!closers || !have_out)) return CheckClose{kCloseNull, 0u};
    if (n_socks != 0 && !have_socks_close) return CheckClose{kCloseNull, 0u};
    for (uint32_t i = 0; i < n_closers; ++i) {
        const fs_cl_sock& c = closers[i];
        if (c.state < kFinWait1 || c.state > kLastAck) return CheckClose{kCloseState, i};
        if (c.key[0] != 6) return CheckClose{kCloseKeyNotTcp, i};
        if (c.reserved[0] | c.reserved[1] | c.reserved2) return CheckClose{kCloseReserved, i};
        if (c.snd_wnd > kMaxWnd) return CheckClose{kCloseSndWnd, i};
    }
    table.resize(table_slots(n_closers));
    const uint32_t dup = build_table(closers, n_closers, hash_mask, table.data());
    if (dup != kNone) return CheckClose{kCloseEqualKeys, dup};
    for (uint32_t i = 0; n_socks != 0 && i < n_closers; ++i)
        if (lookup(wire_key(closers[i].key), socks, sock_table, table_slots(n_socks) - 1u, hash_mask) != kNone)
            return CheckClose{kCloseKeyListed, i};
    return CheckClose{kCloseGood, 0u};
}

// What of a connection does not change during a walk.
struct Fixed {
    uint32_t snd_nxt, rcv_wnd;
};
// The staged block of a call: the closer records as the caller gave them, their table, and what the
// continuations read of the listed sockets.
struct Block {
    uint64_t table, socks, bytes;
};
inline Block block_of(uint32_t n_closers, uint32_t n_socks) {
    Block b;
    b.table = (uint64_t)n_closers * sizeof(fs_cl_sock);
    b.socks = b.table + 4ull * table_slots(n_closers);
    b.bytes = b.socks + (uint64_t)n_socks * sizeof(Fixed);
    return b;
}
inline void stage(const fs_cl_sock* closers, uint32_t n_closers, const uint32_t* table, const fs_rx_sock* socks,
                  uint32_t n_socks, const Block& b, uint8_t* dst) {
    if (n_closers) memcpy(dst, closers, b.table);
    memcpy(dst + b.table, table, b.socks - b.table);
    for (uint32_t i = 0; i < n_socks; ++i) {
        const Fixed x{socks[i].snd_nxt, socks[i].rcv_wnd};
        memcpy(dst + b.socks + (uint64_t)i * sizeof(Fixed), &x, sizeof x);
    }
}

// ---- One frame as the walk reads it (flags9_of and window_of: framesum_recv.h).
struct Seg {
    uint32_t seq, ack, window, flags9, len;
};
// What of a connection changes during a walk.
struct Ctl {
    uint32_t state, nxt, una, wnd, flags;
};

// InWindow (valuesize.go:37-45).
FS_CO_HD bool in_window(uint32_t v, uint32_t first, uint32_t size) { return v - first < size; }
// The Seq checks of control.go:299-311 for a segment without data (DATALEN 0, LEN() = the FIN bit),
// case by case.
FS_CO_HD bool seq_checks_pass(uint32_t nxt, uint32_t rcv_wnd, const Seg& f) {
    const uint32_t seglen = (f.flags9 & kFin) ? 1u : 0u;
    const uint32_t last = seglen == 0u ? f.seq : f.seq + seglen - 1u;  // seqs.go:26-32
    const bool zero_window_ok = rcv_wnd == 0u && f.seq == nxt;         // control.go:291 (DATALEN is 0)
    // :299 needs DATALEN > 0
    if (!in_window(f.seq, nxt, rcv_wnd) && !zero_window_ok) return false;  // :302
    if (!in_window(last, nxt, rcv_wnd) && !zero_window_ok) return false;   // :305
    if (f.seq != nxt) return false;                                        // :308
    return true;
}
// The state behind a frame that rule 7 judges under `state`, or kEnds when the state refuses it (code 10).
FS_CO_HD uint32_t rule7_state(uint32_t state, uint32_t snd_nxt, const Seg& f) {
    const bool fin = (f.flags9 & kFin) != 0, ack = (f.flags9 & kAck) != 0;
    switch (state) {
    case kFinWait1:
        if (fin && ack && f.ack == snd_nxt) return kTimeWait;
        if (fin) return kClosing;
        if (ack) return kFinWait2;
        return kEnds;
    case kFinWait2: return fin && ack ? (uint32_t)kTimeWait : kEnds;
    case kClosing: return ack ? (uint32_t)kTimeWait : (uint32_t)kClosing;
    case kLastAck: return ack ? (uint32_t)kClosed : (uint32_t)kLastAck;
    default: return state;  // CloseWait
    }
}
// The code of a frame that meets `state` and rcv.NXT = nxt: the first rule that applies. kEnds: rule 2.
FS_CO_HD uint32_t code_of(uint32_t state, uint32_t nxt, const Fixed& x, const Seg& f) {
    if (state == kTimeWait || state == kClosed) return kCodeIgnored;                                         // rule 1
    if (f.flags9 & kSyn) return kEnds;                                                                   // rule 2
    if (f.seq == nxt - 1u && f.flags9 == kAck && f.ack == x.snd_nxt && f.len == 0u) return kKeepalive;  // rule 3
    if (f.len > 0u) return kCodeData;                                                                        // rule 4
    if (!seq_checks_pass(nxt, x.rcv_wnd, f)) return kRejected;                                           // rule 5
    if (f.flags9 & kRst) return kCodeRst;                                                                   // rule 6
    return rule7_state(state, x.snd_nxt, f) == kEnds ? kCodeExpected : (uint32_t)kTaken;                     // rule 7
}
// Whether a frame of code `code` changes the state or rcv.NXT: the walk decides the frames between two
// such frames at once.
FS_CO_HD bool is_event(uint32_t state, uint32_t code, const Fixed& x, const Seg& f) {
    if (code == kCodeRst || code == kEnds) return true;
    return code == kTaken && ((f.flags9 & kFin) != 0 || rule7_state(state, x.snd_nxt, f) != state);
}
// The connection behind a frame of code `code` (not kEnds).
FS_CO_HD Ctl step(Ctl c, uint32_t code, const Fixed& x, const Seg& f) {
    if (code == kCodeRst) {
        c.state = kClosed, c.flags |= FS_CL_RESET;
    } else if (code == kTaken) {
        const uint32_t next = rule7_state(c.state, x.snd_nxt, f);
        if ((c.state == kFinWait1 || c.state == kFinWait2) && next != c.state) c.flags |= FS_CL_ACK_OWED;
        c.state = next;
        c.wnd = f.window;
        if (f.flags9 & kAck) c.una = f.ack;
        if (f.flags9 & kFin) c.nxt += 1u, c.flags |= FS_CL_FIN;
    }
    return c;
}
FS_CO_HD bool counts_rejected(uint32_t code) { return code == kRejected || code == kCodeData || code == kCodeExpected; }

// ---- The out records. `stop`: kNone for a connection without a flow in the batch.
FS_CO_HD fs_cl_out out_of(const Ctl& c, uint32_t n_taken, uint32_t n_rejected, uint32_t stop) {
    fs_cl_out o;
    const bool closed = c.state == kClosed;
    o.state = c.state;
    o.rcv_nxt = closed ? 0u : c.nxt, o.snd_una = closed ? 0u : c.una, o.snd_wnd = closed ? 0u : c.wnd;
    o.n_taken = n_taken, o.n_rejected = n_rejected, o.stop = stop, o.flags = c.flags;
    return o;
}
FS_CO_HD Ctl ctl_of(const fs_cl_sock& s) { return Ctl{s.state, s.rcv_nxt, s.snd_una, s.snd_wnd, 0u}; }
FS_CO_HD fs_cl_out untouched_closer(const fs_cl_sock& s) { return out_of(ctl_of(s), 0u, 0u, kNone); }
// An Established socket the continuation does not touch: the numbers as the receive call left them.
FS_CO_HD fs_cl_out untouched_sock(uint32_t rcv_nxt, uint32_t snd_una, uint32_t snd_wnd, uint32_t stop) {
    return out_of(Ctl{kEstablished, rcv_nxt, snd_una, snd_wnd, 0u}, 0u, 0u, stop);
}

}  // namespace closing
}  // namespace framesum
