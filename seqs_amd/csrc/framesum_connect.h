// Arithmetic of the connect call (fs_connect_flows_batch, include/framesum_connect.h), free of HIP like
// framesum_close.h, on which it builds: the checks of the opener list (which build the opener
// table: flows::build_table, staged with the records), the rule of one frame of an
// opener's flow (code_of), the event that ends a walk (apply), the reply's header template, and the out
// record. framesum_connect.hip runs exactly this code per frame, and tests/csrc/test_connect.cpp builds
// it alone under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/framesum_connect.h"
#include "framesum_close.h"

namespace framesum {
namespace connect {

using namespace recv;

static_assert(sizeof(fs_cn_sock) == 40 && offsetof(fs_cn_sock, flags) == 13 && offsetof(fs_cn_sock, local_mac) == 16 &&
                  offsetof(fs_cn_sock, remote_mac) == 22 && offsetof(fs_cn_sock, iss) == 28 && offsetof(fs_cn_sock, ip_id) == 36,
              "fs_cn_sock is 40 bytes with no padding");
static_assert(sizeof(fs_cn_out) == 48 && offsetof(fs_cn_out, frame) == 36 && offsetof(fs_cn_out, peer_mss) == 40 &&
                  offsetof(fs_cn_out, reply) == 42 && offsetof(fs_cn_out, rst_seq) == 44,
              "fs_cn_out is 48 bytes with no padding");

constexpr uint32_t kMaxOpeners = FS_CONNECT_MAX_OPENERS;
constexpr uint32_t kSynRcvd = FS_ST_SYN_RCVD, kSynSent = FS_ST_SYN_SENT, kEstablished = FS_ST_ESTABLISHED;
// The codes of ctl_code (1, 4, 5 and 10 are the close call's), and what code_of gives the frames of rules
// 3 and 4: no code of the ABI, the walk ends in front of such a frame.
constexpr uint32_t kCodeExpected = FS_CL_EXPECTED, kCodeBadAck = FS_CN_BAD_ACK;
constexpr uint32_t kEndsRst = 0xFEu, kEndsSyn = 0xFFu;
constexpr uint32_t kOpenWnd = 1u;  // snd.WND of a block Open has made (control_user.go:64)

// ---- The checks of the opener list (section 6 of the header), none of which needs a device.
enum BadConnect {
    kConnectGood = 0, kConnectNull, kTooManyOpeners, kReplyFlags, kConnectFlags, kConnectKeyNotTcp, kConnectReserved,
    kConnectEqualKeys, kConnectKeyListed, kConnectKeyCloser,
};
inline const char* bad_connect_text(BadConnect b) {
    switch (b) {
    case kConnectNull: return "null openers, openers_out or replies";
    case kTooManyOpeners: return "n_openers above 65,536";
    case kReplyFlags: return "reply_flags must be 0 or FS_FCS_APPEND";
    case kConnectFlags: return "flags must be 0 or FS_CN_SEND_SYN";
    case kConnectKeyNotTcp: return "key[0] must be 6 (TCP)";
    case kConnectReserved: return "reserved must be 0";
    case kConnectEqualKeys: return "its key equals an earlier opener's";
    case kConnectKeyListed: return "its key equals a listed socket's";
    case kConnectKeyCloser: return "its key equals a closer's";
    default: return "";
    }
}
struct CheckConnect {
    BadConnect bad;
    uint32_t index;  // the opener `bad` is about
};
// `socks`, `sock_table` and `closers`, `closer_table`: the lists that have passed deliver::check_socks and
// closing::check_closers (their tables built under the same hash_mask). `table`: resized and filled for
// the staged block when the list is good.
inline CheckConnect check_openers(const fs_cn_sock* openers, uint32_t n_openers, uint32_t reply_flags, bool have_out,
                                  bool have_replies, const fs_rx_sock* socks, uint32_t n_socks, const uint32_t* sock_table,
                                  const fs_cl_sock* closers, uint32_t n_closers, const uint32_t* closer_table,
                                  uint32_t hash_mask, std::vector<uint32_t>& table) {
    if (n_openers > kMaxOpeners) return CheckConnect{kTooManyOpeners, 0u};
    if (reply_flags & ~(uint32_t)FS_FCS_APPEND) return CheckConnect{kReplyFlags, 0u};
    if (n_openers != 0 && (!openers || !have_out || !have_replies)) return CheckConnect{kConnectNull, 0u};
    for (uint32_t i = 0; i < n_openers; ++i) {
        const fs_cn_sock& c = openers[i];
        if (c.flags & ~(uint32_t)FS_CN_SEND_SYN) return CheckConnect{kConnectFlags, i};
        if (c.key[0] != 6) return CheckConnect{kConnectKeyNotTcp, i};
        if (c.reserved[0] | c.reserved[1] | c.reserved2) return CheckConnect{kConnectReserved, i};
    }
    table.resize(table_slots(n_openers));
    const uint32_t dup = build_table(openers, n_openers, hash_mask, table.data());
    if (dup != kNone) return CheckConnect{kConnectEqualKeys, dup};
    for (uint32_t i = 0; i < n_openers; ++i) {
        const Key key = wire_key(openers[i].key);
        if (n_socks != 0 && lookup(key, socks, sock_table, table_slots(n_socks) - 1u, hash_mask) != kNone)
            return CheckConnect{kConnectKeyListed, i};
        if (n_closers != 0 && lookup(key, closers, closer_table, table_slots(n_closers) - 1u, hash_mask) != kNone)
            return CheckConnect{kConnectKeyCloser, i};
    }
    return CheckConnect{kConnectGood, 0u};
}

// The staged block of a call: the opener records as the caller gave them, then their table.
struct Block {
    uint64_t table, bytes;
};
inline Block block_of(uint32_t n_openers) {
    Block b;
    b.table = (uint64_t)n_openers * sizeof(fs_cn_sock);
    b.bytes = b.table + 4ull * table_slots(n_openers);
    return b;
}
inline void stage(const fs_cn_sock* openers, uint32_t n_openers, const uint32_t* table, const Block& b, uint8_t* dst) {
    if (n_openers) memcpy(dst, openers, b.table);
    memcpy(dst + b.table, table, b.bytes - b.table);
}

// ---- One frame as the walk reads it (flags9_of and window_of: framesum_recv.h).
using Seg = closing::Seg;

// The Seq checks of control.go:299-311 with rcv.NXT = 0 and LEN = len + FIN (SYN is clear), case by case.
FS_CO_HD bool seq_checks_pass(uint32_t rcv_wnd, const Seg& f) {
    const uint32_t seglen = f.len + ((f.flags9 & kFin) ? 1u : 0u);
    const uint32_t last = seglen == 0u ? f.seq : f.seq + seglen - 1u;        // seqs.go:26-32
    const bool zero_window_ok = rcv_wnd == 0u && f.len == 0u && f.seq == 0u;  // control.go:291
    if (rcv_wnd == 0u && f.len > 0u && f.seq == 0u) return false;                     // :299
    if (!closing::in_window(f.seq, 0u, rcv_wnd) && !zero_window_ok) return false;    // :302
    if (!closing::in_window(last, 0u, rcv_wnd) && !zero_window_ok) return false;     // :305
    if (f.seq != 0u) return false;                                                    // :308
    return true;
}
// acksOld || acksUnsentData (control.go:288-289) with snd.UNA = iss and snd.NXT = iss + 1, literally.
FS_CO_HD bool bad_ack(uint32_t iss, uint32_t ack) { return !less_than(iss, ack) || !less_than_eq(ack, iss + 1u); }

// The code of a frame of an opener's flow: the first rule that applies. kEndsRst: rule 3, kEndsSyn: rule 4.
FS_CO_HD uint32_t code_of(uint32_t iss, uint32_t rcv_wnd, const Seg& f) {
    const bool syn = (f.flags9 & kSyn) != 0, ack = (f.flags9 & kAck) != 0;
    if (f.seq == 0xFFFFFFFFu && f.flags9 == kAck && f.ack == iss + 1u && f.len == 0u) return kKeepalive;  // rule 1
    if (!syn && !seq_checks_pass(rcv_wnd, f)) return kRejected;                                           // rule 2
    if (f.flags9 & kRst) return kEndsRst;                                                                 // rule 3
    if (syn && (f.len > 0u || (f.flags9 & ~(kSyn | kAck)) != 0u)) return kEndsSyn;                        // rule 4
    if (ack && bad_ack(iss, f.ack)) return kCodeBadAck;                                                   // rule 5
    if (!syn) return kCodeExpected;                                                                       // rule 6
    return kTaken;                                                                                        // rules 7 and 8
}
// Whether a frame of code `code` ends the walk (in front of it, or behind it).
FS_CO_HD bool is_event(uint32_t code) { return code == kEndsRst || code == kEndsSyn || code == kCodeBadAck || code == kTaken; }
FS_CO_HD bool counts_rejected(uint32_t code) { return code == kRejected || code == kCodeExpected; }

// ---- The out record. The one of an opener no frame has changed:
FS_CO_HD fs_cn_out untouched(const fs_cn_sock& s) {
    fs_cn_out o;
    o.state = kSynSent;
    o.irs = 0u, o.rcv_nxt = 0u;
    o.snd_una = s.iss, o.snd_nxt = s.iss + 1u, o.snd_wnd = kOpenWnd;
    o.n_rejected = 0u, o.n_keepalive = 0u;
    o.stop = kNone, o.frame = kNone;
    o.peer_mss = 0, o.reply = FS_CN_REPLY_NONE, o.flags = 0;
    o.rst_seq = 0u;
    return o;
}
// The record behind the event frame `f` of code `code` at slot `slot` (batch index `frame`; `mss`: the
// option walk's value for a frame of code 1). The counts and, for a walk that reached the flow's end,
// `stop` are the caller's.
FS_CO_HD fs_cn_out apply(fs_cn_out o, const fs_cn_sock& s, uint32_t code, const Seg& f, uint32_t slot, uint32_t frame,
                         uint32_t mss) {
    if (code == kEndsRst || code == kEndsSyn) {
        o.stop = slot;
        o.flags = (uint8_t)(code == kEndsRst ? FS_CN_STOP_RST : FS_CN_STOP_SYN);
        return o;
    }
    o.stop = slot + 1u;
    o.frame = frame;
    o.snd_wnd = f.window;
    if (code == kCodeBadAck) {  // control.go:341-345
        o.reply = FS_CN_REPLY_RST, o.rst_seq = f.ack;
        o.snd_una = o.snd_nxt = s.iss;
        return o;
    }
    // code 1: control.go:189-199, then control_user.go:211-217
    o.irs = f.seq, o.rcv_nxt = f.seq + 1u;
    o.peer_mss = (uint16_t)mss;
    if (f.flags9 & kAck) {
        o.state = kEstablished, o.reply = FS_CN_REPLY_ACK;
        o.snd_una = f.ack, o.snd_nxt = s.iss + 1u;
    } else {
        o.state = kSynRcvd, o.reply = FS_CN_REPLY_SYNACK;
        o.snd_una = o.snd_nxt = s.iss;
    }
    return o;
}
// handleInitSyn's frame for an opener that owes nothing else.
FS_CO_HD fs_cn_out with_syn(fs_cn_out o, const fs_cn_sock& s) {
    if (o.reply == FS_CN_REPLY_NONE && (s.flags & FS_CN_SEND_SYN)) o.reply = FS_CN_REPLY_SYN;
    return o;
}

// The reply's 54 header bytes as the frame body takes a template (framesum_tx_dev.h), in the manner of
// accept::synack_template: everything but TotalLength, the ID and the two checksums, which the body
// writes. Bytes 18, 19 carry the ID seed. `o.reply` is not FS_CN_REPLY_NONE.
FS_CO_HD void reply_template(const fs_cn_sock& s, const fs_cn_out& o, uint8_t h[54]) {
    for (uint32_t i = 0; i < 54; ++i) h[i] = 0;
    for (uint32_t i = 0; i < 6; ++i) h[i] = s.remote_mac[i], h[6 + i] = s.local_mac[i];
    h[12] = 0x08, h[13] = 0x00;
    h[14] = 0x45;
    h[18] = (uint8_t)(s.ip_id >> 8), h[19] = (uint8_t)s.ip_id;
    h[22] = 64, h[23] = 6;
    for (uint32_t i = 0; i < 4; ++i) h[26 + i] = s.key[5 + i], h[30 + i] = s.key[1 + i];
    h[34] = s.key[11], h[35] = s.key[12];  // ports swapped
    h[36] = s.key[9], h[37] = s.key[10];
    uint32_t seq = s.iss, ack = 0u, flags = kSyn;  // FS_CN_REPLY_SYN
    if (o.reply == FS_CN_REPLY_ACK) seq = s.iss + 1u, ack = o.irs + 1u, flags = kAck;
    else if (o.reply == FS_CN_REPLY_SYNACK) ack = o.irs + 1u, flags = kSyn | kAck;
    else if (o.reply == FS_CN_REPLY_RST) seq = o.rst_seq, flags = kRst;
    accept::put_be32(h + 38, seq);
    accept::put_be32(h + 42, ack);
    h[46] = 0x50;
    h[47] = (uint8_t)flags;
    const uint32_t wnd = s.rcv_wnd > kMaxWnd ? kMaxWnd : s.rcv_wnd;  // (the reference: uint16(rcv.WND))
    h[48] = (uint8_t)(wnd >> 8), h[49] = (uint8_t)wnd;
}

}  // namespace connect
}  // namespace framesum
