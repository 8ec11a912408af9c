/*
 * framesum -- ARP requests answered and replies matched in one call (C ABI, ninth header beside framesum.h,
 * framesum_deliver.h, framesum_send.h, framesum_recv.h, framesum_accept.h, framesum_close.h,
 * framesum_connect.h and framesum_udp.h).
 *
 * fs_arp_flows_batch is fs_udp_flows_batch plus the ARP branch of PortStack.RecvEth: every ARP request for
 * the address of a listed HOST (a local interface) gets its reply built in one of the host's reply slots,
 * every ARP reply is matched to a listed QUERY (a resolution in progress), and every query flagged to be
 * sent has its who-has frame built. With it one RX call per batch serves every branch of RecvEth, and two
 * endpoints that know only each other's IPv4 address can start a connection through the library alone.
 *
 * The reference code this restates: the MAC filter and the ARP branch of RecvEth
 * (stacks/portstack.go:185, 191-197) and arpClient (stacks/arp.go): recv (:134-166), handle (:98-132) and
 * BeginResolve (:60-76).
 *
 * 1. Relation to fs_udp_flows_batch. This call runs that call's enqueue unchanged and adds launches behind
 *    it. Everything that call writes is byte for byte what it writes for the same arguments. With
 *    n_hosts == 0 (then n_queries is 0 too: a query names a host) the only addition is one launch that
 *    fills arp_code (rules 2 to 4: 0, FS_ARP_UNSUPPORTED, or FS_ARP_IGNORED for a supported frame, which
 *    no host can match) and arp_of (FS_ARP_NONE), where given.
 *
 * 2. Candidates. Only frames whose verdict is FS_ARP are candidates: EtherType 0x0806 and at least 42 bytes
 *    (a shorter one is FS_ERR_PACKET_SMOL already, :192-194). Every other frame gets arp_code 0 and arp_of
 *    FS_ARP_NONE. Of a candidate only the Ethernet destination frame[0:6) and the ARP header frame[14:42)
 *    are read; trailing padding is ignored.
 *
 * 3. Support check (arp.go:135-137, 159-160). A candidate gets FS_ARP_UNSUPPORTED unless HardwareType is 1,
 *    ProtoType 0x0800, HardwareLength 6, ProtoLength 4 and Operation 1 or 2.
 *
 * 4. Request (Operation 1, :139-150). The frame matches host h iff hosts[h].ip == ProtoTarget (literally:
 *    0.0.0.0 is an address, not a wildcard, as `ahdr.ProtoTarget != c.stack.ip` has it) and the Ethernet
 *    destination is ff:ff:ff:ff:ff:ff or hosts[h].mac (the MAC filter of :185, applied here because this
 *    call owns the answer). An unmatched request gets FS_ARP_IGNORED. The matched requests of a host are
 *    taken in ascending batch index; the r-th (r from 0) is answered iff r < free, its reply goes to slot
 *    slot0 + r, its arp_code is FS_ARP_ANSWERED and its arp_of the slot. The other matched requests get
 *    FS_ARP_FULL (the reference drops a request while pendingReplyToARP()). The reply is what `handle`
 *    emits for the inverted header (:113-123, 143-150): Ethernet destination = the request's
 *    HardwareSender, source = the host's MAC, EtherType 0x0806; HardwareType 1, ProtoType 0x0800,
 *    HardwareLength 6, ProtoLength 4, Operation 2; sender = the host's MAC and IP; target = the request's
 *    HardwareSender and ProtoSender.
 *
 * 5. Reply (Operation 2, :152-158). The frame matches query q iff q is not flagged FS_ARP_SEND_REQUEST,
 *    its host's IP equals ProtoTarget, its host hears the frame (the MAC filter, as in rule 4) and
 *    queries[q].target == ProtoSender. The matching reply of lowest batch index resolves the query:
 *    queries_out[q] gets state FS_ARP_Q_DONE, mac = HardwareSender and `frame`; that frame's arp_code is
 *    FS_ARP_RESOLVED. Later matches get FS_ARP_STALE (the reference checks `c.result.Operation !=
 *    arpOpWait`). Every match has arp_of q and is counted in n_replies. A reply with no matching query
 *    gets FS_ARP_IGNORED.
 *
 * 6. Requests to send (BeginResolve plus handle's first case, :60-76, 101-111). A query flagged
 *    FS_ARP_SEND_REQUEST has its who-has frame built in slot n_reply_slots + q: broadcast destination, the
 *    host's MAC as source, Operation 1, sender = the host's MAC and IP, HardwareTarget zero, ProtoTarget =
 *    target. It comes back with state FS_ARP_Q_SENT and takes no reply from this batch (the reference's
 *    result.Operation is 1, not arpOpWait, until `handle` has run). With n == 0 the flagged requests are
 *    still built, as the connect call builds the flagged SYNs.
 *
 * 7. Determinism. Nothing in the result depends on a hash, on which lane runs first, or on the grid.
 *
 * 8. Stated differences from the reference.
 *    (a) One pendingResponse becomes `free` slots; free = 1 reproduces the reference between two HandleEth
 *        polls.
 *    (b) The reference returns nil, before the support check, for a frame whose destination MAC is foreign;
 *        here a malformed one is FS_ARP_UNSUPPORTED whatever its MAC. Both drop it.
 *    (c) `c.result = *ahdr` keeps the whole header; here the MAC and the frame index come back.
 *    (d) Several hosts and several queries per call.
 *
 * 9. The frames. arp_frames is (n_reply_slots + n_queries) * FS_ACCEPT_STRIDE bytes; host h owns the slots
 *    [slot0, slot0 + free), all below n_reply_slots; query q's request goes to slot n_reply_slots + q. A
 *    frame is 42 bytes, with FS_ARP_PAD in arp_flags 60 (zero-filled to the Ethernet minimum); with
 *    FS_FCS_APPEND its CRC-32 follows little-endian, over the 42 or 60 bytes (at most 64 in all). Bytes
 *    behind the frame in its 64 are not written, and a slot that takes no frame has no byte written.
 *    arp_out[slot] and arp_status[slot] are the built frame's digest and verdict (FS_ARP unless `mtu`
 *    refuses it), as synack_out and synack_status are; a slot with no frame is left alone.
 *
 * 10. Degenerate sizes. n == 0: every hosts_out entry carries the input `free` with zero counts and first =
 *    FS_ARP_NONE, every queries_out entry FS_ARP_Q_WAIT or FS_ARP_Q_SENT; the flagged requests are built;
 *    the UDP call's n == 0 behaviour stays. n_hosts == 0: see 1.
 *
 * 11. FS_E_INVALID, checked on the host before any device work, each with a text in fs_last_error:
 *    everything fs_udp_flows_batch rejects; null hosts, hosts_out or arp_frames with n_hosts > 0; null
 *    queries, queries_out or arp_frames with n_queries > 0; n_hosts, n_queries or n_reply_slots above
 *    FS_ARP_MAX_HOSTS, FS_ARP_MAX_QUERIES, FS_ARP_MAX_REPLY_SLOTS; reserved not 0; two hosts with equal
 *    ip; a slot range past n_reply_slots; two slot ranges that overlap; queries[q].host >= n_hosts; two
 *    queries with equal (host, target); query flags other than 0 or FS_ARP_SEND_REQUEST; arp_flags outside
 *    FS_ARP_PAD | FS_FCS_APPEND.
 *
 * `hosts` and `queries` are HOST memory, consumed before the call returns (staged per call with their
 * tables in a block of their own, as the ports and the listeners are); everything else is a DEVICE
 * pointer; arp_out, arp_status (one entry per frame slot), arp_code and arp_of (n entries each) are
 * nullable. Asynchronous on `stream`; scratch rules are fs_udp_flows_batch's, and this call adds 16 bytes
 * per frame beside the sort's temporary storage, 8 per reply slot and 8 per query.
 * fs_ctx_set_workgroups caps the grids of this call's kernels too.
 */
#ifndef FRAMESUM_ARP_H
#define FRAMESUM_ARP_H

#include "framesum_udp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_ARP_NONE 0xFFFFFFFFu /* arp_of of a frame with no slot and no query; `first` and `frame` without a frame */
#define FS_ARP_MAX_HOSTS 65536u
#define FS_ARP_MAX_QUERIES 65536u
#define FS_ARP_MAX_REPLY_SLOTS 65536u
#define FS_ARP_FRAME 42u        /* a built frame's bytes */
#define FS_ARP_FRAME_PADDED 60u /* ... with FS_ARP_PAD */

#define FS_ARP_PAD 1u /* arp_flags (beside FS_FCS_APPEND = 2): zero-fill the built frames to 60 bytes */

#define FS_ARP_SEND_REQUEST 1u /* fs_arp_query.flags: build the who-has frame; the query takes no reply in this call */

enum fs_arp_code { /* arp_code */
    FS_ARP_NOT_ARP = 0,     /* the verdict is not FS_ARP */
    FS_ARP_UNSUPPORTED = 1, /* errARPUnsupported */
    FS_ARP_IGNORED = 2,     /* a request for no listed host, a reply to no listed query, or a foreign MAC */
    FS_ARP_ANSWERED = 3,    /* a request whose reply was built: arp_of is the slot */
    FS_ARP_FULL = 4,        /* a matched request beyond the host's `free` */
    FS_ARP_RESOLVED = 5,    /* the reply that resolved a query: arp_of is the query */
    FS_ARP_STALE = 6        /* a later reply to the same query: arp_of is the query */
};

enum fs_arp_q_state { FS_ARP_Q_WAIT = 0, FS_ARP_Q_DONE = 1, FS_ARP_Q_SENT = 2 }; /* fs_arp_query_out.state */

typedef struct fs_arp_host { /* 20 bytes, no padding. HOST memory */
    uint8_t ip[4];           /* wire order */
    uint8_t mac[6];          /* wire order */
    uint16_t reserved;       /* must be 0 */
    uint32_t slot0;          /* its reply slots are [slot0, slot0 + free) */
    uint32_t free;           /* the replies it may emit in this call */
} fs_arp_host;

typedef struct fs_arp_query { /* 12 bytes, no padding. HOST memory */
    uint32_t host;            /* an index into hosts */
    uint8_t target[4];        /* the address to resolve, wire order */
    uint16_t flags;           /* 0 or FS_ARP_SEND_REQUEST */
    uint16_t reserved;        /* must be 0 */
} fs_arp_query;

typedef struct fs_arp_host_out { /* 16 bytes. DEVICE memory, every entry written */
    uint32_t n_requests;         /* the matched requests */
    uint32_t n_answered;         /* min(n_requests, free) */
    uint32_t first;              /* batch index of the first matched request, else FS_ARP_NONE */
    uint32_t free;               /* after the call */
} fs_arp_host_out;

typedef struct fs_arp_query_out { /* 16 bytes, no padding. DEVICE memory, every entry written */
    uint8_t state;                /* fs_arp_q_state */
    uint8_t reserved;             /* 0 */
    uint8_t mac[6];               /* HardwareSender of the resolving reply, else zero */
    uint32_t frame;               /* batch index of the reply that resolved it, else FS_ARP_NONE */
    uint32_t n_replies;           /* all replies that matched it */
} fs_arp_query_out;

fs_status fs_arp_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                             uint32_t n, uint32_t mtu, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks,
                             uint8_t* rings, uint64_t rings_bytes, fs_rx_sock_out* socks_out, uint8_t* delivered,
                             const fs_rx_snd* snd, fs_rx_snd_out* snd_out, uint8_t* code, const fs_listener* listeners,
                             uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots, uint32_t synack_flags,
                             fs_accept_conn* conns, fs_listener_out* listeners_out, uint32_t* accept_of,
                             uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status, const fs_cl_sock* closers,
                             uint32_t n_closers, fs_cl_out* closers_out, fs_cl_out* socks_close, uint8_t* ctl_code,
                             const fs_cn_sock* openers, uint32_t n_openers, uint32_t reply_flags, fs_cn_out* openers_out,
                             uint8_t* replies, fs_digest* reply_out, uint8_t* reply_status,
                             const fs_udp_port* ports, uint32_t n_ports, uint8_t* cells, uint64_t cells_bytes,
                             fs_udp_port_out* ports_out, uint32_t* port_of, uint32_t* cell_of,
                             const fs_arp_host* hosts, uint32_t n_hosts, const fs_arp_query* queries, uint32_t n_queries,
                             uint32_t n_reply_slots, uint32_t arp_flags, fs_arp_host_out* hosts_out,
                             fs_arp_query_out* queries_out, uint8_t* arp_frames, fs_digest* arp_out, uint8_t* arp_status,
                             uint8_t* arp_code, uint32_t* arp_of,
                             uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order,
                             uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, void* stream);

/* fs_arp_flows_batch with every pointer in HOST memory, as fs_udp_flows_batch_host: arp_frames, arp_out and
 * arp_status go to the device first and come back whole (a slot without a frame keeps the caller's bytes);
 * hosts_out, queries_out, arp_code and arp_of come back whole. */
fs_status fs_arp_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                                  const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags,
                                  const fs_rx_sock* socks, uint32_t n_socks, uint8_t* rings, uint64_t rings_bytes,
                                  fs_rx_sock_out* socks_out, uint8_t* delivered, const fs_rx_snd* snd,
                                  fs_rx_snd_out* snd_out, uint8_t* code, const fs_listener* listeners,
                                  uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots,
                                  uint32_t synack_flags, fs_accept_conn* conns, fs_listener_out* listeners_out,
                                  uint32_t* accept_of, uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status,
                                  const fs_cl_sock* closers, uint32_t n_closers, fs_cl_out* closers_out,
                                  fs_cl_out* socks_close, uint8_t* ctl_code, const fs_cn_sock* openers,
                                  uint32_t n_openers, uint32_t reply_flags, fs_cn_out* openers_out, uint8_t* replies,
                                  fs_digest* reply_out, uint8_t* reply_status, const fs_udp_port* ports, uint32_t n_ports,
                                  uint8_t* cells, uint64_t cells_bytes, fs_udp_port_out* ports_out, uint32_t* port_of,
                                  uint32_t* cell_of, const fs_arp_host* hosts, uint32_t n_hosts,
                                  const fs_arp_query* queries, uint32_t n_queries, uint32_t n_reply_slots,
                                  uint32_t arp_flags, fs_arp_host_out* hosts_out, fs_arp_query_out* queries_out,
                                  uint8_t* arp_frames, fs_digest* arp_out, uint8_t* arp_status, uint8_t* arp_code,
                                  uint32_t* arp_of, uint8_t* payload, uint64_t payload_cap,
                                  fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order, uint32_t* run_of,
                                  fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status);

#ifdef __cplusplus
}
#endif
#endif /* FRAMESUM_ARP_H */
