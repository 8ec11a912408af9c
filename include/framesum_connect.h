/*
 * framesum -- the active open of a TCP connection in one call (C ABI, seventh header beside framesum.h,
 * framesum_deliver.h, framesum_send.h, framesum_recv.h, framesum_accept.h and framesum_close.h).
 *
 * fs_connect_flows_batch is fs_close_flows_batch plus the receive side of SynSent: for every listed
 * OPENER (a connection whose ControlBlock has sent, or is about to send, its SYN) it walks the frames of
 * the opener's flow, returns the state the ControlBlock is in behind them and builds the one control
 * frame the opener owes: the handshake's ACK, the SYN-ACK of a simultaneous open, the RST that refuses a
 * bad Ack, or the SYN itself. With it both ends of a connection run on the library; what stays on the
 * host is the timers and per-socket arithmetic.
 *
 * The reference code this restates: rcvSynSent (control.go:175-201), validateIncomingSegment
 * (control.go:281-351), resetSnd / resetRcv (control.go:263-279), Recv's update (control_user.go:211-217),
 * Open (control_user.go:49-71), IncomingIsKeepalive (control_user.go:260-264) behind TCPConn.recv's gate
 * (stacks/tcpconn.go:349), PendingSegment (control.go:100-152), setSrcDest, handleInitSyn and
 * synsentSegment (stacks/tcpconn.go:433-450, 477-484), and the state numbers of seqs.go:175-208: Listen
 * 1, SynRcvd 2, SynSent 3, Established 4.
 *
 * 1. Relation to fs_close_flows_batch. This call runs that call's enqueue unchanged and adds launches
 *    behind it. Everything that call writes is byte for byte what it writes for the same arguments, with
 *    one exception: the ctl_code entries of frames in an opener's flow are 0 from the close call, and this
 *    call's stage writes them. The accept stage does not know the openers: a lone SYN to a listener's
 *    address in an opener's flow is a candidate there exactly as it is without this call. With n_openers
 *    == 0 no launch is added.
 *
 * 2. The records: fs_cn_sock and fs_cn_out below. An opener is a ControlBlock in SynSent: snd.UNA = iss,
 *    snd.NXT = iss + 1, rcv.NXT = 0; snd.WND is 1 until a frame sets it (Open's resetSnd(iss, 1),
 *    control_user.go:64).
 *
 * 3. The walk of an opener whose flow is in the batch. It walks the flow's slots in delivery order, the
 *    slots k of [first_frame, first_frame + n_frames) (frame order[k]). Per frame it reads what the close
 *    call's rule reads: Seq, Ack, Window, the nine flag bits and len. The state is fixed throughout: una =
 *    iss, snd_nxt = iss + 1, rcv_nxt = 0; every frame that changes the state also ends the walk. A frame
 *    gets the FIRST rule that applies; ctl_code[frame] is the rule's code:
 *
 *      rule 1  keepalive (control_user.go:260-264 with rcv.NXT = 0; tcpconn.go:349): Seq == 2^32 - 1, the
 *              nine flag bits are ACK alone, Ack == iss + 1, len == 0: code 5. Nothing changes.
 *      rule 2  SYN clear, and the Seq checks of control.go:299-311 fail with rcv.NXT = 0 and LEN = len +
 *              FIN: code 4. Nothing changes. The four cases, with Last = Seq when LEN is 0 and Seq + LEN - 1
 *              otherwise (seqs.go:26-32), and zeroWindowOK = rcv_wnd == 0 && len == 0 && Seq == 0
 *              (control.go:291):
 *                :299 fails iff rcv_wnd == 0 and len > 0 and Seq == 0.
 *                :302 fails iff Seq >= rcv_wnd (InWindow, valuesize.go:37-45) and not zeroWindowOK.
 *                :305 fails iff Last >= rcv_wnd and not zeroWindowOK.
 *                :308 fails iff Seq != 0.
 *              With Seq != 0, :308 fails if no earlier case has. With Seq == 0 and len == 0, Last is 0:
 *              both window cases pass at rcv_wnd > 0, and zeroWindowOK covers rcv_wnd 0. With Seq == 0 and
 *              len > 0, :299 fails at rcv_wnd 0, and else only :305 can fail, Last being len + FIN - 1.
 *              So a frame passes iff Seq == 0 and (len == 0, or rcv_wnd > 0 and len + FIN - 1 < rcv_wnd).
 *              (The kernels and the host-only header run the four literal cases; tests check them
 *              against this one-line form.)
 *      rule 3  RST set: the walk ENDS at this slot; `stop` is this slot, the flags get FS_CN_STOP_RST, and
 *              this frame and the frames behind it keep ctl_code 0. (Difference (a).)
 *      rule 4  SYN set, with len > 0 or with any flag bit other than SYN and ACK: the walk ENDS at this
 *              slot with FS_CN_STOP_SYN, as under rule 3. (Difference (b).)
 *      rule 5  ACK set and Ack != iss + 1: code 11. This is control.go:341-345, `acksOld ||
 *              acksUnsentData` with UNA = iss and NXT = iss + 1: acksOld is !LessThan(iss, Ack), which is
 *              clear iff Ack - iss lies in [1, 2^31] (valuesize.go:27-29: the sign of the 32-bit
 *              difference); acksUnsentData is !LessThanEq(Ack, iss + 1), which is clear iff Ack == iss + 1
 *              or Ack - (iss + 1) lies in [2^31, 2^32 - 1], that is Ack - iss in {1} or {0} or [2^31 + 1,
 *              2^32 - 1]. Both are clear only at Ack - iss == 1: only iss + 1 passes. reply = RST, rst_seq =
 *              Ack, snd_wnd = Window, snd_una = snd_nxt = iss (resetSnd, control.go:345); the state stays
 *              3. The walk ENDS behind this frame. (State difference (c).)
 *      rule 6  SYN clear: code 10 (errExpectedSYN, control.go:179). Nothing changes.
 *      rule 7  the SYN-ACK, flags exactly SYN | ACK (control.go:189-192): code 1, state 4; irs = Seq,
 *              rcv_nxt = Seq + 1, snd_una = iss + 1 (control_user.go:213-215), snd_nxt = iss + 1, snd_wnd =
 *              Window; peer_mss from the option walk of framesum_accept.h section 4; reply = ACK. The
 *              walk ENDS behind this frame: the frames after it are an Established connection's, the
 *              receive call's once the host lists the socket.
 *      rule 8  flags exactly SYN (the simultaneous open, control.go:193-199): code 1, state 2; irs = Seq,
 *              rcv_nxt = Seq + 1, snd_una = snd_nxt = iss, snd_wnd = Window; peer_mss as in rule 7; reply =
 *              SYN-ACK. The walk ENDS behind this frame. The host then lists the connection as the accept
 *              call's half-open connections are listed (framesum_accept.h section 5).
 *
 *    n_rejected counts codes 4 and 10, n_keepalive code 5. `stop` is the slot after the last frame the
 *    walk handled (first_frame + n_frames when it reached the flow's end), as fs_cl_out.stop. `frame` is the
 *    batch index of the frame of rule 5, 7 or 8, else FS_DELIVER_NONE. When no rule gave the opener a reply
 *    and FS_CN_SEND_SYN is set, reply = SYN: handleInitSyn's frame (tcpconn.go:443-450, 477-484). The
 *    3-second timer that decides when (tcpconn.go:456-459) stays on the host, which sets the flag.
 *
 *    An opener without a flow in the batch, and every opener when n is 0, gets state 3, the input numbers
 *    (snd_una = iss, snd_nxt = iss + 1, snd_wnd = 1, irs = rcv_nxt = 0), zero counts, stop = frame =
 *    FS_DELIVER_NONE, and the SYN reply if flagged. So a call with n == 0 and flagged openers builds the
 *    first SYNs of a batch of dials.
 *
 * 4. The reply goes to replies + opener * FS_ACCEPT_STRIDE: 54 bytes, or 58 with FS_FCS_APPEND in
 *    reply_flags. The remaining bytes of the 64 are not written, and no byte of an opener with reply 0 is
 *    written.
 *      Ethernet: destination remote_mac, source local_mac (setSrcDest, tcpconn.go:433-441), EtherType
 *        0x0800.
 *      IPv4: as the SYN-ACK of framesum_accept.h section 4; source is the key's destination address,
 *        destination the key's source address, ID prand16(ip_id).
 *      TCP: ports swapped from the key, data offset 5, Window = min(rcv_wnd, 65535), urgent pointer 0, and
 *        by reply kind (PendingSegment, control.go:133-141: Ack is rcv.NXT only with ACK pending, Seq is
 *        rstPtr with RST pending; synsentSegment, tcpconn.go:477-484):
 *          ACK      Seq iss + 1   Ack irs + 1   flags ACK
 *          SYN-ACK  Seq iss       Ack irs + 1   flags SYN | ACK
 *          RST      Seq rst_seq   Ack 0         flags RST
 *          SYN      Seq iss       Ack 0         flags SYN
 *    Both checksums, the FCS and the `mtu` verdict are exactly as fs_send_rings_batch writes a frame.
 *    reply_out[o] and reply_status[o] are what fs_digest_batch reports for that frame; they are written
 *    for openers with a reply only.
 *
 * 5. Differences from the reference.
 *      (a) an RST. The reference's handleRST (control.go:407-425) turns a pre-established block into a
 *          listener (Seq == 0) or queues a challenge ACK. Both are left to the host: the walk ends in
 *          front of the frame.
 *      (b) a SYN that carries data, or flag bits beside SYN and ACK. The reference would advance rcv.NXT
 *          over them (and write the bytes to the socket's ring). No ring exists yet: the walk ends in
 *          front of the frame. This is the accept call's difference for a SYN that carries data.
 *      (c) the state after rule 5. The reference is left with snd.NXT = iss. A host that resends its SYN
 *          lists the opener with the same `iss` again: the record's snd.NXT is iss + 1 once more.
 *
 * 6. FS_E_INVALID, checked on the host before any device work: everything fs_close_flows_batch rejects;
 *    null openers, openers_out or replies with n_openers > 0; n_openers above FS_CONNECT_MAX_OPENERS; flags
 *    other than 0 or FS_CN_SEND_SYN; key[0] not 6; reserved fields not 0; reply_flags other than 0 or
 *    FS_FCS_APPEND; two openers with equal keys; an opener's key equal to a listed socket's key or a
 *    closer's key.
 *
 * `openers`, like `closers`, is HOST memory, consumed before the call returns (staged per call in a block
 * of its own); openers_out, replies (n_openers * FS_ACCEPT_STRIDE bytes), reply_out and reply_status (both
 * nullable) are DEVICE pointers. Asynchronous on `stream`; scratch rules are fs_close_flows_batch's, and
 * this call adds 20 bytes per frame and 92 per opener. fs_ctx_set_workgroups caps the grids of this
 * call's kernels too.
 */
#ifndef FRAMESUM_CONNECT_H
#define FRAMESUM_CONNECT_H

#include "framesum_close.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the reference's state numbers before Established (seqs.go:175-208) */
#define FS_ST_LISTEN 1u
#define FS_ST_SYN_RCVD 2u
#define FS_ST_SYN_SENT 3u

/* ctl_code: 1, 4, 5 and 10 as the close call's (FS_CL_TAKEN, FS_CL_REJECTED, FS_CL_KEEPALIVE, FS_CL_EXPECTED) */
#define FS_CN_BAD_ACK 11u /* rule 5: the Ack is not iss + 1 */

/* fs_cn_sock.flags */
#define FS_CN_SEND_SYN 1u

/* fs_cn_out.reply */
#define FS_CN_REPLY_NONE 0u
#define FS_CN_REPLY_ACK 1u
#define FS_CN_REPLY_SYNACK 2u
#define FS_CN_REPLY_RST 3u
#define FS_CN_REPLY_SYN 4u

/* fs_cn_out.flags */
#define FS_CN_STOP_RST 1u
#define FS_CN_STOP_SYN 2u

#define FS_CONNECT_MAX_OPENERS 65536u

typedef struct fs_cn_sock {      /* 40 bytes, no padding. HOST memory. A ControlBlock in SynSent: snd.UNA = iss, snd.NXT = iss + 1, rcv.NXT = 0 */
    uint8_t key[13];             /* as fs_rx_sock.key: the key of the frames the peer sends us */
    uint8_t flags;               /* 0 or FS_CN_SEND_SYN */
    uint8_t reserved[2];         /* must be 0 */
    uint8_t local_mac[6], remote_mac[6]; /* Ethernet source / destination of every frame built for this opener (setSrcDest, tcpconn.go:433-441) */
    uint32_t iss, rcv_wnd;
    uint16_t ip_id;              /* the ID seed: frames carry prand16(ip_id), as fs_accept_slot.ip_id */
    uint16_t reserved2;          /* must be 0 */
} fs_cn_sock;

typedef struct fs_cn_out {       /* 48 bytes, no padding. DEVICE memory, all entries written */
    uint32_t state;              /* 3 SynSent, 4 Established, 2 SynRcvd (seqs.go:175-208) */
    uint32_t irs, rcv_nxt;
    uint32_t snd_una, snd_nxt, snd_wnd;
    uint32_t n_rejected;         /* codes 4 and 10 */
    uint32_t n_keepalive;        /* code 5 */
    uint32_t stop;               /* as fs_cl_out.stop */
    uint32_t frame;              /* batch index of the frame of rule 5, 7 or 8, else FS_DELIVER_NONE */
    uint16_t peer_mss;           /* as fs_accept_conn.peer_mss, from that frame; else 0 */
    uint8_t reply;               /* FS_CN_REPLY_NONE 0, _ACK 1, _SYNACK 2, _RST 3, _SYN 4 */
    uint8_t flags;               /* FS_CN_STOP_RST 1, FS_CN_STOP_SYN 2 */
    uint32_t rst_seq;            /* rule 5: the refused Ack; else 0 */
} fs_cn_out;

fs_status fs_connect_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                                 uint32_t n, uint32_t mtu, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks,
                                 uint8_t* rings, uint64_t rings_bytes, fs_rx_sock_out* socks_out, uint8_t* delivered,
                                 const fs_rx_snd* snd, fs_rx_snd_out* snd_out, uint8_t* code, const fs_listener* listeners,
                                 uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots, uint32_t synack_flags,
                                 fs_accept_conn* conns, fs_listener_out* listeners_out, uint32_t* accept_of,
                                 uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status, const fs_cl_sock* closers,
                                 uint32_t n_closers, fs_cl_out* closers_out, fs_cl_out* socks_close, uint8_t* ctl_code,
                                 const fs_cn_sock* openers, uint32_t n_openers, uint32_t reply_flags, fs_cn_out* openers_out,
                                 uint8_t* replies, fs_digest* reply_out, uint8_t* reply_status,
                                 uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order,
                                 uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, void* stream);

/* fs_connect_flows_batch with every pointer in HOST memory, as fs_close_flows_batch_host: openers_out comes
 * back whole; the replies, reply_out and reply_status spans go to the device first and come back whole, as
 * fs_accept_flows_batch_host does with synacks. */
fs_status fs_connect_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
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
                                      fs_digest* reply_out, uint8_t* reply_status, uint8_t* payload, uint64_t payload_cap,
                                      fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order, uint32_t* run_of,
                                      fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status);

#ifdef __cplusplus
}
#endif
#endif /* FRAMESUM_CONNECT_H */
