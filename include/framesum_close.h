/*
 * framesum -- the end of a TCP connection in one call (C ABI, sixth header beside framesum.h,
 * framesum_deliver.h, framesum_send.h, framesum_recv.h and framesum_accept.h).
 *
 * fs_close_flows_batch is fs_accept_flows_batch plus the receive side of the closing states and of an
 * RST: for every listed CLOSER (a socket whose ControlBlock is in FinWait1, FinWait2, Closing, TimeWait,
 * CloseWait or LastAck) it walks the frames of the closer's flow and returns the state the ControlBlock
 * is in behind them; for every Established socket of `socks` it goes on where the receive call's walk
 * ended at an admitted FIN or at an RST. With it one RX call per batch serves a connection from its SYN
 * to its last ACK; what stays on the host is per-socket arithmetic (Close(), Send's state changes,
 * control_user.go:118-137, and the timers).
 *
 * The reference code this restates: validateIncomingSegment (control.go:281-351), handleRST
 * (control.go:407-425) and close (control.go:389-395), Recv (control_user.go:164-224: the state switch
 * at :174-199, the update at :211-217), rcvFinWait1 / rcvFinWait2 (control.go:234-261),
 * IncomingIsKeepalive (control_user.go:260-264), the two gates of TCPConn.recv in front of Recv
 * (stacks/tcpconn.go:337 with IsClosed, seqs.go:224; stacks/tcpconn.go:349) and the state numbers of
 * seqs.go:175-208: Closed 0, Established 4, FinWait1 5, FinWait2 6, Closing 7, TimeWait 8, CloseWait 9,
 * LastAck 10.
 *
 * 1. Relation to fs_accept_flows_batch. Everything that call writes (rings, socks_out, delivered,
 *    snd_out, code, conns, listeners_out, accept_of, synacks, synack_out, synack_status, payload, runs,
 *    flows, order, run_of, totals, out, status) is byte for byte what it writes for the same arguments:
 *    this call runs that enqueue unchanged and adds launches behind it. The accept stage does not know
 *    the list of closers: a closer's flow whose first frame is a lone SYN to a listener is a candidate
 *    there exactly as it is without this call (and this call's walk of that closer ends at slot 0, rule
 *    2 below, unless the closer is in TimeWait, rule 1). `code` stays the accept call's; the codes
 *    below go to `ctl_code` only.
 *
 * 2. The control walk of a closer c whose flow is in the batch. It walks the flow's frames in delivery
 *    order, the slots k of [first_frame, first_frame + n_frames) (frame order[k]), starting with S =
 *    closers[c].state, nxt = rcv_nxt, una = snd_una, wnd = snd_wnd; snd_nxt and rcv_wnd are the
 *    record's throughout. Per frame it reads at L4 = 14 + 4 IHL: Seq, Ack, Window (the raw field at L4 +
 *    14), the nine flag bits (bit 0 of byte L4 + 12, and byte L4 + 13) and len, the payload length.
 *    Each frame gets the FIRST rule that applies; ctl_code[frame] is the rule's code:
 *
 *      rule 1  S is TimeWait or Closed: code 8. The frame is ignored (tcpconn.go:337: IsClosed,
 *              seqs.go:224); nothing changes.
 *      rule 2  SYN set: the walk ENDS; `stop` is this slot, and this frame and the frames behind it keep
 *              ctl_code 0: left to the host, as the delivery leaves the frames from its `stop` on.
 *      rule 3  keepalive (control_user.go:260-264 with rcv.NXT = nxt; tcpconn.go:349): Seq == nxt - 1,
 *              the nine flag bits are ACK alone, Ack == snd_nxt, len == 0: code 5. Nothing changes.
 *      rule 4  len > 0: code 7. Nothing changes. (Difference (a) below.)
 *      rule 5  the Seq checks of control.go:299-311 with DATALEN 0, so LEN() = the FIN bit, fail: code
 *              4. Nothing changes. The four cases, with Last = Seq when LEN() is 0 and Seq + LEN() - 1 =
 *              Seq when it is 1 (seqs.go:26-32), and zeroWindowOK = rcv_wnd == 0 && Seq == nxt
 *              (control.go:291):
 *                :299 needs DATALEN > 0: never.
 *                :302 fails iff Seq - nxt >= rcv_wnd (InWindow, valuesize.go:37-45) and not zeroWindowOK.
 *                :305 is :302 again, because Last == Seq.
 *                :308 fails iff Seq != nxt.
 *              With Seq == nxt, :302 passes (0 < rcv_wnd, or zeroWindowOK at rcv_wnd 0); with Seq != nxt,
 *              :308 fails if :302 has not. So a frame without data passes iff Seq == nxt, at every
 *              rcv_wnd, the bare FIN at rcv_wnd 0 included. (The kernels and the host-only header run the
 *              four literal cases; tests check them against this one-line form.)
 *      rule 6  RST set: code 9, S = Closed, FS_CL_RESET (handleRST, control.go:407-425, then close,
 *              :389-395). The frame has passed rule 5, so Seq == nxt. A consequence, not a rule: without
 *              SYN the reference never reaches handleRST's challenge-ACK branch (:409-413), because
 *              errRequireSequential (:308-311) comes first; an RST with another Seq is code 4 and owes
 *              nothing.
 *      rule 7  by state (control_user.go:174-199):
 *                FinWait1 (rcvFinWait1, control.go:234-253): FIN and ACK and Ack == snd_nxt: S =
 *                  TimeWait; else FIN: S = Closing; else ACK: S = FinWait2; each with FS_CL_ACK_OWED;
 *                  else code 10 (errFinwaitExpectedACK), nothing changes.
 *                FinWait2 (rcvFinWait2, control.go:255-261): FIN and ACK both set: S = TimeWait,
 *                  FS_CL_ACK_OWED; else code 10 (errFinwaitExpectedFinack), nothing changes.
 *                Closing: ACK set: S = TimeWait (control_user.go:192-196).
 *                CloseWait: nothing (control_user.go:187).
 *                LastAck: ACK set: S = Closed (control_user.go:188-191).
 *              A frame that was not refused has code 1 and is ACCEPTED (control_user.go:211-217): wnd =
 *              Window; if ACK is set, una = Ack (there is no duplicate test and no unsent-data test:
 *              control.go:325 and :333 are `established` only); nxt += the FIN bit, and FS_CL_FIN with
 *              it.
 *
 *    The out record: state = S, rcv_nxt = nxt, snd_una = una, snd_wnd = wnd behind the last frame the
 *    walk handled; n_taken counts code 1, n_rejected counts codes 4, 7 and 10; `stop` is the slot after
 *    the last frame the walk handled (first_frame + n_frames when it reached the flow's end); flags as
 *    above. A record whose state is Closed carries 0 in rcv_nxt, snd_una and snd_wnd (difference (b)).
 *    A closer without a flow in the batch, and every closer when n is 0, gets the input state and
 *    numbers, zero counts, zero flags and stop = FS_DELIVER_NONE.
 *
 * 3. The continuation of an Established socket s of `socks`, written to socks_close[s]. It starts at
 *    slot socks_out[s].stop with nxt = socks_out[s].rcv_nxt, una = snd_out[s].snd_una, wnd =
 *    snd_out[s].snd_wnd; snd_nxt and rcv_wnd are socks[s]'s.
 *      FS_RECV_FIN is set in snd_out[s].flags (the admitted FIN is slot stop - 1): S = CloseWait
 *        (rcvEstablished, control.go:224-228), and the walk of rule 2 runs over the slots [stop,
 *        first_frame + n_frames).
 *      Else the slot at `stop` lies in the flow and carries RST and no SYN: rules 3 to 6 apply to it
 *        under S = Established. Code 9: state Closed, FS_CL_RESET, and the walk goes on, so every later
 *        frame of the flow has code 8. Any other code (4, or 7 for an RST that carries data): the state
 *        stays 4, n_rejected is 1, and the walk ends behind that frame: the frames after it could carry
 *        data, which only the delivery may admit.
 *      Otherwise (a SYN at `stop`, the flow's end reached, or no flow in the batch): state 4, the numbers
 *        as the receive call left them, zero counts and flags, stop = socks_out[s].stop, no frame
 *        touched.
 *    Every other frame of an Established socket is the receive call's (framesum_recv.h), not this
 *    call's.
 *
 * 4. Consequences. This call's own stage never writes a ring byte. ctl_code[i] is 0 for every frame no
 *    control walk handled.
 *
 * 5. Differences from the reference.
 *      (a) data in a closing state. The reference would advance rcv.NXT over a data segment that passes
 *          its checks in FinWait1 (and write the bytes to the socket's ring). A closer has no ring, so
 *          every frame with len > 0 is code 7 and changes nothing. The reference itself takes at most
 *          such segments in FinWait1, Closing, CloseWait and LastAck: rcvFinWait2 rejects everything but
 *          FIN | ACK.
 *      (b) the numbers of a Closed record. close() zeroes both sequence spaces, and Recv then goes on to
 *          control_user.go:212-217 for the LastAck case (snd.WND = Window, snd.UNA = Ack, rcv.NXT += LEN)
 *          on the zeroed block. Here a record whose state comes back Closed carries 0 in all three, after
 *          an RST and after LastAck's ACK alike.
 *      (c) a frame with SYN ends the walk and is left to the host (rule 2), whatever the reference
 *          would make of it.
 *      (d) the failed RST of an Established socket ends that socket's walk (section 3).
 *
 * 6. Degenerate sizes. n_closers == 0 and n_socks == 0: the accept call plus a zeroed ctl_code; no other
 *    launch is added. n == 0: the out records as section 2 and 3 give them without a flow.
 *
 * 7. FS_E_INVALID, checked on the host before any device work: everything fs_accept_flows_batch rejects;
 *    null closers or closers_out with n_closers > 0; null socks_close with n_socks > 0; n_closers above
 *    FS_CLOSE_MAX_CLOSERS; a state outside 5..10; key[0] not 6; reserved bytes or reserved2 not 0; two
 *    closers with equal keys; a closer's key equal to a listed socket's; snd_wnd above 65,535.
 *
 * `closers`, like `socks`, is HOST memory, consumed before the call returns (staged per call in a block
 * of its own); closers_out, socks_close and ctl_code (n bytes, nullable) are DEVICE pointers.
 * Asynchronous on `stream`; scratch rules are fs_accept_flows_batch's, and this call adds 20 bytes per
 * frame and 4 per closer. fs_ctx_set_workgroups caps the grids of this call's kernels too.
 */
#ifndef FRAMESUM_CLOSE_H
#define FRAMESUM_CLOSE_H

#include "framesum_accept.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the reference's state numbers (seqs.go:175-208) */
#define FS_ST_CLOSED 0u
#define FS_ST_ESTABLISHED 4u
#define FS_ST_FIN_WAIT_1 5u
#define FS_ST_FIN_WAIT_2 6u
#define FS_ST_CLOSING 7u
#define FS_ST_TIME_WAIT 8u
#define FS_ST_CLOSE_WAIT 9u
#define FS_ST_LAST_ACK 10u

/* ctl_code: 0 no control walk handled the frame; 1, 4 and 5 as the receive call's codes */
#define FS_CL_TAKEN 1u
#define FS_CL_REJECTED 4u
#define FS_CL_KEEPALIVE 5u
#define FS_CL_DATA 7u      /* a frame with payload in a closing state */
#define FS_CL_IGNORED 8u   /* TimeWait or Closed */
#define FS_CL_RST 9u       /* the RST that closed the connection */
#define FS_CL_EXPECTED 10u /* FinWait1 / FinWait2 expected other flags */

/* fs_cl_out.flags */
#define FS_CL_ACK_OWED 1u
#define FS_CL_FIN 2u   /* this walk took a FIN from the peer */
#define FS_CL_RESET 4u

#define FS_CLOSE_MAX_CLOSERS 65536u

typedef struct fs_cl_sock {      /* 40 bytes, no padding. HOST memory. A closer has no ring */
    uint8_t key[13];             /* as fs_rx_sock.key */
    uint8_t state;               /* FS_ST_FIN_WAIT_1 .. FS_ST_LAST_ACK */
    uint8_t reserved[2];         /* must be 0 */
    uint32_t rcv_nxt, rcv_wnd;
    uint32_t snd_una, snd_nxt;
    uint32_t snd_wnd;            /* at most 65,535 */
    uint32_t reserved2;          /* must be 0 */
} fs_cl_sock;

typedef struct fs_cl_out {       /* 32 bytes, no padding. DEVICE memory, all entries written */
    uint32_t state;
    uint32_t rcv_nxt, snd_una, snd_wnd;
    uint32_t n_taken;            /* frames with code 1 */
    uint32_t n_rejected;         /* codes 4, 7 and 10 */
    uint32_t stop;               /* the slot after the last frame the walk handled, or FS_DELIVER_NONE */
    uint32_t flags;              /* FS_CL_ACK_OWED, FS_CL_FIN, FS_CL_RESET */
} fs_cl_out;

fs_status fs_close_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                               uint32_t n, uint32_t mtu, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks,
                               uint8_t* rings, uint64_t rings_bytes, fs_rx_sock_out* socks_out, uint8_t* delivered,
                               const fs_rx_snd* snd, fs_rx_snd_out* snd_out, uint8_t* code, const fs_listener* listeners,
                               uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots, uint32_t synack_flags,
                               fs_accept_conn* conns, fs_listener_out* listeners_out, uint32_t* accept_of,
                               uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status, const fs_cl_sock* closers,
                               uint32_t n_closers, fs_cl_out* closers_out, fs_cl_out* socks_close, uint8_t* ctl_code,
                               uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order,
                               uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, void* stream);

/* fs_close_flows_batch with every pointer in HOST memory, as fs_accept_flows_batch_host: closers_out,
 * socks_close and ctl_code come back whole. */
fs_status fs_close_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                                    const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags,
                                    const fs_rx_sock* socks, uint32_t n_socks, uint8_t* rings, uint64_t rings_bytes,
                                    fs_rx_sock_out* socks_out, uint8_t* delivered, const fs_rx_snd* snd,
                                    fs_rx_snd_out* snd_out, uint8_t* code, const fs_listener* listeners,
                                    uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots,
                                    uint32_t synack_flags, fs_accept_conn* conns, fs_listener_out* listeners_out,
                                    uint32_t* accept_of, uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status,
                                    const fs_cl_sock* closers, uint32_t n_closers, fs_cl_out* closers_out,
                                    fs_cl_out* socks_close, uint8_t* ctl_code, uint8_t* payload, uint64_t payload_cap,
                                    fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order, uint32_t* run_of,
                                    fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status);

#ifdef __cplusplus
}
#endif
#endif /* FRAMESUM_CLOSE_H */
