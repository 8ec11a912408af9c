/*
 * framesum -- the receive side of an established TCP connection in one call (C ABI, fourth header
 * beside framesum.h, framesum_deliver.h and framesum_send.h).
 *
 * fs_recv_flows_batch is fs_deliver_flows_batch plus the per-frame job that call leaves to the host:
 * for every listed socket it applies what ControlBlock.Recv does to the SEND side of an Established
 * connection (snd.UNA, snd.WND, the pending ACK) for each frame of the socket's flow, and returns the
 * per-socket result and a per-frame code. With it the host loop is one RX call, per-socket arithmetic
 * (tx_sock_from in the Python binding), one TX call (fs_send_rings_batch, framesum_send.h).
 *
 * The reference code this restates: validateIncomingSegment (control.go:281-351), Recv
 * (control_user.go:164-224, in particular :212-215), IncomingIsKeepalive (control_user.go:260-264,
 * called at stacks/tcpconn.go:349 before Recv), LessThan / LessThanEq (valuesize.go:27-34) and the
 * nine flag bits (eth/headers.go:174, :487).
 *
 * Relation to fs_deliver_flows_batch. rings, socks_out, delivered, payload, runs, flows, order, run_of,
 * totals, out and status are byte for byte what fs_deliver_flows_batch writes for the same arguments:
 * the call runs that enqueue unchanged and adds launches behind it.
 *
 * The walk. For a socket s whose flow is in the batch, take from the delivery: first =
 * flows[flow].first_frame; stop = socks_out[s].stop; nxt_k = rcv.NXT as the delivery's walk has it
 * before slot k, i.e. socks[s].rcv_nxt plus len + fin of every admitted slot in [first, k). The slots k
 * in [first, stop) are walked in delivery order, starting with una = snd[s].snd_una and wnd =
 * snd[s].snd_wnd. Per frame, read at L4 = 14 + 4 IHL: Seq, Ack, Window (the raw 16-bit field at L4 +
 * 14), the nine flag bits (bit 0 of byte L4 + 12, and byte L4 + 13), and len, its payload length.
 * snd_nxt and rcv_wnd are socks[s]'s. All comparisons are the reference's modular ones: LessThan(v, w)
 * is (int32)(v - w) < 0, LessThanEq(v, w) is v == w or LessThan(v, w).
 *
 *   A PURE frame has len 0 and FIN clear (SYN and RST cannot occur before `stop`). Its code is the
 *   first of these that applies:
 *     5  keepalive: Seq == nxt_k - 1, the nine flag bits are ACK alone, and Ack == snd_nxt. Nothing
 *        changes.
 *     4  Seq != nxt_k (errSeqNotInWindow or errRequireSequential; a zero rcv_wnd with Seq == nxt_k
 *        passes, zeroWindowOK).
 *     2  duplicate: ACK set and !LessThan(una, Ack). Dropped, so its window is not taken either.
 *     3  ACK set and !LessThanEq(Ack, snd_nxt): it acknowledges unsent data. Dropped; an ACK is owed.
 *     1  taken: wnd = Window; if ACK is set, una = Ack.
 *   A CONSIDERED frame has data or FIN. Its code is
 *     1  iff the delivery admitted it (delivered == 1): wnd = Window, and if ACK is set una = Ack,
 *        even when that moves una backwards (control_user.go:213-215). The duplicate test does not
 *        apply to it (ctlOrDataSegment).
 *     4  if it is not admitted and rule (a) or (b) of the delivery fails;
 *     3  if it is not admitted, (a) and (b) hold and (c) fails;
 *     6  otherwise: the ring is full, the delivery's stated difference from the reference.
 *
 * code[i] is 1..6 for every frame of a listed socket's flow before `stop` and 0 for every other frame
 * of the batch. `code` (n bytes) may be NULL.
 * FS_RECV_ACK_OWED is set iff some considered frame has code 1 (rcvEstablished, control.go:217-232) or
 * some frame has code 3 (control.go:335). FS_RECV_FIN is set iff a FIN was admitted.
 *
 * Two differences from the reference. The ring-full case (code 6) is the delivery's, see
 * framesum_deliver.h. And the reference's duplicate ACK clears a pending ACK (control.go:327); inside
 * one batch that would lose the ACK for data admitted earlier in the same batch, so a duplicate here
 * never clears FS_RECV_ACK_OWED.
 * (A consequence of the delivery's rule (b), not a third rule: at rcv_wnd 0 a FIN without data at Seq ==
 * nxt_k is not admitted and gets code 4, where the reference's zeroWindowOK lets it pass the window
 * checks, control.go:291.)
 *
 * Sockets without a flow in the batch, and n == 0: snd_out = the input state, zero counts, zero flags.
 * With n_socks == 0 the call is fs_deliver_flows_batch with n_socks 0, plus a zeroed `code`.
 *
 * FS_E_INVALID, checked on the host before any device work: everything fs_deliver_flows_batch rejects;
 * null snd or snd_out with n_socks > 0; snd_wnd above 65,535; (int32)(snd_una - snd_nxt) > 0. With this
 * last check every value una can take lies at most 2^31 behind snd_nxt.
 *
 * `snd`, like `socks`, is HOST memory, consumed before the call returns (staged per call in a block of
 * its own); `snd_out` and `code` are DEVICE pointers. Asynchronous on `stream`; scratch rules are
 * fs_deliver_flows_batch's, and this call adds 8 bytes per frame. fs_ctx_set_workgroups caps the grids
 * of this call's kernels too.
 */
#ifndef FRAMESUM_RECV_H
#define FRAMESUM_RECV_H

#include "framesum_deliver.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_RECV_ACK_OWED 1u /* fs_rx_snd_out.flags: an ACK is to be sent */
#define FS_RECV_FIN 2u      /* fs_rx_snd_out.flags: the peer's FIN was admitted */

typedef struct fs_rx_snd {       /* 8 bytes. HOST memory, one per socket, parallel to socks */
    uint32_t snd_una, snd_wnd;   /* tcb.snd.UNA, tcb.snd.WND (at most 65,535) */
} fs_rx_snd;

typedef struct fs_rx_snd_out {   /* 32 bytes, no padding. DEVICE memory, n_socks entries, all written */
    uint32_t snd_una, snd_wnd;   /* after the call */
    uint32_t n_taken;            /* frames with code 1 */
    uint32_t n_dup, n_unsent, n_rejected, n_keepalive; /* codes 2, 3, 4 + 6, 5 */
    uint32_t flags;              /* FS_RECV_ACK_OWED, FS_RECV_FIN */
} fs_rx_snd_out;

fs_status fs_recv_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                              uint32_t n, uint32_t mtu, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks,
                              uint8_t* rings, uint64_t rings_bytes, fs_rx_sock_out* socks_out, uint8_t* delivered,
                              const fs_rx_snd* snd, fs_rx_snd_out* snd_out, uint8_t* code, uint8_t* payload,
                              uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order,
                              uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, void* stream);

/* fs_recv_flows_batch with every pointer in HOST memory, as fs_deliver_flows_batch_host: snd_out and
 * code come back with the rest. */
fs_status fs_recv_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                                   const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags,
                                   const fs_rx_sock* socks, uint32_t n_socks, uint8_t* rings, uint64_t rings_bytes,
                                   fs_rx_sock_out* socks_out, uint8_t* delivered, const fs_rx_snd* snd,
                                   fs_rx_snd_out* snd_out, uint8_t* code, uint8_t* payload, uint64_t payload_cap,
                                   fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order, uint32_t* run_of,
                                   fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status);

#ifdef __cplusplus
}
#endif
#endif /* FRAMESUM_RECV_H */
