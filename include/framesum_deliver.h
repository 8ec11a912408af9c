/*
 * framesum -- in-order TCP delivery into socket rings (C ABI, second header beside framesum.h).
 *
 * fs_deliver_flows_batch is fs_coalesce_flows_batch plus the step that call stops before. The
 * reference delivers one frame at a time: TCPConn.recv (stacks/tcpconn.go:347-371) checks the remote
 * address, hands the segment to the ControlBlock (scb.Recv, control.go:281-312: the in-order rule
 * errRequireSequential at :308, the window checks at :299-305, the ACK check at :289 / :333) and
 * then appends the payload to the socket's ring (`sock.rx.Write(payload)`, tcpconn.go:369; the
 * ring's placement and its wrap are stacks/ring.go:17-40). A stack that uses the flow-aware
 * coalesce does that on the host once per flow, and copies the admitted bytes a second time out of
 * the packed payload buffer. This call does it on the GPU for every flow that belongs to a socket
 * the caller lists: the flow's data segments are admitted in order and their bytes go straight
 * from the frames into that socket's ring in device memory, wrapping at the ring's end; the
 * socket's advanced receive state comes back. The host keeps the control plane: ACK processing,
 * SYN / RST handling and state changes. The packed payload becomes optional.
 *
 * Relation to fs_coalesce_flows_batch. payload, runs, flows, order, run_of, totals, out and status
 * are byte for byte what fs_coalesce_flows_batch writes for the same arguments: the call runs that
 * enqueue unchanged. With payload NULL and payload_cap 0 no packed copy is made. Delivery reads
 * the frames, not the packed buffer, and does not depend on payload_cap.
 *
 * Which flows are delivered. A flow belongs to socket s iff its 13 key bytes (framesum.h) equal
 * socks[s].key. Keys in `socks` are distinct, so a socket has at most one flow. Flows without a
 * socket, and UDP flows, get nothing beyond what fs_coalesce_flows_batch gives them.
 *
 * The walk over a socket's flow. The flow's frames are walked in delivery order (order[first_frame
 * .. first_frame + n_frames) of its fs_rx_flow) with the state (nxt, wpos, free) taken from the
 * socket record.
 *   A frame with SYN or RST set ends the walk: `stop` is that frame's index into `order`; that
 *   frame and every later frame of the flow are left to the host untouched.
 *   Otherwise a frame is CONSIDERED iff its payload is non-empty or FIN is set. Pure ACKs are
 *   passed over: they change nothing here, and the host reads their ACK and window fields itself.
 *   With len the payload length and fin the FIN bit, a considered frame is ADMITTED iff
 *     (a) Seq == nxt (control.go:308);
 *     (b) len + fin <= rcv_wnd (InWindow of SEQ and of Last() at control.go:302-305 when SEQ ==
 *         nxt; a zero window admits nothing, :299);
 *     (c) ACK clear, or (int32)(Ack - snd_nxt) <= 0 (:289, :333: an established connection drops a
 *         segment that acknowledges unsent data);
 *     (d) len <= free (ring.go:18-21).
 *   An admitted frame: its payload byte j goes to rings[ring_off + (wpos + j) mod ring_size]; wpos =
 *   (wpos + len) mod ring_size; free -= len; nxt += len + fin (mod 2^32); delivered[i] = 1.
 *   A considered frame that is not admitted changes nothing and gets delivered[i] = 2. Every other
 *   frame of the batch gets delivered[i] = 0.
 *   After an admitted FIN the walk ends: `stop` is the index after it. If the walk reaches the
 *   flow's end, stop = first_frame + n_frames.
 * Seq, Ack and the flags are read at L4 = 14 + 4 IHL, as the key's ports are: IP options and TCP
 * options do not exclude a frame.
 *
 * One difference from the reference. When (a)-(c) hold and the ring is full, the reference has
 * already advanced rcv.NXT in scb.Recv before rx.Write fails (tcpconn.go:353-371), and the bytes
 * are lost to the connection. Here the frame is not admitted and rcv_nxt stays, so the peer's
 * retransmission is admitted later.
 *
 * The caller lists only sockets whose ControlBlock is in StateEstablished; the rules above are that
 * state's.
 *
 * Ring bytes that no admitted frame covers are not written (not even read and written back), and
 * nothing is written to `rings` outside the listed rings.
 *
 * FS_E_INVALID, checked on the host before any device work: everything fs_coalesce_flows_batch
 * rejects; null socks, rings or socks_out with n_socks > 0; n_socks above FS_DELIVER_MAX_SOCKS
 * (which bounds the staged block); key[0] != 6 or reserved != 0; two equal keys; ring_size 0 or above
 * 2^31; ring_wpos >= ring_size or ring_free > ring_size; a ring outside rings_bytes; two rings that
 * overlap.
 *
 * Degenerate sizes. n_socks of 0 is fs_coalesce_flows_batch plus a zeroed `delivered`. n of 0 writes
 * zero totals and every socks_out[s] with the input state, flow = stop = 0xFFFFFFFF and zero counts.
 *
 * `socks` is HOST memory, consumed before the call returns (staged per call in a block of its own,
 * like the sends of fs_segment_batch, together with a hash table over the keys built on the host);
 * every other pointer is a DEVICE pointer. `delivered` (n bytes) may be NULL. Asynchronous on
 * `stream`. Scratch rules are fs_coalesce_flows_batch's (one stream per context, or ordered by the
 * caller); this call adds 16 bytes per frame and 4 per socket. Two calls that name the same socket
 * are ordered by the caller: the second takes its state from the first's socks_out.
 * fs_ctx_set_workgroups caps the grids of this call's kernels too.
 */
#ifndef FRAMESUM_DELIVER_H
#define FRAMESUM_DELIVER_H

#include "framesum.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_DELIVER_MAX_SOCKS 65536u
#define FS_DELIVER_NONE 0xFFFFFFFFu /* fs_rx_sock_out.flow / .stop of a socket without a flow in the batch */

typedef struct fs_rx_sock {      /* 48 bytes, no padding. HOST memory, consumed before the call returns */
    uint8_t  key[13];            /* the flow key as the socket's received frames carry it (framesum.h):
                                    protocol (must be 6), source = remote address, destination = local
                                    address, source = remote port, destination = local port */
    uint8_t  reserved[3];        /* must be 0 */
    uint32_t rcv_nxt;            /* tcb.rcv.NXT */
    uint32_t rcv_wnd;            /* tcb.rcv.WND */
    uint32_t snd_nxt;            /* tcb.snd.NXT */
    uint32_t ring_size;          /* 1 .. 2^31 */
    uint64_t ring_off;           /* the ring is rings[ring_off : ring_off + ring_size) */
    uint32_t ring_wpos;          /* next byte to write, < ring_size */
    uint32_t ring_free;          /* bytes that may be written, <= ring_size */
} fs_rx_sock;

typedef struct fs_rx_sock_out {  /* 32 bytes, no padding. DEVICE memory, n_socks entries, all written */
    uint32_t rcv_nxt, ring_wpos, ring_free;  /* the socket's state after the call */
    uint32_t bytes;              /* written into the ring by this call */
    uint32_t n_delivered, n_dropped;         /* considered frames admitted / not admitted */
    uint32_t flow;               /* index into flows of the socket's flow in this batch, 0xFFFFFFFF: none */
    uint32_t stop;               /* above; 0xFFFFFFFF when flow is */
} fs_rx_sock_out;

fs_status fs_deliver_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                                 uint32_t n, uint32_t mtu, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks,
                                 uint8_t* rings, uint64_t rings_bytes, fs_rx_sock_out* socks_out, uint8_t* delivered,
                                 uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows,
                                 uint32_t* order, uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out,
                                 uint8_t* status, void* stream);

/* fs_deliver_flows_batch with every pointer in HOST memory, as fs_coalesce_flows_batch_host
 * (frames_bytes bounds every frame, rings_bytes every ring): in addition it copies the span of
 * `rings` that the listed rings cover to the device and back, so that the bytes between rings keep
 * the caller's values, and copies socks_out and delivered back. */
fs_status fs_deliver_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                                      const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags,
                                      const fs_rx_sock* socks, uint32_t n_socks, uint8_t* rings, uint64_t rings_bytes,
                                      fs_rx_sock_out* socks_out, uint8_t* delivered, uint8_t* payload,
                                      uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order,
                                      uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status);

#ifdef __cplusplus
}
#endif
#endif /* FRAMESUM_DELIVER_H */
