/*
 * framesum -- the ring send from device-resident sockets (C ABI, tenth header beside framesum.h,
 * framesum_deliver.h, framesum_send.h, framesum_recv.h, framesum_accept.h, framesum_close.h,
 * framesum_connect.h, framesum_udp.h and framesum_arp.h).
 *
 * fs_send_rings_resident is fs_send_rings_batch (framesum_send.h) with the socket table in DEVICE
 * memory. fs_send_rings_batch evaluates the per-socket rule on the host and stages one record per
 * sending socket, so the ACK that answers a delivery waits for a host round trip although every number
 * it carries is already on the device. Here kernels evaluate the rule, find the layout by a scan and
 * take an RX call's device outputs (socks_out, snd_out) directly as the receive-side state: an RX call
 * and the TX call that answers it are enqueued back to back on one stream, and the host reads both
 * calls' results with one synchronisation afterwards.
 *
 * Everything that depends on a socket's contents is decided on the device and reported per socket,
 * never as a call failure. Sockets are processed in index order, in four steps.
 *
 * 1. Hand-off (rx_socks_out given): exactly tx_sock_from of the Python binding. With
 *    r = rx_index ? rx_index[i] : i, rcv_nxt = rx_socks_out[r].rcv_nxt and rcv_wnd =
 *    rx_socks_out[r].ring_free; with rx_snd_out as well, snd_una and snd_wnd come from it and FS_TX_ACK
 *    is or-ed into the socket's flags where FS_RECV_ACK_OWED is set. rx_index[i] == FS_TX_NO_RX: the
 *    socket keeps its own fields. n_rx is the number of entries of the RX arrays; an index >= n_rx
 *    makes the socket invalid (FS_TX_BAD_RX_INDEX).
 * 2. Checks: those of fs_send_rings_batch for one socket, with rings_bytes. A socket that fails is
 *    INVALID: it makes no frame, nothing of its ring is read, its state is unchanged, and
 *    socks_out[i].sent = FS_TX_INVALID | (reason << 16) with reason one of FS_TX_BAD_*.
 * 3. The rule of framesum_send.h, unchanged: data, fin, S and the last frame's flags. A socket with
 *    S == 0 is IDLE; it is never deferred.
 * 4. Capacity. The host cannot know the layout, so the caller gives room and the call fills it in socket
 *    order. F_i and B_i are the inclusive sums, over the valid sockets 0..i, of their planned frames and
 *    of the bytes of `frames` their slots own, summed as if nothing were deferred, in 64 bits. A socket
 *    with S > 0 is BUILT iff F_i <= frames_cap and B_i <= frames_bytes; otherwise it is DEFERRED: no
 *    frame, state unchanged, sent = FS_TX_DEFERRED. The deferred sockets are therefore those with S > 0
 *    behind the first one that does not fit; a caller sends them by calling again.
 *
 * Built sockets get exactly the frames, offsets, lengths, digests, verdicts and socks_out records that
 * fs_send_rings_batch gives for the list of built sockets: frames in socket order, then segment order;
 * first_frame counts built frames only; `align`, FS_FCS_APPEND, the `mtu` and zero-port verdicts, the
 * ID chain and the window clamp apply as there, and nothing outside the sent ring bytes is read.
 * Entries of the four arrays from totals.n_frames on are not written; bytes of `frames` behind
 * totals.frames_bytes, and between frames, are not written either.
 * A socket that is not built reports its own snd_nxt, ring_rpos and ring_buffered, bytes 0, n_frames 0,
 * first_frame FS_SEND_NONE and its template's ID.
 *
 * FS_TX_WRITEBACK (a call flag, beside FS_FCS_APPEND). Every built socket's snd_nxt, ring_rpos,
 * ring_buffered and template ID (hdr[18:20]) are updated in `socks`; FS_TX_ACK is cleared from its
 * flags (every frame carries the acknowledgement), and FS_TX_FIN where `sent` reports it, so that
 * neither goes out twice. With a hand-off, rcv_nxt, rcv_wnd, snd_una and snd_wnd are written for every
 * valid socket. Idle sockets get the hand-off only; deferred sockets get the hand-off and keep
 * FS_TX_ACK (the one the hand-off set too); invalid sockets get nothing. The table then persists across
 * turns: between them the application only raises ring_buffered and sets flags. Without the flag
 * `socks` is only read.
 *
 * FS_E_INVALID, checked on the host before any device work: a null ctx; flags other than FS_FCS_APPEND
 * and FS_TX_WRITEBACK, or align out of range; a null socks, socks_out or totals with n_socks > 0; a null
 * rings or frames with a non-zero size; rx_snd_out without rx_socks_out; rx_index without
 * rx_socks_out; n_rx != n_socks without rx_index; n_socks above FS_SEND_MAX_SOCKS; frames_cap above
 * 2^31. n_socks == 0 writes zero totals (when totals is given) and nothing else.
 *
 * Every pointer but ctx is a DEVICE pointer. Asynchronous on `stream`. The scratch follows the RX
 * calls' rule: it is owned by the context and sized from n_socks and frames_cap, so use one stream per
 * context, or order the calls. fs_ctx_set_workgroups caps these grids too. There is no _host form:
 * fs_send_rings_batch_host is that.
 */
#ifndef FRAMESUM_SEND_RESIDENT_H
#define FRAMESUM_SEND_RESIDENT_H

#include "framesum_send.h"
#include "framesum_recv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_TX_WRITEBACK 0x100u /* call flag: write the state after the call back into `socks` */
#define FS_TX_DEFERRED 0x100u  /* fs_tx_sock_out.sent: frames planned, no room: call again */
#define FS_TX_INVALID 0x200u   /* fs_tx_sock_out.sent: a check failed, the reason in bits 16.. */
#define FS_TX_NO_RX 0xFFFFFFFFu /* rx_index entry of a socket without an RX record */
/* the reasons, in the order of fs_send_rings_batch's checks */
#define FS_TX_BAD_ETHERTYPE 1u
#define FS_TX_BAD_IHL 2u
#define FS_TX_BAD_PROTO 3u
#define FS_TX_BAD_DATA_OFFSET 4u
#define FS_TX_BAD_MSS 5u
#define FS_TX_BAD_SOCK_FLAGS 6u
#define FS_TX_BAD_MAX_FRAMES 7u
#define FS_TX_BAD_RING_SIZE 8u
#define FS_TX_BAD_RING_POS 9u
#define FS_TX_BAD_BUFFERED 10u
#define FS_TX_BAD_RING_RANGE 11u
#define FS_TX_BAD_RX_INDEX 12u

typedef struct fs_tx_totals {    /* 40 bytes, no padding. DEVICE memory, one record */
    uint64_t n_frames;           /* frames built: the entries written of the four arrays */
    uint64_t frames_bytes;       /* the built sockets' slots: the bytes of `frames` in use */
    uint64_t data_bytes;         /* ring bytes the built frames carry */
    uint32_t n_built, n_idle, n_deferred, n_invalid;   /* sockets; their sum is n_socks */
} fs_tx_totals;

fs_status fs_send_rings_resident(fs_ctx* ctx, fs_tx_sock* socks, uint32_t n_socks,
                                 const fs_rx_sock_out* rx_socks_out, const fs_rx_snd_out* rx_snd_out,
                                 const uint32_t* rx_index, uint32_t n_rx, const uint8_t* rings, uint64_t rings_bytes,
                                 uint32_t mtu, uint32_t flags, uint32_t align, uint8_t* frames, uint64_t frames_bytes,
                                 uint32_t frames_cap, uint64_t* offsets, uint32_t* lengths, fs_digest* out,
                                 uint8_t* status, fs_tx_sock_out* socks_out, fs_tx_totals* totals, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRAMESUM_SEND_RESIDENT_H */
