/*
 * framesum -- TCP segments built from socket TX rings (C ABI, third header beside framesum.h and
 * framesum_deliver.h).
 *
 * fs_send_rings_batch is the transmit counterpart of fs_deliver_flows_batch. The reference sends in
 * three steps (TCPConn.send, stacks/tcpconn.go:383-431): it asks the ControlBlock how much may go out
 * (PendingSegment, control.go:100-152, limited by snd.maxSend() = snd.WND - (snd.NXT - snd.UNA),
 * control.go:82-89), reads that many bytes out of the socket's TX ring (sock.tx.Read, which wraps:
 * stacks/ring.go:42-66), and builds the headers from the connection state (CalculateHeaders,
 * port_tcp.go:162-194: Seq = snd.NXT, Ack = rcv.NXT, Window = rcv.WND) before PutHeaders writes them.
 * This call does the three for every listed socket at once: the per-socket rule below is evaluated on
 * the host, and one kernel reads each socket's bytes straight out of its ring in device memory,
 * across the ring's end, into finished frames. No linear copy of the ring is made, and the mss grid
 * does not break at the wrap.
 *
 * The per-socket rule (all arithmetic mod 2^32 where it wraps):
 *   in_flight = snd_nxt - snd_una
 *   room      = snd_wnd > in_flight ? snd_wnd - in_flight : 0
 *   data      = min(ring_buffered, room, max_frames * mss)       (max_frames 0: FS_SEGMENT_MAX_FRAMES)
 *   fin       = (flags & FS_TX_FIN) && data == ring_buffered
 *   S         = ceil(data / mss); when that is 0 and fin or FS_TX_ACK is set, S = 1 with an empty
 *               payload; otherwise the socket makes no frame.
 * The FIN needs no window room (control.go:119). It rides on the last data segment, or on a frame of
 * its own when data is 0, and it waits until every buffered byte has left: the usual rule, an
 * extension in the spirit of fs_segment_batch's FIN / PSH rule.
 * Frame k (0 <= k < S) carries chunk_k = min(mss, data - k*mss) ring bytes: its payload byte j is
 * rings[ring_off + (ring_rpos + k*mss + j) mod ring_size]. Its header is the template with
 *   Seq = snd_nxt + k*mss, Ack = rcv_nxt, Window = min(rcv_wnd, 65535),
 *   flags = ACK, plus PSH on the last data segment with FS_TX_PSH, plus FIN on the last frame when fin,
 *   IPv4 ID = prand16 applied k times to the template's ID,
 * and everything else exactly as fs_segment_batch writes a TCP send's frame k: IPv4 byte 0 written as
 * 0x45, TotalLength, the urgent pointer cleared, both checksums, the FCS with FS_FCS_APPEND, and the
 * `mtu` and zero-port verdicts with zeroed checksum fields.
 * After the call: snd_nxt += data + fin; ring_rpos = (ring_rpos + data) mod ring_size;
 * ring_buffered -= data. socks_out[i] holds these, the frames' place, and the template ID for the
 * next call. It follows from the rule alone: fs_send_rings_layout writes the same records without a
 * device.
 *
 * Differences from the reference.
 *   A window that shrank below what is in flight (in_flight > snd_wnd) makes the reference panic
 *   (control.go:121); here it is a room of 0.
 *   The reference truncates the window with uint16(rcv.WND); here a window above 65,535 is sent as
 *   65,535. No window-scale option is built (data offset 5: no options at all).
 *   The reference resets an emptied ring to position 0 (ring.go:107-109); this call reports the
 *   modular position (ring_rpos + data) mod ring_size, which names the same empty ring.
 *
 * Layout and outputs. Frames lie in socket order, then segment order; `align`, `flags`
 * (FS_FCS_APPEND) and the slots follow fs_segment_batch's rule, and offsets, lengths, out and status
 * (each nullable) have its meaning. Bytes of `frames` that belong to no frame and no FCS are not
 * written. `rings` is only read, and only inside the bytes the frames carry: no byte outside a listed
 * ring's sent range is loaded, not by the 16-byte piece that straddles the ring's end either. Rings
 * may overlap.
 *
 * FS_E_INVALID, checked on the host before any device work: a null ctx; flags or align out of range;
 * what fs_segment_batch rejects for a TCP template (EtherType not 0x0800, IHL not 5, protocol not 6,
 * data offset not 5); mss 0 or above 65,495; unknown bits in a socket's flags; max_frames above
 * FS_SEGMENT_MAX_FRAMES; ring_size 0 or above 2^31; ring_rpos >= ring_size; ring_buffered >
 * ring_size; a ring outside rings_bytes; n_socks above FS_SEND_MAX_SOCKS; a null socks, rings or
 * frames while there is something to build; more than 2^31 frames; frames_bytes below the layout's.
 * fs_send_rings_layout checks the same, less what needs rings_bytes, frames and frames_bytes.
 * n_socks of 0 is success and writes nothing; a batch whose sockets all make no frame is success,
 * launches nothing and still writes socks_out. After FS_E_INVALID the contents of socks_out are
 * unspecified (the records are written while the sockets are checked).
 *
 * `socks` and `socks_out` are HOST memory: socks is consumed, and socks_out written, before the call
 * returns. rings, frames, offsets, lengths, out and status are DEVICE pointers. Asynchronous on
 * `stream`. Calls on one context need no synchronization between them (each stages its records in a
 * block of its own, like fs_segment_batch); a second call for the same socket takes its state from
 * the first call's socks_out. fs_ctx_set_workgroups caps this kernel's grid too.
 */
#ifndef FRAMESUM_SEND_H
#define FRAMESUM_SEND_H

#include "framesum.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_SEND_MAX_SOCKS 65536u
#define FS_SEND_NONE 0xFFFFFFFFu /* fs_tx_sock_out.first_frame of a socket that made no frame */
#define FS_TX_ACK 1u   /* nothing else to send: still emit one bare ACK (the reply to a delivery) */
#define FS_TX_FIN 2u   /* the user closed: FIN goes out once every buffered byte has */
#define FS_TX_PSH 4u   /* PSH on the socket's last data segment of this call */

typedef struct fs_tx_sock {      /* 104 bytes, no padding. HOST memory, consumed before the call returns */
    uint8_t  hdr[54];            /* template as fs_tx_send.hdr, TCP only: MACs, ToS, ID seed, fragment
                                    field, TTL, addresses, ports. Seq, Ack, flags, window, both
                                    checksums, TotalLength and the urgent pointer are overwritten */
    uint16_t mss;                /* 1 .. 65495 */
    uint64_t ring_off;           /* the TX ring is rings[ring_off : ring_off + ring_size) */
    uint32_t ring_size;          /* 1 .. 2^31 */
    uint32_t ring_rpos;          /* next unsent byte, < ring_size (ring.off) */
    uint32_t ring_buffered;      /* unsent bytes, <= ring_size (ring.Buffered()) */
    uint32_t snd_una, snd_nxt, snd_wnd;
    uint32_t rcv_nxt, rcv_wnd;
    uint32_t max_frames;         /* 1 .. FS_SEGMENT_MAX_FRAMES; 0 means FS_SEGMENT_MAX_FRAMES */
    uint32_t flags;              /* FS_TX_* */
} fs_tx_sock;

typedef struct fs_tx_sock_out {  /* 32 bytes. HOST memory, n_socks entries, written before the call returns */
    uint32_t snd_nxt, ring_rpos, ring_buffered;   /* state after the call */
    uint32_t bytes, n_frames, first_frame;        /* first_frame: index into offsets/lengths/out/status, FS_SEND_NONE when n_frames is 0 */
    uint32_t ip_id;              /* the template ID for the next call: prand16 applied n_frames times */
    uint32_t sent;               /* FS_TX_FIN if a FIN went out, FS_TX_ACK if the frame is a bare ACK */
} fs_tx_sock_out;

/* Host-only arithmetic: the frames and bytes of `frames` a batch of sockets needs, and (socks_out not
 * NULL) every socket's record. */
fs_status fs_send_rings_layout(const fs_tx_sock* socks, uint32_t n_socks, uint32_t flags, uint32_t align,
                               uint64_t* n_frames, uint64_t* frames_bytes, fs_tx_sock_out* socks_out);

fs_status fs_send_rings_batch(fs_ctx* ctx, const fs_tx_sock* socks, uint32_t n_socks, const uint8_t* rings,
                              uint64_t rings_bytes, uint32_t mtu, uint32_t flags, uint32_t align, uint8_t* frames,
                              uint64_t frames_bytes, uint64_t* offsets, uint32_t* lengths, fs_digest* out,
                              uint8_t* status, fs_tx_sock_out* socks_out, void* stream);

/* fs_send_rings_batch with every pointer in HOST memory: copies the span of `rings` that the call
 * reads to the device, builds the frames, copies the frame span and the four arrays back (on the
 * context's compute stream), and returns when they are written. The bytes between frames keep the
 * caller's values. */
fs_status fs_send_rings_batch_host(fs_ctx* ctx, const fs_tx_sock* socks, uint32_t n_socks, const uint8_t* rings,
                                   uint64_t rings_bytes, uint32_t mtu, uint32_t flags, uint32_t align,
                                   uint8_t* frames, uint64_t frames_bytes, uint64_t* offsets, uint32_t* lengths,
                                   fs_digest* out, uint8_t* status, fs_tx_sock_out* socks_out);

#ifdef __cplusplus
}
#endif
#endif /* FRAMESUM_SEND_H */
