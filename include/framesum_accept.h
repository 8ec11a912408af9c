/*
 * framesum -- the passive open in one call (C ABI, fifth header beside framesum.h, framesum_deliver.h,
 * framesum_send.h and framesum_recv.h).
 *
 * fs_accept_flows_batch is fs_recv_flows_batch plus the job that call leaves to the host for every flow
 * WITHOUT a listed socket: a first SYN to a listening address and port takes one of the listener's free
 * connections, and its SYN-ACK is built, with both checksums and the FCS, on the device.
 *
 * The reference code this restates: TCPListener.recv (stacks/tcplistener.go:128-164: the flag test at
 * :133, the first free connection at :135-141, the Ack test at :137, ErrDroppedPacket at :153-156),
 * freeConnForReuse (tcplistener.go:178-185), rcvListen (control.go:157-173: resetSnd / resetRcv),
 * rcv.NXT += LEN() (control_user.go:216-217), PendingSegment / Send in StateSynRcvd (control.go:100-152,
 * control_user.go:106-158; zeroWindowOK, control.go:358) and CalculateHeaders / PutHeaders
 * (stacks/port_tcp.go:162-194; the ID is prand16 of the connection's seed, port_tcp.go:173).
 *
 * 1. Relation to fs_recv_flows_batch. Everything that call writes (rings, socks_out, delivered, snd_out,
 *    code, payload, runs, flows, order, run_of, totals, out, status) is byte for byte what it writes for
 *    the same arguments: this call runs that enqueue unchanged and adds launches behind it.
 *
 * 2. Candidates. Flow f of the batch is a CANDIDATE iff
 *      no socket in `socks` has its key;
 *      its protocol (key byte 0) is 6;
 *      its first frame in delivery order, order[flows[f].first_frame], read at L4 = 14 + 4 IHL, has the
 *      nine flag bits (bit 0 of byte L4 + 12, and byte L4 + 13) equal to SYN alone, an Ack field of 0
 *      and an empty payload;
 *      some listener's `local` equals the key's destination address and port (key bytes 5..8, 11..12).
 *    IP options and TCP options do not exclude a frame. Later frames of the flow are left untouched, as
 *    frames behind `stop` are.
 *
 * 3. Slots, per listener. The candidates of one listener take its slots in ascending order of flow
 *    number: the r-th candidate (r from 0) takes slots[slot_first + r], as the reference takes the first
 *    free connection. Candidates with r >= n_slots get FS_ACCEPT_FULL (the reference's
 *    ErrDroppedPacket). accept_of[f], for every flow f < totals->n_flows, is the slot index (an index
 *    into `slots` / `conns`, not relative to the listener), FS_ACCEPT_FULL, or FS_ACCEPT_NONE for a
 *    flow that is no candidate; entries from n_flows on are FS_ACCEPT_NONE. Nothing in the result
 *    depends on a hash function, on the order in which lanes run, or on the grid.
 *
 * 4. A filled slot gets its fs_accept_conn (below) and its SYN-ACK at synacks + slot * FS_ACCEPT_STRIDE.
 *    peer_mss is the value of the first well-formed MSS option (kind 2, length 4) in
 *    frame[L4 + 20 : L4 + 4 dataoff): kind 0 ends the walk, kind 1 advances one byte, any other kind needs
 *    its length byte inside the range, a length of at least 2 and the whole option inside the range,
 *    else the walk ends; at most 40 steps; 0 when there is none. (An extension: the reference reads no
 *    options. The ring send's `mss` needs it.)
 *    The SYN-ACK is 54 bytes, 58 with FS_FCS_APPEND; bytes 54 / 58 .. 63 of its 64 are not written, and
 *    no byte of an unfilled slot is. Ethernet destination = the SYN's source MAC, source = the
 *    listener's `mac`, EtherType 0x0800; IPv4 byte 0 = 0x45, ToS 0, TotalLength 40, ID = prand16(ip_id),
 *    fragment field 0, TTL 64, protocol 6, source = the `local` address, destination = the key's source
 *    address; ports swapped; Seq = iss, Ack = the SYN's Seq + 1, data offset 5, flags SYN | ACK,
 *    Window = min(rcv_wnd, 65535) (the ring send's stated difference from the reference's uint16()
 *    truncation), urgent pointer 0; both checksums, the FCS and the `mtu` verdict exactly as
 *    fs_send_rings_batch writes a frame (the same frame body builds it). The frame goes out at window 0
 *    too. synack_out[slot] / synack_status[slot] are what fs_digest_batch(..., mtu, ...) reports for
 *    that frame; they are written for filled slots only.
 *
 * 5. Differences from the reference.
 *      A SYN that carries data is not a candidate (the reference would advance rcv.NXT over bytes for
 *      which no ring exists yet).
 *      The reference's scan over its connections can hand a SYN from a known remote to an earlier free
 *      connection before it reaches the connection that owns that remote. Here a flow with a listed
 *      socket is never a candidate: a host that lists its half-open connections in `socks` never spends
 *      two slots on a retransmitted SYN.
 *      Listeners match address and port; there is no wildcard address.
 *    A half-open connection is listed for the next call with key = conn.key, rcv_nxt = conn.rcv_nxt,
 *    snd_nxt = conn.snd_nxt (= iss + 1) and snd[s] = {iss, conn.snd_wnd}. The handshake's third ACK is
 *    then code 1 with snd_una == iss + 1; a wrong Ack is code 2 or 3: rcvSynRcvd's test, because only
 *    iss + 1 lies in (snd_una, snd_nxt].
 *
 * 6. Degenerate sizes. n_listeners == 0: the receive call, plus zeroed `conns`, plus accept_of all
 *    FS_ACCEPT_NONE; no other launch is added. n == 0: zeroed `conns` and `listeners_out`. n_slots == 0
 *    with listeners: every candidate is FS_ACCEPT_FULL.
 *
 * 7. FS_E_INVALID, checked on the host before any device work: everything fs_recv_flows_batch rejects;
 *    null listeners, listeners_out, slots, conns or synacks where their count is above 0; counts above
 *    FS_ACCEPT_MAX_LISTENERS / FS_ACCEPT_MAX_SLOTS; a listener's or a slot's `reserved` not 0; two
 *    listeners with equal `local`; a `local` with port 0; a slot range outside n_slots; two listeners
 *    whose slot ranges overlap; synack_flags other than 0 or FS_FCS_APPEND.
 *
 * `listeners` and `slots`, like `socks`, are HOST memory, consumed before the call returns (staged per
 * call in a block of their own); conns, listeners_out, accept_of, synacks, synack_out and synack_status
 * are DEVICE pointers. Asynchronous on `stream`; scratch rules are fs_recv_flows_batch's, and this call
 * adds 20 bytes per frame, the sort's temporary storage and 88 bytes per slot. fs_ctx_set_workgroups
 * caps the grids of this call's kernels too.
 */
#ifndef FRAMESUM_ACCEPT_H
#define FRAMESUM_ACCEPT_H

#include "framesum_recv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_ACCEPT_STRIDE 64u            /* bytes of `synacks` per slot */
#define FS_ACCEPT_NONE 0xFFFFFFFFu      /* accept_of: the flow is no candidate */
#define FS_ACCEPT_FULL 0xFFFFFFFEu      /* accept_of: a candidate whose listener had no slot left */
#define FS_ACCEPT_MAX_LISTENERS 65536u
#define FS_ACCEPT_MAX_SLOTS 65536u

typedef struct fs_listener {     /* 24 bytes, no padding. HOST memory */
    uint8_t local[6];            /* wire order: destination address (key bytes 5..8), destination port (11..12) */
    uint8_t mac[6];              /* Ethernet source of the SYN-ACKs */
    uint32_t slot_first, n_slots; /* its free connections: slots[slot_first .. slot_first + n_slots); n_slots may be 0 */
    uint32_t reserved;           /* must be 0 */
} fs_listener;

typedef struct fs_accept_slot {  /* 12 bytes, no padding. HOST memory: what freeConnForReuse prepares */
    uint32_t iss;
    uint32_t rcv_wnd;
    uint16_t ip_id;              /* the ID seed: the frame carries prand16(ip_id) */
    uint16_t reserved;           /* must be 0 */
} fs_accept_slot;

typedef struct fs_accept_conn {  /* 48 bytes, no padding. DEVICE memory, n_slots entries, indexed by slot */
    uint8_t key[13];             /* wire order: the flow's key, what fs_rx_sock.key wants for the next call */
    uint8_t used;                /* 1: filled. A slot that was not filled is 48 zero bytes */
    uint8_t remote_mac[6];       /* the SYN's frame[6:12) */
    uint16_t peer_mss;
    uint16_t reserved;           /* written 0 */
    uint32_t frame;              /* batch index of the SYN */
    uint32_t flow;
    uint32_t irs;
    uint32_t rcv_nxt;            /* irs + 1 */
    uint32_t snd_nxt;            /* iss + 1 */
    uint32_t snd_wnd;            /* the SYN's raw Window field */
} fs_accept_conn;

typedef struct fs_listener_out { /* 16 bytes. DEVICE memory, n_listeners entries, all written */
    uint32_t n_syn;              /* candidates */
    uint32_t n_accepted;
    uint32_t n_full;             /* n_syn - n_accepted */
    uint32_t reserved;           /* written 0 */
} fs_listener_out;

fs_status fs_accept_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                                uint32_t n, uint32_t mtu, uint32_t flags, const fs_rx_sock* socks, uint32_t n_socks,
                                uint8_t* rings, uint64_t rings_bytes, fs_rx_sock_out* socks_out, uint8_t* delivered,
                                const fs_rx_snd* snd, fs_rx_snd_out* snd_out, uint8_t* code, const fs_listener* listeners,
                                uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots, uint32_t synack_flags,
                                fs_accept_conn* conns, fs_listener_out* listeners_out, uint32_t* accept_of,
                                uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status, uint8_t* payload,
                                uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order,
                                uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, void* stream);

/* fs_accept_flows_batch with every pointer in HOST memory, as fs_recv_flows_batch_host. The `synacks`
 * span (n_slots * FS_ACCEPT_STRIDE bytes), `synack_out` and `synack_status` go to the device first and
 * come back WHOLE, so that the bytes of unfilled slots, and the bytes behind a frame, keep the caller's
 * values. accept_of comes back whole (n entries). */
fs_status fs_accept_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                                     const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags,
                                     const fs_rx_sock* socks, uint32_t n_socks, uint8_t* rings, uint64_t rings_bytes,
                                     fs_rx_sock_out* socks_out, uint8_t* delivered, const fs_rx_snd* snd,
                                     fs_rx_snd_out* snd_out, uint8_t* code, const fs_listener* listeners,
                                     uint32_t n_listeners, const fs_accept_slot* slots, uint32_t n_slots,
                                     uint32_t synack_flags, fs_accept_conn* conns, fs_listener_out* listeners_out,
                                     uint32_t* accept_of, uint8_t* synacks, fs_digest* synack_out, uint8_t* synack_status,
                                     uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows,
                                     uint32_t* order, uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out,
                                     uint8_t* status);

#ifdef __cplusplus
}
#endif
#endif /* FRAMESUM_ACCEPT_H */
