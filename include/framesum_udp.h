/*
 * framesum -- UDP datagrams into per-port queues in one call (C ABI, eighth header beside framesum.h,
 * framesum_deliver.h, framesum_send.h, framesum_recv.h, framesum_accept.h, framesum_close.h and
 * framesum_connect.h).
 *
 * fs_udp_flows_batch is fs_connect_flows_batch plus the UDP half of PortStack.RecvEth: every accepted UDP
 * frame is matched to a listed PORT by its destination address and destination port, and its headers'
 * fields and its payload are copied into the next free CELL of that port's queue, in arrival order,
 * with the datagram's boundaries and its source kept. One RX call per batch then serves a whole
 * PortStack: the host no longer opens an accepted UDP frame.
 *
 * The reference code this restates: the UDP branch of RecvEth (stacks/portstack.go:222-281): the gates
 * that the verdict already carries (:222-245), findPort(ps.portsUDP, uhdr.DestinationPort) (:246), the
 * copy of the Ethernet, IPv4 and UDP headers and of the payload into ps.auxUDP (:262-270) and
 * port.ihandler.recv(pkt) (:281); the address gate `ps.ip == [4]byte{}` (:209); the MAC filter (:185);
 * UDPPacket.Payload() (stacks/port_udp.go:82-89). The benchmark of stacks/benchmark_test.go:12-46 ends
 * every iteration in that delivery.
 *
 * 1. Relation to fs_connect_flows_batch. This call runs that call's enqueue unchanged and adds launches
 *    behind it. Everything that call writes is byte for byte what it writes for the same arguments. With
 *    n_ports == 0 the only additions are the fills of port_of and cell_of with FS_UDP_NONE (where given).
 *    The flow-aware arrays still group the UDP frames by 5-tuple; a port takes datagrams from any source.
 *
 * 2. The records: fs_udp_port, fs_udp_cell and fs_udp_port_out below. A port's queue is the n_cells
 *    cells of cell_size bytes at cells + cells_off; `wcell` is the cell the next datagram goes to and
 *    `free` the number of cells the consumer has handed back. A cell is a 32-byte fs_udp_cell followed by
 *    `stored` payload bytes taken from frame[14 + 4 IHL + 8 ...). No byte of the cell behind them is
 *    written, and no byte of a cell that takes no datagram is written.
 *      len         TotalLength - 4 IHL - 8: the datagram's payload bytes as the IPv4 header counts them
 *                  (the slice of :262-270).
 *      stored      min(len, cell_size - 32): `copy(pkt.payload[:], payload)` (:270) copies no more than
 *                  its destination holds, and Payload() (port_udp.go:82-89) refuses uLen >
 *                  len(pkt.payload); a consumer sees stored < len and decides.
 *      udp_length  uhdr.Length as a number, so that the consumer can apply Payload()'s `ipLen != uLen`.
 *      src_port    the UDP source port as a number.
 *      src_ip, dst_ip, src_mac, dst_mac   wire order. dst_mac lets the host apply the MAC filter of
 *                  :185, which stays socket-layer policy (the verdict does not carry it).
 *
 * 3. Match. Frame i is matched to port p iff its verdict is FS_OK, frame[23] == 17, and ports[p].local
 *    equals the frame's destination address and destination port -- or no port's does and ports[p].local
 *    is 0.0.0.0 with that port (a PortStack without an address takes every destination, :209). An exact
 *    address wins over the wildcard. IP options do not exclude a frame (the port is read at 14 + 4 IHL +
 *    2). A UDP Length that disagrees with the IP length does not exclude a frame: the verdict already
 *    follows the reference's arithmetic there, and the cell carries both numbers. TCP frames to the same
 *    address and port are not matched.
 *
 * 4. Order and admission. The matched frames of a port are taken in ascending batch index, which is
 *    arrival order, whatever their source. The r-th (r from 0) is admitted iff r < free, and goes to cell
 *    (wcell + r) mod n_cells; the rest get FS_UDP_FULL. After the call wcell = (wcell + n_admitted) mod
 *    n_cells and free -= n_admitted: fs_udp_port_out carries both, with the counts, the batch index of
 *    the port's first matched frame and the sum of `stored`. n_truncated counts admitted datagrams with
 *    stored < len.
 *
 * 5. Determinism. Nothing in the result depends on a hash, on which lane runs first, or on the grid.
 *
 * 6. Difference from the reference. The reference has no queue: a port's handler takes one packet at a
 *    time (`port.ihandler.recv(pkt)`, :281, into the one ps.auxUDP) and drops a packet while one is
 *    pending. The queue of cells and FS_UDP_FULL are this call's batch form of that: with n_cells = 1
 *    and free = 1 a port takes the first matched datagram of a batch and refuses the rest, as the
 *    reference's handler does between two polls.
 *
 * 7. Degenerate sizes. n == 0: every ports_out entry carries the input wcell and free with zero counts
 *    and first = FS_UDP_NONE; the connect call's n == 0 behaviour (flagged openers' SYNs) stays.
 *    n_ports == 0: see 1.
 *
 * 8. FS_E_INVALID, checked on the host before any device work, each with a text in fs_last_error:
 *    everything fs_connect_flows_batch rejects; null ports, cells or ports_out with n_ports > 0; n_ports
 *    above FS_UDP_MAX_PORTS; reserved not 0; port 0; two ports with equal `local`; cell_size not a multiple
 *    of 8 in 40 .. 65,568; cells_off not a multiple of 8; n_cells outside 1 .. 2^31; wcell >= n_cells;
 *    free > n_cells; a queue that ends past cells_bytes; two queues that overlap.
 *
 * `ports` is HOST memory, consumed before the call returns (staged per call with its table in a block of
 * its own, as the listeners are); cells, ports_out, port_of and cell_of (both nullable, n entries each)
 * are DEVICE pointers. Asynchronous on `stream`; scratch rules are fs_connect_flows_batch's, and this call
 * adds 20 bytes per frame beside the sort's temporary storage. fs_ctx_set_workgroups caps the grids of
 * this call's kernels too.
 */
#ifndef FRAMESUM_UDP_H
#define FRAMESUM_UDP_H

#include "framesum_connect.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_UDP_NONE 0xFFFFFFFFu /* port_of / cell_of of a frame no port matched; fs_udp_port_out.first of a port without a frame */
#define FS_UDP_FULL 0xFFFFFFFEu /* cell_of of a matched frame that found no free cell */
#define FS_UDP_MAX_PORTS 65536u
#define FS_UDP_CELL_HEADER 32u

typedef struct fs_udp_port {     /* 32 bytes, no padding. HOST memory */
    uint8_t local[6];            /* destination address then destination port, wire order; address 0.0.0.0: any destination address; port 0 is invalid */
    uint8_t reserved[2];         /* must be 0 */
    uint32_t n_cells;            /* 1 .. 2^31 */
    uint32_t cell_size;          /* a multiple of 8, 40 .. 65,568 */
    uint64_t cells_off;          /* a multiple of 8: the queue is cells[cells_off : cells_off + n_cells * cell_size) */
    uint32_t wcell;              /* < n_cells: the cell the next datagram goes to */
    uint32_t free;               /* <= n_cells */
} fs_udp_port;

typedef struct fs_udp_cell {     /* 32 bytes, no padding; `stored` payload bytes follow */
    uint32_t frame;              /* batch index */
    uint16_t len;                /* TotalLength - 4 IHL - 8 */
    uint16_t stored;             /* min(len, cell_size - 32) */
    uint16_t udp_length;         /* uhdr.Length as a number */
    uint16_t src_port;           /* as a number */
    uint8_t src_ip[4], dst_ip[4], src_mac[6], dst_mac[6]; /* wire order */
} fs_udp_cell;

typedef struct fs_udp_port_out { /* 32 bytes, no padding. DEVICE memory, every entry written */
    uint32_t wcell, free;        /* the state after the call */
    uint32_t n_matched, n_admitted, n_truncated;
    uint32_t first;              /* batch index of the first matched frame, else FS_UDP_NONE */
    uint64_t bytes;              /* sum of `stored` */
} fs_udp_port_out;

fs_status fs_udp_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
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
                             uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order,
                             uint32_t* run_of, fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, void* stream);

/* fs_udp_flows_batch with every pointer in HOST memory, as fs_connect_flows_batch_host: the span of `cells`
 * that the listed queues cover goes to the device first and comes back, as the rings do; ports_out,
 * port_of and cell_of come back whole. */
fs_status fs_udp_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
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
                                  uint32_t* cell_of, uint8_t* payload, uint64_t payload_cap,
                                  fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order, uint32_t* run_of,
                                  fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status);

#ifdef __cplusplus
}
#endif
#endif /* FRAMESUM_UDP_H */
