/*
 * framesum — MI355X-native batched frame-checksum engine (C ABI).
 *
 * Drop-in boundary for the soypat/seqs per-frame checksum path. The Go
 * reference computes, for every frame through stacks.PortStack.RecvEth, the
 * RFC 791/1071 one's-complement checksums of eth/crc.go + eth/headers.go one
 * frame per synchronous call. This ABI replaces those per-frame calls with
 * one batched, device-resident call; the per-frame Go functions stay as they
 * are. Plain pointers and sizes only: no HIP, torch or C++
 * types cross the boundary, so cgo / ctypes / JNI can bind it directly
 * (INTEGRATION.md shows the bindings).
 *
 * Replaced reference interfaces (paths relative to the soypat/seqs root):
 *   fs_digest.l4_csum + fs verdict  <- stacks/portstack.go:239-244 (UDP) and
 *        :301-308 (TCP): `gotsum := uhdr.CalculateChecksumIPv4(&ihdr, payload)`
 *        / `thdr.CalculateChecksumIPv4(&ihdr, tcpOptions, payload)` and the
 *        compare that yields ErrChecksumTCPorUDP (portstack.go:132), together
 *        with the RecvEth gates that choose the L4 range (:167-214, :226-237,
 *        :285-299) and the verdict errors (:120-142).
 *   fs_digest.ip_csum               <- eth/headers.go:333-340
 *        (*IPv4Header).CalculateChecksum() applied to frame[14:34].
 *   the CRC791 arithmetic itself    <- eth/crc.go:13-84 (Write/AddUint16/
 *        AddUint32/AddUint8/Sum16/Reset), evaluated on the GPU.
 *   fs_digest.crc32                 <- NEW: IEEE 802.3 CRC-32 (Ethernet FCS)
 *        over frame[0:len). The reference has no CRC-32.
 *
 * Conventions (mirroring the reference's): pure functions over caller-owned
 * buffers, no retention after the call's stream work completes; malformed
 * frames are reported per frame in `status` (the RecvEth error class), never
 * as a call failure. Errors of the call itself are negative fs_status codes
 * (no exceptions cross the ABI); fs_last_error() gives the message.
 * Threading: one fs_ctx per host thread (a context is not internally locked).
 */
#ifndef FRAMESUM_H
#define FRAMESUM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRAMESUM_ABI_VERSION 1u

typedef int32_t fs_status;
#define FS_SUCCESS 0
#define FS_E_INVALID (-1)   /* bad argument (null pointer, n too large, ...) */
#define FS_E_HIP (-2)       /* HIP runtime error (message in fs_last_error) */
#define FS_E_NOMEM (-3)     /* device or pinned-host allocation failed */
#define FS_E_NODEVICE (-4)  /* no such device / device is not gfx950 */

/* Per-frame verdict written to `status` (stacks/portstack.go:120-142). The
 * stack model: MTU `mtu` (0 disables both MTU gates so jumbo frames can be
 * evaluated; the reference caps MTU at 2048, portstack.go:17,46-48), address
 * filters off (MAC :185-186 and IP destination :209-210 are socket-layer
 * policy, not checksum inputs), one UDP and one TCP port open. */
enum fs_verdict {
    FS_OK = 0,                          /* L4 checksum verified (RecvEth continues) */
    FS_ERR_PACKET_SMOL = 1,             /* errPacketSmol */
    FS_ERR_EXCEEDS_MTU = 2,             /* errPacketExceedsMTU */
    FS_IGNORED_NOT_IPV4 = 3,            /* RecvEth returns nil: not IPv4/ARP */
    FS_ARP = 4,                         /* ARP frame (no checksum) */
    FS_ERR_IP_VERSION = 5,              /* errIPVersion */
    FS_ERR_INVALID_IHL = 6,             /* errInvalidIHL */
    FS_ERR_BAD_IP_TOTAL_LEN_OR_IHL = 7, /* errBadIPTotalLenOrIHL */
    FS_ERR_UNKNOWN_IP_PROTO = 8,        /* errUnknownIPProto */
    FS_ERR_TOO_SHORT_TCP_OR_UDP = 9,    /* errTooShortTCPOrUDP */
    FS_ERR_ZERO_PORT = 10,              /* errZeroPort */
    FS_ERR_BAD_UDP_LENGTH = 11,         /* errBadUDPLength */
    FS_ERR_BAD_TCP_OFFSET = 12,         /* errBadTCPOffset */
    FS_ERR_CHECKSUM = 13,               /* ErrChecksumTCPorUDP */
    FS_ERR_FCS = 14                     /* fs_digest_batch_fcs only: FCS missing or wrong (the
                                           frame is dropped before RecvEth; not in the reference) */
};

/* 8-byte per-frame digest. crc32: IEEE CRC-32 of frame[0:len).
 * ip_csum: IPv4Header.CalculateChecksum() of frame[14:34] (0 if len < 34).
 * l4_csum: the TCP/UDP checksum RecvEth computes (`gotsum`), 0 when the frame
 * is rejected before the compare (status not FS_OK / FS_ERR_CHECKSUM). */
typedef struct fs_digest {
    uint32_t crc32;
    uint16_t ip_csum;
    uint16_t l4_csum;
} fs_digest;

typedef struct fs_ctx fs_ctx;

/* Library / device queries. */
uint32_t fs_abi_version(void);
int fs_device_count(void);

/* Context: owns the device copy of the CRC shift tables, a host-mapped report block (the
 * automatic kernel choice), the host-staged entry points' staging buffers and pinned mirrors,
 * and three internal streams for them (a compute stream and two copy streams). */
fs_status fs_ctx_create(int device, fs_ctx** out);
fs_status fs_ctx_destroy(fs_ctx* ctx);
/* Message for the last failing call on `ctx` (or of fs_ctx_create when ctx is NULL). */
const char* fs_last_error(const fs_ctx* ctx);

/* Every batched call takes at most 2^31 frames (n); larger n is FS_E_INVALID. */

/* Batched digest, device-resident. All pointers are DEVICE pointers.
 *   frame i = frames[offsets[i] : offsets[i] + lengths[i]]  (any byte alignment,
 *   frames may overlap or be sparse; the engine reads whole 64-byte-aligned
 *   blocks that hold frame bytes -- up to 63 bytes around a frame, never outside
 *   the memory pages that hold its bytes -- and ignores the bytes outside it).
 *   out[i] receives the digest; status (nullable) receives the fs_verdict.
 * Asynchronous on `stream` (a hipStream_t; NULL = the null stream). */
fs_status fs_digest_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                          uint32_t n, uint32_t mtu, fs_digest* out, uint8_t* status, void* stream);

/* TX checksum fill, device-resident and in place. The
 * reference fills a frame's checksums while it builds the frame from header structs:
 *   stacks/port_tcp.go:178 `pkt.IP.Checksum = pkt.IP.CalculateChecksum()` and :193
 *   `pkt.TCP.Checksum = pkt.TCP.CalculateChecksumIPv4(&pkt.IP, nil, payload)`;
 *   stacks/dhcp_client.go:479/:486 and dhcp_server.go:203/:216 (IP, then UDP).
 * For frames whose headers are already in place, flags:
 *   FS_FILL_CSUM  writes the IPv4 header checksum (eth/headers.go:333-340) to frame[24:26]
 *                 and the TCP/UDP checksum RecvEth verifies (the same arithmetic, with the
 *                 frame's own TCP options; none when the data offset is 5, as :193 passes
 *                 nil; frames with options are an extension of the reference's TX path,
 *                 parity unpinned) to the L4 checksum field, both big-endian, for every frame whose
 *                 RecvEth evaluation reaches the checksum compare (verdict FS_OK or
 *                 FS_ERR_CHECKSUM before the fill); other frames are not written.
 *   FS_FCS_APPEND writes the IEEE CRC-32 of the frame (as filled) little-endian at
 *                 frame[len:len+4), the FCS in wire order: those 4 bytes must be spare
 *                 (part of no frame of the batch).
 * out/status receive what fs_digest_batch would report for the frames as written (filled
 * frames: FS_OK). Frames must not overlap. Asynchronous on `stream`. */
#define FS_FILL_CSUM 1u
#define FS_FCS_APPEND 2u
fs_status fs_fill_batch(fs_ctx* ctx, uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths, uint32_t n,
                        uint32_t mtu, uint32_t flags, fs_digest* out, uint8_t* status, void* stream);

/* fs_fill_batch from/to HOST memory (the TX buffer a stack writes frames into): copies the
 * batch's byte span to the device, fills, copies the span back into `frames`, and returns
 * when the frames and `out`/`status` are written. frames_bytes bounds every frame (plus its
 * 4 FCS bytes with FS_FCS_APPEND). */
fs_status fs_fill_batch_host(fs_ctx* ctx, uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                             const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags, fs_digest* out,
                             uint8_t* status);

/* TX frame build, device-resident: TCP segmentation and UDP frame build in one fused pass (what
 * a NIC calls segmentation offload). The reference builds a TX frame in three steps that this
 * call does for a whole batch: stacks/port_tcp.go:162-194 TCPPacket.CalculateHeaders derives the
 * per-segment header fields, PutHeaders (port_tcp.go:95-106, port_udp.go:68-78) writes them in
 * front of a payload slice, and TCPConn.send cuts that slice from the socket's ring.
 *
 * A send is a header template and a payload range. It makes S frames: 1 when mss is 0 or the
 * payload is empty, else ceil(payload_len / mss); frame k carries payload bytes
 * [k*mss, min(payload_len, (k+1)*mss)) of the range (its chunk). Frame k's header is the template
 * with:
 *   IPv4  byte 0 written as 0x45 (eth/headers.go:289-291), TotalLength = 20 + 20 (UDP: 8) + chunk,
 *         ID = prand16 applied k times to the template's ID (port_tcp.go:173, :197-203: x ^= x<<7;
 *         x ^= x>>9; x ^= x<<8 on uint16), Checksum = CalculateChecksum of the header as written;
 *   TCP   Seq = template Seq + k*mss (mod 2^32), FIN and PSH cleared on every frame but the last (the
 *         usual segmentation rule: an extension, the reference's flags come from its ControlBlock),
 *         urgent pointer 0 (:189), Checksum = CalculateChecksumIPv4(&ip, nil, chunk);
 *   UDP   Length = 8 + payload_len, Checksum = CalculateChecksumIPv4 (a computed 0 is written as 0).
 * Every other header byte is copied. With FS_FCS_APPEND the frame's CRC-32 follows it little-endian.
 * Both checksums are written into every frame whose RecvEth evaluation reaches the checksum compare,
 * as FS_FILL_CSUM does; a frame RecvEth rejects earlier (a zero port, a frame above `mtu`, a
 * TotalLength that wraps the reference's uint16 `end`) gets zero checksum fields and its verdict.
 *
 * Layout: frames lie in send order, then segment order; each starts at a multiple of `align` (a
 * power of two, 1..4096) inside `frames` and owns a slot of round_up(len + (4 with FS_FCS_APPEND),
 * align) bytes; fs_segment_layout gives the frame count and the sum of the slots. Bytes of `frames`
 * that belong to no frame and no FCS are not written (not even read and written back).
 * offsets[i] / lengths[i] (without FCS) describe frame i as fs_digest_batch takes them; out / status
 * are what fs_digest_batch(..., mtu, ...) would report for it. Those four arrays may each be NULL.
 *
 * FS_E_INVALID, checked on the host before any device work (fs_segment_layout checks the same, less
 * the payload range): a null ctx, sends or frames; align or flags out of range; reserved not 0;
 * EtherType not 0x0800; IHL not 5; protocol not 6 or 17; TCP data offset not 5; UDP with mss not 0;
 * a chunk above 65,495 (TCP) or 65,507 (UDP) bytes; S above FS_SEGMENT_MAX_FRAMES; a payload range
 * outside payload_bytes; more than 2^31 frames; frames_bytes below the layout's. n_sends of 0 is
 * success and writes nothing.
 *
 * `sends` is HOST memory, consumed before the call returns; payload, frames, offsets, lengths, out
 * and status are DEVICE pointers. Asynchronous on `stream`. Calls on one context need no
 * synchronization between them, on one stream or several: each call stages its sends in a block of
 * its own that is reused only once its kernel has ended. fs_ctx_set_workgroups caps this kernel's
 * grid too (uncapped, it launches two 12-wave workgroups per compute unit); fs_ctx_set_kernel and
 * fs_ctx_last_kernel do not concern it. */
#define FS_SEGMENT_MAX_FRAMES 4096u /* frames one send may produce */

typedef struct fs_tx_send {  /* 72 bytes, no padding */
    uint8_t hdr[54];      /* Ethernet 14 + IPv4 20 (IHL 5) + TCP 20 (data offset 5), wire order, as
                             PutHeaders writes them. UDP: Ethernet + IPv4 + UDP 8 = the first 42 bytes */
    uint16_t mss;         /* TCP payload bytes per frame; 0: the whole payload in one frame */
    uint64_t payload_off; /* this send's payload = payload[payload_off : payload_off + payload_len) */
    uint32_t payload_len;
    uint32_t reserved;    /* must be 0 */
} fs_tx_send;

/* Host-only arithmetic: how many frames and how many bytes of `frames` a batch of sends needs. */
fs_status fs_segment_layout(const fs_tx_send* sends, uint32_t n_sends, uint32_t flags, uint32_t align,
                            uint64_t* n_frames, uint64_t* frames_bytes);

fs_status fs_segment_batch(fs_ctx* ctx, const fs_tx_send* sends, uint32_t n_sends, const uint8_t* payload,
                           uint64_t payload_bytes, uint32_t mtu, uint32_t flags, uint32_t align, uint8_t* frames,
                           uint64_t frames_bytes, uint64_t* offsets, uint32_t* lengths, fs_digest* out,
                           uint8_t* status, void* stream);

/* fs_segment_batch with every pointer in HOST memory: copies the payload to the device, builds the
 * frames, copies the frame span and the four arrays back (on the context's compute stream), and
 * returns when they are written. The bytes between frames keep the caller's values. */
fs_status fs_segment_batch_host(fs_ctx* ctx, const fs_tx_send* sends, uint32_t n_sends, const uint8_t* payload,
                                uint64_t payload_bytes, uint32_t mtu, uint32_t flags, uint32_t align,
                                uint8_t* frames, uint64_t frames_bytes, uint64_t* offsets, uint32_t* lengths,
                                fs_digest* out, uint8_t* status);

/* RX coalesce, device-resident: verify a batch and gather the payload of every accepted frame into one
 * contiguous buffer, reporting the runs of consecutive TCP segments that continue each other (what a
 * NIC calls LRO/GRO), so that a stack delivers one run per recv instead of one frame. The mirror of
 * fs_segment_batch: segmenting sends and coalescing the frames gives the sends' payload back. The
 * reference does this one frame at a time after RecvEth: stacks/portstack.go:217, :239 and :301-303
 * slice the payload out of the frame, and TCPConn.recv (stacks/tcpconn.go:347-369) checks that the
 * segment is the next in order and appends it to the socket's ring (`sock.rx.Write(payload)`, :369).
 *
 * out / status are bit for bit what fs_digest_batch(..., mtu, ...) reports for the batch, with
 * FS_RX_FCS what fs_digest_batch_fcs reports (lengths then include the 4-byte FCS): the call runs
 * that launch itself, automatic kernel choice and all. Either may be NULL and then goes to scratch
 * of the context.
 *
 * A frame is accepted iff its verdict is FS_OK. Its payload is what RecvEth hands to the port: UDP
 * frame[14 + IHL*4 + 8 : 14 + TotalLength), TCP frame[14 + IHL*4 + dataoff*4 : 14 + TotalLength).
 * It is IP-bounded (trailing Ethernet padding and the FCS are not part of it) and may be empty (a
 * pure ACK).
 *
 * `payload` receives the payloads of the accepted frames in batch order, back to back: a frame's
 * bytes start at the sum of the payload lengths of the accepted frames before it, and
 * totals->payload_bytes is the sum over all of them. A frame whose payload would end beyond
 * payload_cap is not copied: none of its bytes is written and nothing else about the result
 * changes, so the caller compares payload_bytes with payload_cap. Bytes of `payload` that belong to
 * no copied frame are not written (not even read and written back).
 *
 * Frame i joins frame i - 1 iff both are accepted, both are TCP with IHL 5 and data offset 5, both
 * payloads are non-empty, neither has SYN, RST or URG set, frame i - 1 has neither FIN nor PSH set,
 * Seq(i) == Seq(i - 1) + payload_len(i - 1) mod 2^32, and their 54-byte headers are equal in every
 * byte except the fields fs_segment_batch varies per segment: IPv4 TotalLength, ID and checksum, TCP
 * Seq, the FIN and PSH bits, and the TCP checksum (the fragment fields are compared as bytes, not
 * interpreted, as RecvEth does not interpret them). A run is a maximal chain of joined frames; an
 * accepted frame that joins nothing is a run of one (UDP, TCP with options, pure ACKs). Runs are
 * listed in order of first_frame: runs[0 .. totals->n_runs) are written, the entries beyond are not.
 * run_of[i] (nullable) is frame i's run index, or 0xFFFFFFFF for a frame that was not accepted.
 *
 * A run longer than 4 GiB: the join rule compares Seq modulo 2^32, so a chain may carry 2^32 bytes or
 * more (at least 65,592 frames), which the 32-bit fs_rx_run.payload_len cannot hold. Such a run is not
 * broken: its payload_len is its length modulo 2^32, and everything else stays exact: n_frames, the
 * payload itself, the next run's payload_off (so a run's length is also next.payload_off -
 * payload_off, or totals->payload_bytes - payload_off for the last run), fs_rx_flow.payload_len (64-bit)
 * and the totals. A caller that can meet such runs takes the length from there.
 *
 * FS_E_INVALID, checked on the host before any device work: a null ctx, frames, offsets, lengths,
 * runs or totals; a null payload with payload_cap not 0; flags other than 0 or FS_RX_FCS; n above
 * 2^31; frames not 4-byte aligned (as fs_digest_batch). n of 0 is success: it writes zero totals and
 * nothing else.
 *
 * All pointers are DEVICE pointers; `runs` has room for n entries. Asynchronous on `stream`. The
 * call's scratch (24 bytes per frame, and out / status when they are NULL) belongs to the context
 * and grows with n, so the coalesce calls of one context go on one stream or are ordered by the
 * caller; a call with a larger n than any before waits for the device while it reallocates.
 * fs_ctx_set_workgroups caps the grids of these kernels too (uncapped: up to 8 workgroups of 256
 * lanes per compute unit); fs_ctx_set_kernel applies to the digest launch only. */
#define FS_RX_FCS 1u /* frames carry their 4-byte FCS: verdicts as fs_digest_batch_fcs gives them */

typedef struct fs_rx_run {  /* 24 bytes, no padding */
    uint64_t payload_off;   /* the run's bytes are payload[payload_off : payload_off + payload_len) */
    uint32_t payload_len;   /* modulo 2^32 for a run of 4 GiB or more (above); payload_off is always exact */
    uint32_t first_frame;   /* batch index of the run's first frame */
    uint32_t n_frames;      /* frames first_frame .. first_frame + n_frames - 1, all accepted */
    uint8_t tcp_flags;      /* TCP: first frame's flags byte | (last frame's FIN, PSH); UDP: 0 */
    uint8_t reserved[3];    /* written as 0 */
} fs_rx_run;

typedef struct fs_rx_totals {
    uint64_t payload_bytes;
    uint32_t n_runs;
    uint32_t reserved;
} fs_rx_totals;

fs_status fs_coalesce_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                            uint32_t n, uint32_t mtu, uint32_t flags, uint8_t* payload, uint64_t payload_cap,
                            fs_rx_run* runs, uint32_t* run_of, fs_rx_totals* totals, fs_digest* out, uint8_t* status,
                            void* stream);

/* fs_coalesce_batch with every pointer in HOST memory: copies the batch's byte span (inside
 * frames_bytes, which bounds every frame) to the device, coalesces, copies the written part of the
 * payload, runs[0 .. n_runs), run_of, the totals, out and status back (on the context's compute
 * stream), and returns when they are written. `frames` needs no alignment here. */
fs_status fs_coalesce_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                                 const uint32_t* lengths, uint32_t n, uint32_t mtu, uint32_t flags, uint8_t* payload,
                                 uint64_t payload_cap, fs_rx_run* runs, uint32_t* run_of, fs_rx_totals* totals,
                                 fs_digest* out, uint8_t* status);

/* Flow-aware RX coalesce, device-resident: fs_coalesce_batch for traffic in which the segments of
 * several connections interleave (A0 B0 A1 B1 ...), where joining a segment only to the frame right
 * before it finds runs of one. The accepted frames are grouped by flow, each flow's payload is
 * gathered contiguously, and the runs are found inside each flow. The reference demultiplexes one
 * frame at a time: findPort(ps.portsTCP, thdr.DestinationPort) (stacks/portstack.go:309, :246 for
 * UDP) picks the socket, and TCPConn.recv checks the remote address and the in-order Seq before
 * sock.rx.Write(payload) (stacks/tcpconn.go:347-369).
 *
 * Verdicts and payload ranges: out / status, accepted (= FS_OK), a frame's payload range, FS_RX_FCS
 * and the payload_cap rule (a frame whose payload would end beyond payload_cap is not copied, and
 * nothing else about the result changes) are exactly fs_coalesce_batch's; the call runs the same
 * digest launch.
 *
 * The flow key of an accepted frame is 13 bytes: the protocol frame[23], the source and destination
 * IPv4 address frame[26 : 34), and the source and destination port frame[L4 : L4 + 4) with L4 = 14 +
 * 4 * IHL (with IP options the ports move). MAC addresses are not part of it. A flow is the set of
 * accepted frames with equal keys.
 *
 * Flows are numbered by the batch index of their first frame, ascending. The delivery order is flow
 * 0's frames in batch order, then flow 1's, and so on. order[k], for k < totals->n_accepted, is the
 * batch index of the k-th frame in delivery order; the entries beyond are not written. `order` is
 * required and has room for n entries; `flows` (room for n entries) may be NULL.
 *
 * `payload` receives the payloads back to back in delivery order, so a flow's bytes are contiguous.
 *
 * order[k] joins order[k - 1] under fs_coalesce_batch's join rule, unchanged. The header bytes it
 * compares include the key bytes of the frames that can join, so frames of different flows never
 * join. A frame that is not accepted belongs to no flow, and, unlike in fs_coalesce_batch, it does
 * not break a run by standing between two frames in the batch; if it carried bytes of the flow, the
 * Seq gap breaks the run.
 *
 * Runs are maximal chains, listed in delivery order: runs[0 .. totals->n_runs) are written. In a
 * run of this call first_frame is an index into `order`: the run's frames are order[first_frame ..
 * first_frame + n_frames). run_of[i] (nullable) is frame i's run index, or 0xFFFFFFFF for a frame
 * that was not accepted. flows[f], f < totals->n_flows, describes flow f: its bytes in `payload`,
 * its runs in `runs`, its frames in `order`.
 *
 * When every flow's frames are contiguous in the batch and no rejected frame stands between two
 * frames that join, payload, runs and run_of are byte for byte fs_coalesce_batch's, and order is
 * ascending. (A run's first_frame counts accepted frames here: it is the batch index when every
 * frame before the run is accepted, and order[first_frame] is the batch index always.)
 *
 * FS_E_INVALID, checked on the host before any device work: what fs_coalesce_batch rejects, a null
 * order, and n above 2^30 (the flow table's index stays 32-bit). n of 0 is success: it writes zero
 * totals and nothing else.
 *
 * All pointers are DEVICE pointers. Asynchronous on `stream`. The call's scratch belongs to the
 * context and grows with n, as fs_coalesce_batch's does (one stream, or ordered by the caller): 68
 * bytes per frame, 8 bytes per slot of the flow table (the power of two from 2 n up: 16 to 32
 * bytes per frame) and the sort's temporary storage (rocPRIM asks for 8 bytes per frame): 92 bytes
 * per frame at 65,536 frames; a call with a larger n than any before waits for the device while it
 * reallocates. fs_ctx_set_workgroups caps the grids of this call's own kernels; the sort's launches
 * are the rocPRIM library's and size themselves. */
typedef struct fs_rx_flow {      /* 32 bytes, no padding */
    uint64_t payload_off;        /* the flow's bytes: payload[payload_off : payload_off + payload_len) */
    uint64_t payload_len;
    uint32_t first_run, n_runs;  /* runs[first_run .. first_run + n_runs) */
    uint32_t first_frame, n_frames; /* order[first_frame .. first_frame + n_frames) */
} fs_rx_flow;

typedef struct fs_rx_flow_totals { /* 24 bytes */
    uint64_t payload_bytes;
    uint32_t n_runs, n_flows, n_accepted, reserved /* written 0 */;
} fs_rx_flow_totals;

fs_status fs_coalesce_flows_batch(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                                  uint32_t n, uint32_t mtu, uint32_t flags, uint8_t* payload, uint64_t payload_cap,
                                  fs_rx_run* runs, fs_rx_flow* flows, uint32_t* order, uint32_t* run_of,
                                  fs_rx_flow_totals* totals, fs_digest* out, uint8_t* status, void* stream);

/* fs_coalesce_flows_batch with every pointer in HOST memory, as fs_coalesce_batch_host: copies the
 * batch's byte span to the device, coalesces, copies the written part of the payload, runs[0 ..
 * n_runs), flows[0 .. n_flows), order[0 .. n_accepted), run_of, the totals, out and status back, and
 * returns when they are written. `frames` needs no alignment here. */
fs_status fs_coalesce_flows_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes,
                                       const uint64_t* offsets, const uint32_t* lengths, uint32_t n, uint32_t mtu,
                                       uint32_t flags, uint8_t* payload, uint64_t payload_cap, fs_rx_run* runs,
                                       fs_rx_flow* flows, uint32_t* order, uint32_t* run_of, fs_rx_flow_totals* totals,
                                       fs_digest* out, uint8_t* status);

/* RX of raw wire frames that still carry their 4-byte FCS (NICs that do not strip it;
 * SURVEY.md §8f rank 4, not in the reference): lengths[i] includes the FCS. out/status are
 * fs_digest_batch's for frame[0:len-4), the bytes RecvEth would receive, except that status
 * is FS_ERR_FCS when len < 4 or the little-endian FCS differs from that CRC-32. */
fs_status fs_digest_batch_fcs(fs_ctx* ctx, const uint8_t* frames, const uint64_t* offsets, const uint32_t* lengths,
                              uint32_t n, uint32_t mtu, fs_digest* out, uint8_t* status, void* stream);

/* Same computation from/to HOST memory (the NIC / loopback buffer handed to
 * RecvEth): stages H2D, runs the kernel and copies D2H on the context's
 * stream, returning when the results are in `out`/`status`. Pinned memory
 * (fs_host_alloc) gives full PCIe rate; pageable memory works (offsets, lengths, out and status
 * that are pinned are copied straight from / to, or written by the kernel in place, the others go
 * through the context's pinned mirror; an array counts as pinned only when all of it lies inside
 * one pinned allocation). With fs_ctx_set_kernel 0 or 8 a batch whose frames are all <= 128 bytes
 * runs the small-frame kernel: the lengths are on the host here; when its frames, offsets and
 * lengths are all pinned, that kernel reads them in place over PCIe (one launch, no copy). */
fs_status fs_digest_batch_host(fs_ctx* ctx, const uint8_t* frames, uint64_t frames_bytes, const uint64_t* offsets,
                               const uint32_t* lengths, uint32_t n, uint32_t mtu, fs_digest* out, uint8_t* status);

/* Multi-GPU form of fs_digest_batch_host for one host process (BASELINE configs[4]: frames
 * streamed from host memory to several GPUs; SURVEY.md §8b fs_digest_batch_multi). Replaces
 * the same per-frame calls as fs_digest_batch_host (stacks/portstack.go:163 RecvEth ->
 * :240 / :303 CalculateChecksumIPv4), for a NIC ring too large for one GPU's PCIe link.
 * The batch is cut into nctx contiguous blocks of frames holding about equal byte counts;
 * block k runs on ctxs[k] (one context per GPU; several contexts may share a GPU), every
 * block at once, each on its own host thread with its own H2D / kernel / D2H pipeline.
 * A block's digests and verdicts are copied straight into out/status at the block's own
 * indices: the host arrays are the gather, so no device collective is involved (the
 * device-resident RCCL form is fs_digest_batch_sharded below).
 * Blocks are runs of frames in BUFFER order: when the offsets are not non-decreasing, the
 * frames are first ordered by offset, so each context still copies only its own bytes.
 * ctxs must be distinct. Returns when every block is done; on failure, the status of the
 * lowest failing block, whose message is in fs_last_error of that block's context (every
 * entry point clears its context's message first, so only failing contexts hold one). */
fs_status fs_digest_batch_multi(fs_ctx* const* ctxs, int nctx, const uint8_t* frames, uint64_t frames_bytes,
                                const uint64_t* offsets, const uint32_t* lengths, uint32_t n, uint32_t mtu,
                                fs_digest* out, uint8_t* status);

/* ---- Device-resident multi-GPU form with RCCL (BASELINE configs[3], C4; SURVEY.md §8b
 * "N GPUs + RCCL gather", §8e). Replaces the same per-frame calls as fs_digest_batch
 * (stacks/portstack.go:163 RecvEth -> :240 / :303 CalculateChecksumIPv4) for a batch held
 * in the HBM of several GPUs of one node, driven from ONE host process (a Go PortStack):
 * frames are independent (eth/crc.go:12-17, CRC791 is per call), so the batch shards with
 * no data-path collective, and RCCL over xGMI is used only to gather the 8-byte digests and
 * 1-byte verdicts back to the first device.
 *
 * A group holds one context, one stream and one RCCL communicator (ncclCommInitAll) per
 * device; devices must be distinct. */
typedef struct fs_group fs_group;
fs_status fs_group_create(const int* devices, int ndev, fs_group** out);
fs_status fs_group_destroy(fs_group* g);
/* Message for the last failing call on `g` (or of fs_group_create when g is NULL). */
const char* fs_group_last_error(const fs_group* g);

/* Round-robin sharding of a global batch of n frames over nshards shards: global frame i
 * is local frame i / nshards of shard i % nshards; shard k holds fs_shard_count(n, nshards, k)
 * frames. */
uint64_t fs_shard_count(uint64_t n, uint32_t nshards, uint32_t shard);

/* Digest a global batch sharded round-robin over the group's devices. frames[k], offsets[k],
 * lengths[k] are DEVICE pointers on the group's k-th device describing shard k (its
 * fs_shard_count(n, ndev, k) frames, laid out as fs_digest_batch expects). The call works in
 * chunks of the shards' rows (at most 8, ~32K rows each). For each chunk, every device digests
 * its rows on its own compute stream; its digest and verdict pieces then go to the first
 * device by grouped point-to-point RCCL transfers (ncclSend / ncclRecv on a second stream per
 * device), and a de-interleave kernel there puts that chunk's frames in global order. So a
 * chunk's transfer and de-interleave overlap the next chunk's kernels. out (n digests) and
 * status (n bytes, nullable) are DEVICE pointers on the group's first device. Returns when
 * they are written; on an error return every stream of the group has been drained first, so
 * no work of the failed call is still in flight. At most 2^31 frames per shard. N > 1
 * devices has not run on hardware (the build boxes have one GPU). */
fs_status fs_digest_batch_sharded(fs_group* g, const uint8_t* const* frames, const uint64_t* const* offsets,
                                  const uint32_t* const* lengths, uint64_t n, uint32_t mtu, fs_digest* out,
                                  uint8_t* status);

/* The de-interleave step alone, for callers that gather the shards themselves (one process
 * per GPU, e.g. torch.distributed over RCCL): `gathered` (device memory of ctx's device)
 * holds nshards slabs back to back; slab k is shard k's m = ceil(n / nshards) digests (8 B
 * each) followed by its m verdict bytes, padded to a multiple of 256 bytes:
 * fs_shard_slab_bytes(n, nshards) bytes per slab. Writes out[i] / status[i] (nullable) for
 * global frames i < n. Asynchronous on `stream`. */
uint64_t fs_shard_slab_bytes(uint64_t n, uint32_t nshards);
fs_status fs_deinterleave(fs_ctx* ctx, const uint8_t* gathered, uint32_t nshards, uint64_t n, fs_digest* out,
                          uint8_t* status, void* stream);

/* Kernel variant of a context's launches. The engine has four kernels: a one-pass kernel for
 * batches of similar frame lengths (each frame read as the 64-byte blocks that hold it), a
 * mixed-length kernel that splits long frames into 768-byte pieces when a tile of 16 frames mixes
 * very different lengths, a segment kernel that cuts every frame of such a tile into equal chunks
 * (for tiles whose longest frame is beyond the pieces' reach, e.g. a 128-KB frame among 64-byte
 * ones), and a small-frame kernel (one lane per frame, small workgroups) for traffic of short
 * frames such as the reference's 47-byte benchmark frames. The kernels report whether a launch's
 * batch had mixed-length tiles (and whether one of them held such a giant frame) and whether it had
 * a frame longer than 128 bytes (sampled on steady traffic: each report is a store to host memory);
 * the host reads those reports a few launches late.
 *   0 (default): automatic. Mixed-length tiles select the mixed-length kernel (the segment kernel
 *     when the report says giant), similar lengths the one-pass kernel; after 16 launches seen to
 *     run with no frame over 128 bytes, the small-frame kernel, until a launch reports a longer frame.
 *   2 / 3 / 4: always the mixed-length / the segment / the one-pass kernel.
 *   8: the small-frame kernel preferred: it runs until a launch reports a frame over 128 bytes,
 *     then the automatic choice among the others until 2 launches have run short again.
 * The host-staged calls see every length: with 0 or 8 a batch whose frames are all <= 128 bytes
 * runs the small-frame kernel; with 0 or 8 a batch whose lengths all lie within 256 bytes of each other
 * runs the one-pass kernel from the context's first call; any other batch the automatic choice. A
 * TX fill never runs the small-frame kernel. Because reports arrive late, a launch of the
 * small-frame kernel can still meet long frames: they stay correct there but one lane streams each
 * of them (hundreds of us for a batch of jumbo frames). Any other variant is FS_E_INVALID. Results
 * are identical in every case; only the speed differs. */
fs_status fs_ctx_set_kernel(fs_ctx* ctx, int variant);

/* The kernel (2 mixed-length, 3 segment, 4 one-pass, 8 small-frame) the context's latest launch
 * ran; 0 before its first launch, FS_E_INVALID for a null context. With variant 0 a context's first
 * 16 device-resident launches run the mixed-length kernel (2), which keeps itself chosen while it
 * meets mixed tiles (moving to the segment kernel, 3, when they hold giant frames); uniform traffic
 * then moves to the one-pass kernel (4), and traffic of frames <= 128 bytes to the small-frame
 * kernel (8). The window costs uniform 1500-byte traffic about 1.5 us per launch (~23 us once per
 * context, measured on MI355X); mixed traffic it saves ~80 us per launch. A caller that knows its
 * device-resident traffic is uniform can set variant 4 (host-staged calls see the lengths and skip
 * the window for uniform batches by themselves). */
int fs_ctx_last_kernel(const fs_ctx* ctx);

/* Workgroups per launch of a context's kernels: 0 (the default) launches one 16-wave
 * workgroup per compute unit, so a batch of 65,536 frames gives every wave one tile of 16
 * frames; k > 0 caps the grid at k workgroups (at most one per CU), so each wave streams
 * several tiles back to back and consecutive launches on other streams run side by side on
 * the remaining CUs. A negative value is FS_E_INVALID. Results never depend on it. */
fs_status fs_ctx_set_workgroups(fs_ctx* ctx, int workgroups);

/* Pinned host memory helpers for fs_digest_batch_host callers. */
fs_status fs_host_alloc(fs_ctx* ctx, uint64_t bytes, void** out);
fs_status fs_host_free(fs_ctx* ctx, void* p);

#ifdef __cplusplus
}
#endif
#endif /* FRAMESUM_H */
