"""The framesum C ABI (include/framesum.h) as ctypes sees it: constants, record layouts, the
prototype table and the library loader. No torch here: seqs_amd/framesum.py builds the calls on it.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("FRAMESUM_LIB") or os.path.join(_HERE, "lib", "libframesum.so")

# The test library: the same sources built with -DFS_TEST_HOOKS (seqs_amd/csrc/Makefile), which adds
# the fault-injection setters fs_test_set_fault / fs_test_group_set_fault. Only tests load it; the
# product library has no such hook (and reads no environment variable for one).
TEST_LIB_PATH = os.path.join(_HERE, "lib", "test", "libframesum_test.so")

FS_SUCCESS = 0
FS_E_INVALID = -1
FS_E_HIP = -2
FS_E_NOMEM = -3
FS_E_NODEVICE = -4

# fs_verdict (include/framesum.h) — RecvEth error classes (stacks/portstack.go:120-142).
VERDICTS = {
    0: "OK",
    1: "errPacketSmol",
    2: "errPacketExceedsMTU",
    3: "ignored (not IPv4/ARP)",
    4: "ARP",
    5: "errIPVersion",
    6: "errInvalidIHL",
    7: "errBadIPTotalLenOrIHL",
    8: "errUnknownIPProto",
    9: "errTooShortTCPOrUDP",
    10: "errZeroPort",
    11: "errBadUDPLength",
    12: "errBadTCPOffset",
    13: "ErrChecksumTCPorUDP",
    14: "FCS missing or wrong (fs_digest_batch_fcs)",
}

# fs_fill_batch flags
FILL_CSUM = 1
FCS_APPEND = 2
FS_ERR_FCS = 14
# fs_coalesce_batch flag: the frames carry their 4-byte FCS
RX_FCS = 1
NO_RUN = 0xFFFFFFFF  # run_of of a frame that was not accepted

DIGEST_DTYPE = np.dtype([("crc32", "<u4"), ("ip_csum", "<u2"), ("l4_csum", "<u2")])
# fs_tx_send: one send of the TX frame build (72 bytes, no padding)
SEND_DTYPE = np.dtype([("hdr", "u1", (54,)), ("mss", "<u2"), ("payload_off", "<u8"), ("payload_len", "<u4"),
                       ("reserved", "<u4")])
SEGMENT_MAX_FRAMES = 4096
# fs_rx_run: one run of the RX coalesce (24 bytes, no padding), and fs_rx_totals (16 bytes)
RUN_DTYPE = np.dtype([("payload_off", "<u8"), ("payload_len", "<u4"), ("first_frame", "<u4"), ("n_frames", "<u4"),
                      ("tcp_flags", "u1"), ("reserved", "u1", (3,))])
TOTALS_DTYPE = np.dtype([("payload_bytes", "<u8"), ("n_runs", "<u4"), ("reserved", "<u4")])
# fs_rx_flow: one flow of the flow-aware RX coalesce (32 bytes, no padding), and fs_rx_flow_totals (24 bytes)
FLOW_DTYPE = np.dtype([("payload_off", "<u8"), ("payload_len", "<u8"), ("first_run", "<u4"), ("n_runs", "<u4"),
                       ("first_frame", "<u4"), ("n_frames", "<u4")])
FLOW_TOTALS_DTYPE = np.dtype([("payload_bytes", "<u8"), ("n_runs", "<u4"), ("n_flows", "<u4"), ("n_accepted", "<u4"),
                              ("reserved", "<u4")])
# fs_rx_sock: one socket of the in-order delivery (48 bytes, no padding), and fs_rx_sock_out (32 bytes)
SOCK_DTYPE = np.dtype([("key", "u1", (13,)), ("reserved", "u1", (3,)), ("rcv_nxt", "<u4"), ("rcv_wnd", "<u4"),
                       ("snd_nxt", "<u4"), ("ring_size", "<u4"), ("ring_off", "<u8"), ("ring_wpos", "<u4"),
                       ("ring_free", "<u4")])
SOCK_OUT_DTYPE = np.dtype([("rcv_nxt", "<u4"), ("ring_wpos", "<u4"), ("ring_free", "<u4"), ("bytes", "<u4"),
                           ("n_delivered", "<u4"), ("n_dropped", "<u4"), ("flow", "<u4"), ("stop", "<u4")])
DELIVER_MAX_SOCKS = 65536
NO_FLOW = 0xFFFFFFFF  # fs_rx_sock_out.flow / .stop of a socket without a flow in the batch
# fs_rx_snd: one socket's send side for the receive call (8 bytes), and fs_rx_snd_out (32 bytes, no padding)
SND_DTYPE = np.dtype([("snd_una", "<u4"), ("snd_wnd", "<u4")])
SND_OUT_DTYPE = np.dtype([("snd_una", "<u4"), ("snd_wnd", "<u4"), ("n_taken", "<u4"), ("n_dup", "<u4"), ("n_unsent", "<u4"),
                          ("n_rejected", "<u4"), ("n_keepalive", "<u4"), ("flags", "<u4")])
RECV_ACK_OWED, RECV_FIN = 1, 2  # fs_rx_snd_out.flags
# the per-frame codes of the receive call
RECV_NONE, RECV_TAKEN, RECV_DUPLICATE, RECV_UNSENT, RECV_REJECTED, RECV_KEEPALIVE, RECV_RING_FULL = range(7)
# The accept call (include/framesum_accept.h): fs_listener (24 bytes), fs_accept_slot (12), fs_accept_conn
# (48) and fs_listener_out (16), none with padding
LISTENER_DTYPE = np.dtype([("local", "u1", (6,)), ("mac", "u1", (6,)), ("slot_first", "<u4"), ("n_slots", "<u4"),
                           ("reserved", "<u4")])
ACCEPT_SLOT_DTYPE = np.dtype([("iss", "<u4"), ("rcv_wnd", "<u4"), ("ip_id", "<u2"), ("reserved", "<u2")])
ACCEPT_CONN_DTYPE = np.dtype([("key", "u1", (13,)), ("used", "u1"), ("remote_mac", "u1", (6,)), ("peer_mss", "<u2"),
                              ("reserved", "<u2"), ("frame", "<u4"), ("flow", "<u4"), ("irs", "<u4"), ("rcv_nxt", "<u4"),
                              ("snd_nxt", "<u4"), ("snd_wnd", "<u4")])
LISTENER_OUT_DTYPE = np.dtype([("n_syn", "<u4"), ("n_accepted", "<u4"), ("n_full", "<u4"), ("reserved", "<u4")])
ACCEPT_STRIDE = 64
ACCEPT_NONE, ACCEPT_FULL = 0xFFFFFFFF, 0xFFFFFFFE  # accept_of of a flow that is no candidate / found no slot
ACCEPT_MAX_LISTENERS = ACCEPT_MAX_SLOTS = 65536
# The close call (include/framesum_close.h): fs_cl_sock (40 bytes) and fs_cl_out (32), neither with padding
CLOSER_DTYPE = np.dtype([("key", "u1", (13,)), ("state", "u1"), ("reserved", "u1", (2,)), ("rcv_nxt", "<u4"),
                         ("rcv_wnd", "<u4"), ("snd_una", "<u4"), ("snd_nxt", "<u4"), ("snd_wnd", "<u4"), ("reserved2", "<u4")])
CLOSE_OUT_DTYPE = np.dtype([("state", "<u4"), ("rcv_nxt", "<u4"), ("snd_una", "<u4"), ("snd_wnd", "<u4"), ("n_taken", "<u4"),
                            ("n_rejected", "<u4"), ("stop", "<u4"), ("flags", "<u4")])
# the reference's state numbers (seqs.go:175-208)
ST_CLOSED, ST_ESTABLISHED, ST_FIN_WAIT_1, ST_FIN_WAIT_2, ST_CLOSING, ST_TIME_WAIT, ST_CLOSE_WAIT, ST_LAST_ACK = 0, 4, 5, 6, 7, 8, 9, 10
# the per-frame codes of the close call's ctl_code (1, 4 and 5 as the receive call's)
CLOSE_NONE, CLOSE_TAKEN, CLOSE_REJECTED, CLOSE_KEEPALIVE, CLOSE_DATA, CLOSE_IGNORED, CLOSE_RST, CLOSE_EXPECTED = 0, 1, 4, 5, 7, 8, 9, 10
CLOSE_ACK_OWED, CLOSE_FIN, CLOSE_RESET = 1, 2, 4  # fs_cl_out.flags
CLOSE_MAX_CLOSERS = 65536
# The connect call (include/framesum_connect.h): fs_cn_sock (40 bytes) and fs_cn_out (48), neither with padding
OPENER_DTYPE = np.dtype([("key", "u1", (13,)), ("flags", "u1"), ("reserved", "u1", (2,)), ("local_mac", "u1", (6,)),
                         ("remote_mac", "u1", (6,)), ("iss", "<u4"), ("rcv_wnd", "<u4"), ("ip_id", "<u2"), ("reserved2", "<u2")])
CONNECT_OUT_DTYPE = np.dtype([("state", "<u4"), ("irs", "<u4"), ("rcv_nxt", "<u4"), ("snd_una", "<u4"), ("snd_nxt", "<u4"),
                              ("snd_wnd", "<u4"), ("n_rejected", "<u4"), ("n_keepalive", "<u4"), ("stop", "<u4"),
                              ("frame", "<u4"), ("peer_mss", "<u2"), ("reply", "u1"), ("flags", "u1"), ("rst_seq", "<u4")])
ST_LISTEN, ST_SYN_RCVD, ST_SYN_SENT = 1, 2, 3  # the reference's state numbers before Established
CN_BAD_ACK = 11  # the connect call's own ctl_code value (1, 4, 5 and 10 keep their close-call names)
CN_SEND_SYN = 1  # fs_cn_sock.flags
CN_REPLY_NONE, CN_REPLY_ACK, CN_REPLY_SYNACK, CN_REPLY_RST, CN_REPLY_SYN = range(5)  # fs_cn_out.reply
CN_STOP_RST, CN_STOP_SYN = 1, 2  # fs_cn_out.flags
CONNECT_MAX_OPENERS = 65536
# The UDP call (include/framesum_udp.h): fs_udp_port (32 bytes), fs_udp_cell (the 32-byte header of a cell) and
# fs_udp_port_out (32), none with padding
UDP_PORT_DTYPE = np.dtype([("local", "u1", (6,)), ("reserved", "u1", (2,)), ("n_cells", "<u4"), ("cell_size", "<u4"),
                           ("cells_off", "<u8"), ("wcell", "<u4"), ("free", "<u4")])
UDP_CELL_DTYPE = np.dtype([("frame", "<u4"), ("len", "<u2"), ("stored", "<u2"), ("udp_length", "<u2"), ("src_port", "<u2"),
                           ("src_ip", "u1", (4,)), ("dst_ip", "u1", (4,)), ("src_mac", "u1", (6,)), ("dst_mac", "u1", (6,))])
UDP_PORT_OUT_DTYPE = np.dtype([("wcell", "<u4"), ("free", "<u4"), ("n_matched", "<u4"), ("n_admitted", "<u4"),
                               ("n_truncated", "<u4"), ("first", "<u4"), ("bytes", "<u8")])
UDP_NONE, UDP_FULL = 0xFFFFFFFF, 0xFFFFFFFE  # port_of / cell_of of a frame no port matched / that found no free cell
UDP_MAX_PORTS = 65536
UDP_CELL_HEADER = 32
# The ARP call (include/framesum_arp.h): fs_arp_host (20 bytes), fs_arp_query (12), fs_arp_host_out (16) and
# fs_arp_query_out (16), none with padding
ARP_HOST_DTYPE = np.dtype([("ip", "u1", (4,)), ("mac", "u1", (6,)), ("reserved", "<u2"), ("slot0", "<u4"), ("free", "<u4")])
ARP_QUERY_DTYPE = np.dtype([("host", "<u4"), ("target", "u1", (4,)), ("flags", "<u2"), ("reserved", "<u2")])
ARP_HOST_OUT_DTYPE = np.dtype([("n_requests", "<u4"), ("n_answered", "<u4"), ("first", "<u4"), ("free", "<u4")])
ARP_QUERY_OUT_DTYPE = np.dtype([("state", "u1"), ("reserved", "u1"), ("mac", "u1", (6,)), ("frame", "<u4"), ("n_replies", "<u4")])
ARP_NONE = 0xFFFFFFFF  # arp_of of a frame with no slot and no query; `first` and `frame` without a frame
ARP_MAX_HOSTS = ARP_MAX_QUERIES = ARP_MAX_REPLY_SLOTS = 65536
ARP_FRAME, ARP_FRAME_PADDED = 42, 60
ARP_PAD = 1  # arp_flags, beside FCS_APPEND
ARP_SEND_REQUEST = 1  # fs_arp_query.flags
ARP_NOT_ARP, ARP_UNSUPPORTED, ARP_IGNORED, ARP_ANSWERED, ARP_FULL, ARP_RESOLVED, ARP_STALE = range(7)  # arp_code
ARP_Q_WAIT, ARP_Q_DONE, ARP_Q_SENT = range(3)  # fs_arp_query_out.state
# fs_tx_sock: one socket of the ring send (104 bytes, no padding), and fs_tx_sock_out (32 bytes)
TX_SOCK_DTYPE = np.dtype([("hdr", "u1", (54,)), ("mss", "<u2"), ("ring_off", "<u8"), ("ring_size", "<u4"),
                          ("ring_rpos", "<u4"), ("ring_buffered", "<u4"), ("snd_una", "<u4"), ("snd_nxt", "<u4"),
                          ("snd_wnd", "<u4"), ("rcv_nxt", "<u4"), ("rcv_wnd", "<u4"), ("max_frames", "<u4"),
                          ("flags", "<u4")])
TX_SOCK_OUT_DTYPE = np.dtype([("snd_nxt", "<u4"), ("ring_rpos", "<u4"), ("ring_buffered", "<u4"), ("bytes", "<u4"),
                              ("n_frames", "<u4"), ("first_frame", "<u4"), ("ip_id", "<u4"), ("sent", "<u4")])
SEND_MAX_SOCKS = 65536
SEND_NONE = 0xFFFFFFFF  # fs_tx_sock_out.first_frame of a socket that made no frame
TX_ACK, TX_FIN, TX_PSH = 1, 2, 4  # fs_tx_sock.flags
# The resident ring send (include/framesum_send_resident.h): fs_tx_totals (40 bytes, no padding), the call
# flag, the two per-socket outcomes in fs_tx_sock_out.sent and the reasons of an invalid socket (bits 16..)
TX_TOTALS_DTYPE = np.dtype([("n_frames", "<u8"), ("frames_bytes", "<u8"), ("data_bytes", "<u8"), ("n_built", "<u4"),
                            ("n_idle", "<u4"), ("n_deferred", "<u4"), ("n_invalid", "<u4")])
TX_WRITEBACK = 0x100
TX_DEFERRED, TX_INVALID = 0x100, 0x200
TX_NO_RX = 0xFFFFFFFF  # an rx_index entry: the socket has no RX record
(TX_BAD_ETHERTYPE, TX_BAD_IHL, TX_BAD_PROTO, TX_BAD_DATA_OFFSET, TX_BAD_MSS, TX_BAD_SOCK_FLAGS, TX_BAD_MAX_FRAMES,
 TX_BAD_RING_SIZE, TX_BAD_RING_POS, TX_BAD_BUFFERED, TX_BAD_RING_RANGE, TX_BAD_RX_INDEX) = range(1, 13)


def sock_key(remote_ip, remote_port: int, local_ip, local_port: int) -> np.ndarray:
    """The 13-byte key of a TCP socket as its received frames carry it (fs_rx_sock.key): protocol 6,
    source = remote address, destination = local address, source = remote port, destination = local
    port. An address is 4 bytes, a dotted string or an integer."""
    def addr(a) -> bytes:
        if isinstance(a, str):
            a = bytes(int(x) for x in a.split("."))
        elif isinstance(a, int):
            a = a.to_bytes(4, "big")
        a = bytes(a)
        assert len(a) == 4, "an IPv4 address is 4 bytes"
        return a

    key = bytes([6]) + addr(remote_ip) + addr(local_ip) + int(remote_port).to_bytes(2, "big") + \
        int(local_port).to_bytes(2, "big")
    return np.frombuffer(key, dtype=np.uint8).copy()


class FramesumError(RuntimeError):
    pass


_st, _int, _u32, _u64, _str = ctypes.c_int32, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p
_p = ctypes.c_void_p  # any pointer, and hipStream_t
_pp, _pu64, _pint = ctypes.POINTER(_p), ctypes.POINTER(_u64), ctypes.POINTER(_int)

# name -> (restype, argtypes): every function include/framesum.h declares, in its order (checked
# against the header by tests/test_abi.py and tests/test_binding_prototypes.py).
PROTOTYPES = {
    "fs_abi_version": (_u32, []),
    "fs_device_count": (_int, []),
    "fs_ctx_create": (_st, [_int, _pp]),
    "fs_ctx_destroy": (_st, [_p]),
    "fs_last_error": (_str, [_p]),
    "fs_digest_batch": (_st, [_p, _p, _p, _p, _u32, _u32, _p, _p, _p]),
    "fs_fill_batch": (_st, [_p, _p, _p, _p, _u32, _u32, _u32, _p, _p, _p]),
    "fs_fill_batch_host": (_st, [_p, _p, _u64, _p, _p, _u32, _u32, _u32, _p, _p]),
    "fs_segment_layout": (_st, [_p, _u32, _u32, _u32, _pu64, _pu64]),
    "fs_segment_batch": (_st, [_p, _p, _u32, _p, _u64, _u32, _u32, _u32, _p, _u64, _p, _p, _p, _p, _p]),
    "fs_segment_batch_host": (_st, [_p, _p, _u32, _p, _u64, _u32, _u32, _u32, _p, _u64, _p, _p, _p, _p]),
    "fs_coalesce_batch": (_st, [_p, _p, _p, _p, _u32, _u32, _u32, _p, _u64, _p, _p, _p, _p, _p, _p]),
    "fs_coalesce_batch_host": (_st, [_p, _p, _u64, _p, _p, _u32, _u32, _u32, _p, _u64, _p, _p, _p, _p, _p]),
    "fs_coalesce_flows_batch": (_st, [_p, _p, _p, _p, _u32, _u32, _u32, _p, _u64, _p, _p, _p, _p, _p, _p, _p, _p]),
    "fs_coalesce_flows_batch_host": (_st, [_p, _p, _u64, _p, _p, _u32, _u32, _u32, _p, _u64, _p, _p, _p, _p, _p, _p, _p]),
    "fs_digest_batch_fcs": (_st, [_p, _p, _p, _p, _u32, _u32, _p, _p, _p]),
    "fs_digest_batch_host": (_st, [_p, _p, _u64, _p, _p, _u32, _u32, _p, _p]),
    "fs_digest_batch_multi": (_st, [_pp, _int, _p, _u64, _p, _p, _u32, _u32, _p, _p]),
    "fs_group_create": (_st, [_pint, _int, _pp]),
    "fs_group_destroy": (_st, [_p]),
    "fs_group_last_error": (_str, [_p]),
    "fs_shard_count": (_u64, [_u64, _u32, _u32]),
    "fs_digest_batch_sharded": (_st, [_p, _pp, _pp, _pp, _u64, _u32, _p, _p]),
    "fs_shard_slab_bytes": (_u64, [_u64, _u32]),
    "fs_deinterleave": (_st, [_p, _p, _u32, _u64, _p, _p, _p]),
    "fs_ctx_set_kernel": (_st, [_p, _int]),
    "fs_ctx_last_kernel": (_int, [_p]),
    "fs_ctx_set_workgroups": (_st, [_p, _int]),
    "fs_host_alloc": (_st, [_p, _u64, _pp]),
    "fs_host_free": (_st, [_p, _p]),
}
EXPORTED_SYMBOLS = tuple(PROTOTYPES)

# The functions include/framesum_deliver.h declares (the second header), in its order. Product
# symbols like the ones above: a library that lacks one raises in load_library.
DELIVER_PROTOTYPES = {
    "fs_deliver_flows_batch": (_st, [_p, _p, _p, _p, _u32, _u32, _u32, _p, _u32, _p, _u64, _p, _p, _p, _u64, _p, _p, _p,
                                     _p, _p, _p, _p, _p]),
    "fs_deliver_flows_batch_host": (_st, [_p, _p, _u64, _p, _p, _u32, _u32, _u32, _p, _u32, _p, _u64, _p, _p, _p, _u64, _p,
                                          _p, _p, _p, _p, _p, _p]),
}

# The functions include/framesum_send.h declares (the third header), in its order: product symbols too.
SEND_RINGS_PROTOTYPES = {
    "fs_send_rings_layout": (_st, [_p, _u32, _u32, _u32, _pu64, _pu64, _p]),
    "fs_send_rings_batch": (_st, [_p, _p, _u32, _p, _u64, _u32, _u32, _u32, _p, _u64, _p, _p, _p, _p, _p, _p]),
    "fs_send_rings_batch_host": (_st, [_p, _p, _u32, _p, _u64, _u32, _u32, _u32, _p, _u64, _p, _p, _p, _p, _p]),
}

# The functions include/framesum_recv.h declares (the fourth header), in its order: product symbols too.
# The delivery's prototypes with `snd`, `snd_out` and `code` behind `delivered`.
RECV_PROTOTYPES = {
    "fs_recv_flows_batch": (_st, [_p, _p, _p, _p, _u32, _u32, _u32, _p, _u32, _p, _u64, _p, _p, _p, _p, _p, _p, _u64, _p, _p,
                                  _p, _p, _p, _p, _p, _p]),
    "fs_recv_flows_batch_host": (_st, [_p, _p, _u64, _p, _p, _u32, _u32, _u32, _p, _u32, _p, _u64, _p, _p, _p, _p, _p, _p, _u64,
                                       _p, _p, _p, _p, _p, _p, _p]),
}

# The functions include/framesum_accept.h declares (the fifth header), in its order: product symbols too.
# The receive call's prototypes with listeners, n_listeners, slots, n_slots, synack_flags, conns,
# listeners_out, accept_of, synacks, synack_out and synack_status behind `code`.
ACCEPT_PROTOTYPES = {
    "fs_accept_flows_batch": (_st, [_p, _p, _p, _p, _u32, _u32, _u32, _p, _u32, _p, _u64, _p, _p, _p, _p, _p,
                                    _p, _u32, _p, _u32, _u32, _p, _p, _p, _p, _p, _p,
                                    _p, _u64, _p, _p, _p, _p, _p, _p, _p, _p]),
    "fs_accept_flows_batch_host": (_st, [_p, _p, _u64, _p, _p, _u32, _u32, _u32, _p, _u32, _p, _u64, _p, _p, _p, _p, _p,
                                         _p, _u32, _p, _u32, _u32, _p, _p, _p, _p, _p, _p,
                                         _p, _u64, _p, _p, _p, _p, _p, _p, _p]),
}

# The functions include/framesum_close.h declares (the sixth header), in its order: product symbols too.
# The accept call's prototypes with closers, n_closers, closers_out, socks_close and ctl_code behind
# `synack_status`.
CLOSE_PROTOTYPES = {
    "fs_close_flows_batch": (_st, [_p, _p, _p, _p, _u32, _u32, _u32, _p, _u32, _p, _u64, _p, _p, _p, _p, _p,
                                   _p, _u32, _p, _u32, _u32, _p, _p, _p, _p, _p, _p,
                                   _p, _u32, _p, _p, _p,
                                   _p, _u64, _p, _p, _p, _p, _p, _p, _p, _p]),
    "fs_close_flows_batch_host": (_st, [_p, _p, _u64, _p, _p, _u32, _u32, _u32, _p, _u32, _p, _u64, _p, _p, _p, _p, _p,
                                        _p, _u32, _p, _u32, _u32, _p, _p, _p, _p, _p, _p,
                                        _p, _u32, _p, _p, _p,
                                        _p, _u64, _p, _p, _p, _p, _p, _p, _p]),
}

# The functions include/framesum_connect.h declares (the seventh header), in its order: product symbols too.
# The close call's prototypes with openers, n_openers, reply_flags, openers_out, replies, reply_out and
# reply_status behind `ctl_code`.
CONNECT_PROTOTYPES = {
    "fs_connect_flows_batch": (_st, [_p, _p, _p, _p, _u32, _u32, _u32, _p, _u32, _p, _u64, _p, _p, _p, _p, _p,
                                     _p, _u32, _p, _u32, _u32, _p, _p, _p, _p, _p, _p,
                                     _p, _u32, _p, _p, _p,
                                     _p, _u32, _u32, _p, _p, _p, _p,
                                     _p, _u64, _p, _p, _p, _p, _p, _p, _p, _p]),
    "fs_connect_flows_batch_host": (_st, [_p, _p, _u64, _p, _p, _u32, _u32, _u32, _p, _u32, _p, _u64, _p, _p, _p, _p, _p,
                                          _p, _u32, _p, _u32, _u32, _p, _p, _p, _p, _p, _p,
                                          _p, _u32, _p, _p, _p,
                                          _p, _u32, _u32, _p, _p, _p, _p,
                                          _p, _u64, _p, _p, _p, _p, _p, _p, _p]),
}

# The functions include/framesum_udp.h declares (the eighth header), in its order: product symbols too.
# The connect call's prototypes with ports, n_ports, cells, cells_bytes, ports_out, port_of and cell_of
# behind `reply_status`.
UDP_PROTOTYPES = {
    "fs_udp_flows_batch": (_st, [_p, _p, _p, _p, _u32, _u32, _u32, _p, _u32, _p, _u64, _p, _p, _p, _p, _p,
                                 _p, _u32, _p, _u32, _u32, _p, _p, _p, _p, _p, _p,
                                 _p, _u32, _p, _p, _p,
                                 _p, _u32, _u32, _p, _p, _p, _p,
                                 _p, _u32, _p, _u64, _p, _p, _p,
                                 _p, _u64, _p, _p, _p, _p, _p, _p, _p, _p]),
    "fs_udp_flows_batch_host": (_st, [_p, _p, _u64, _p, _p, _u32, _u32, _u32, _p, _u32, _p, _u64, _p, _p, _p, _p, _p,
                                      _p, _u32, _p, _u32, _u32, _p, _p, _p, _p, _p, _p,
                                      _p, _u32, _p, _p, _p,
                                      _p, _u32, _u32, _p, _p, _p, _p,
                                      _p, _u32, _p, _u64, _p, _p, _p,
                                      _p, _u64, _p, _p, _p, _p, _p, _p, _p]),
}

# The functions include/framesum_arp.h declares (the ninth header), in its order: product symbols too.
# The UDP call's prototypes with hosts, n_hosts, queries, n_queries, n_reply_slots, arp_flags, hosts_out,
# queries_out, arp_frames, arp_out, arp_status, arp_code and arp_of behind `cell_of`.
_ARP_ARGS = [_p, _u32, _p, _u32, _u32, _u32, _p, _p, _p, _p, _p, _p, _p]
ARP_PROTOTYPES = {
    "fs_arp_flows_batch": (_st, UDP_PROTOTYPES["fs_udp_flows_batch"][1][:46] + _ARP_ARGS
                           + UDP_PROTOTYPES["fs_udp_flows_batch"][1][46:]),
    "fs_arp_flows_batch_host": (_st, UDP_PROTOTYPES["fs_udp_flows_batch_host"][1][:47] + _ARP_ARGS
                                + UDP_PROTOTYPES["fs_udp_flows_batch_host"][1][47:]),
}

# The function include/framesum_send_resident.h declares (the tenth header): a product symbol too.
SEND_RESIDENT_PROTOTYPES = {
    "fs_send_rings_resident": (_st, [_p, _p, _u32, _p, _p, _p, _u32, _p, _u64, _u32, _u32, _u32, _p, _u64, _u32,
                                     _p, _p, _p, _p, _p, _p, _p]),
}

# Not in the header, set only where the loaded library has them: the test library's hooks
# (-DFS_TEST_HOOKS) and the diagnostic build's stamp reader (tools/stamps.py).
OPTIONAL_PROTOTYPES = {
    "fs_test_set_fault": (_st, [_p, ctypes.c_long]),
    "fs_test_group_set_fault": (_st, [_p, ctypes.c_long]),
    "fs_test_group_set_fault_gather": (_st, [_p, ctypes.c_long]),
    "fs_test_set_kernel_exact": (_st, [_p, _int]),
    "fs_test_last_host_path": (_int, [_p]),
    "fs_test_set_flow_hash_mask": (_st, [_p, _u32]),
    "fs_test_set_flow_steps": (_st, [_p, _u32]),
    "fs_debug_read_stamps": (_int, [_p, ctypes.c_size_t]),
}
# In the header, yet tolerated when absent: older builds of the library in same-box A/B runs lack it.
_MAY_BE_ABSENT = ("fs_ctx_set_workgroups",)

_lib = None
_libs: dict = {}


def lib_path() -> str:
    return _LIB_PATH


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """Load libframesum.so (raises if it was not built: no fallback path exists). `path`: another
    build of the same ABI (the test library, TEST_LIB_PATH)."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    p = path or _LIB_PATH
    if p in _libs:
        return _libs[p]
    if not os.path.exists(p):
        raise FramesumError(f"{p} is missing — run __graft_entry__.build() (or make -C seqs_amd/csrc)")
    lib = ctypes.CDLL(p)
    tables = {**PROTOTYPES, **DELIVER_PROTOTYPES, **SEND_RINGS_PROTOTYPES, **RECV_PROTOTYPES, **ACCEPT_PROTOTYPES,
              **CLOSE_PROTOTYPES, **CONNECT_PROTOTYPES, **UDP_PROTOTYPES, **ARP_PROTOTYPES,
              **SEND_RESIDENT_PROTOTYPES, **OPTIONAL_PROTOTYPES}
    for name, (restype, argtypes) in tables.items():
        if (name in OPTIONAL_PROTOTYPES or name in _MAY_BE_ABSENT) and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # (a missing product symbol raises here)
        fn.restype, fn.argtypes = restype, argtypes
    _libs[p] = lib
    if path is None:
        _lib = lib
    return lib
