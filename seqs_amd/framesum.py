"""Host-side binding of the framesum C ABI (include/framesum.h).

This is the Python mirror of the reference's batch surface: `digest_batch`
plays the role of running `stacks.PortStack.RecvEth`'s checksum gates plus
`eth.(*IPv4Header).CalculateChecksum` / `(*UDPHeader|*TCPHeader).CalculateChecksumIPv4`
(eth/headers.go:333, :382, :510) over many frames at once, and
`recv_eth_batch` returns the per-frame RecvEth error class
(stacks/portstack.go:120-142). All digests are computed by the gfx950 kernel
in seqs_amd/lib/libframesum.so; there is no CPU fallback — if the library or a
gfx950 device is missing, the calls raise.

The constants, record layouts, prototypes and the loader live in seqs_amd/abi.py
and are re-exported here. torch is used only as device-memory / stream plumbing.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from .abi import (  # noqa: F401 (re-exported: this module is the binding's public face)
    ACCEPT_CONN_DTYPE, ACCEPT_FULL, ACCEPT_MAX_LISTENERS, ACCEPT_MAX_SLOTS, ACCEPT_NONE, ACCEPT_PROTOTYPES, ACCEPT_SLOT_DTYPE,
    ACCEPT_STRIDE, LISTENER_DTYPE, LISTENER_OUT_DTYPE,
    CLOSE_ACK_OWED, CLOSE_DATA, CLOSE_EXPECTED, CLOSE_FIN, CLOSE_IGNORED, CLOSE_KEEPALIVE, CLOSE_MAX_CLOSERS, CLOSE_NONE,
    CLOSE_OUT_DTYPE, CLOSE_PROTOTYPES, CLOSE_REJECTED, CLOSE_RESET, CLOSE_RST, CLOSE_TAKEN, CLOSER_DTYPE,
    ST_CLOSED, ST_CLOSE_WAIT, ST_CLOSING, ST_ESTABLISHED, ST_FIN_WAIT_1, ST_FIN_WAIT_2, ST_LAST_ACK, ST_TIME_WAIT,
    CN_BAD_ACK, CN_REPLY_ACK, CN_REPLY_NONE, CN_REPLY_RST, CN_REPLY_SYN, CN_REPLY_SYNACK, CN_SEND_SYN, CN_STOP_RST, CN_STOP_SYN,
    CONNECT_MAX_OPENERS, CONNECT_OUT_DTYPE, CONNECT_PROTOTYPES, OPENER_DTYPE, ST_LISTEN, ST_SYN_RCVD, ST_SYN_SENT,
    DELIVER_MAX_SOCKS, DELIVER_PROTOTYPES, DIGEST_DTYPE, EXPORTED_SYMBOLS, FCS_APPEND, FILL_CSUM, FLOW_DTYPE,
    FLOW_TOTALS_DTYPE, FS_E_HIP, FS_E_INVALID, FS_E_NODEVICE, FS_E_NOMEM, FS_ERR_FCS, FS_SUCCESS, NO_FLOW, NO_RUN,
    PROTOTYPES, RECV_ACK_OWED, RECV_DUPLICATE, RECV_FIN, RECV_KEEPALIVE, RECV_NONE, RECV_PROTOTYPES, RECV_REJECTED,
    RECV_RING_FULL, RECV_TAKEN, RECV_UNSENT, RUN_DTYPE, RX_FCS, SEGMENT_MAX_FRAMES, SEND_DTYPE, SEND_MAX_SOCKS, SEND_NONE,
    SEND_RINGS_PROTOTYPES, SND_DTYPE, SND_OUT_DTYPE, SOCK_DTYPE, SOCK_OUT_DTYPE, TEST_LIB_PATH, TOTALS_DTYPE, TX_ACK, TX_FIN,
    TX_PSH, TX_SOCK_DTYPE, TX_SOCK_OUT_DTYPE, VERDICTS, FramesumError, lib_path, load_library, sock_key,
    UDP_CELL_DTYPE, UDP_CELL_HEADER, UDP_FULL, UDP_MAX_PORTS, UDP_NONE, UDP_PORT_DTYPE, UDP_PORT_OUT_DTYPE, UDP_PROTOTYPES,
    ARP_ANSWERED, ARP_FRAME, ARP_FRAME_PADDED, ARP_FULL, ARP_HOST_DTYPE, ARP_HOST_OUT_DTYPE, ARP_IGNORED, ARP_MAX_HOSTS,
    ARP_MAX_QUERIES, ARP_MAX_REPLY_SLOTS, ARP_NONE, ARP_NOT_ARP, ARP_PAD, ARP_PROTOTYPES, ARP_Q_DONE, ARP_Q_SENT, ARP_Q_WAIT,
    ARP_QUERY_DTYPE, ARP_QUERY_OUT_DTYPE, ARP_RESOLVED, ARP_SEND_REQUEST, ARP_STALE, ARP_UNSUPPORTED,
    SEND_RESIDENT_PROTOTYPES, TX_TOTALS_DTYPE, TX_WRITEBACK, TX_DEFERRED, TX_INVALID, TX_NO_RX,
    TX_BAD_ETHERTYPE, TX_BAD_IHL, TX_BAD_PROTO, TX_BAD_DATA_OFFSET, TX_BAD_MSS, TX_BAD_SOCK_FLAGS, TX_BAD_MAX_FRAMES,
    TX_BAD_RING_SIZE, TX_BAD_RING_POS, TX_BAD_BUFFERED, TX_BAD_RING_RANGE, TX_BAD_RX_INDEX,
)

_vp, _u64 = ctypes.c_void_p, ctypes.c_uint64


def _tensor_ptr(t):
    return _vp(t.data_ptr())


def _array_ptr(a: np.ndarray):
    return a.ctypes.data_as(_vp)


def _stream_ptr(stream):
    return _vp(stream.cuda_stream)


def _result_tensors(n: int, device, out, status):
    """(out (n, 2) int32, status (n,) uint8) on `device`: the caller's, else new ones."""
    import torch

    if out is None:
        out = torch.empty((n, 2), dtype=torch.int32, device=device)
    if status is None:
        status = torch.empty((n,), dtype=torch.uint8, device=device)
    return out, status


def _host_batch(frames, offsets, lengths, writable: bool = False):
    """(frames uint8, offsets uint64, lengths uint32, n) as C-contiguous arrays. `writable`: the call
    writes into `frames`, which therefore is taken as it is and must be such an array already."""
    if writable:
        assert isinstance(frames, np.ndarray) and frames.dtype == np.uint8 and frames.flags["C_CONTIGUOUS"]
        assert frames.flags["WRITEABLE"], "fill_host writes into `frames`"
    else:
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    n = int(lengths.size)
    assert offsets.size == n, "offsets and lengths must describe the same frames"
    return frames, offsets, lengths, n


def _host_head(frames, offsets, lengths, n):
    """The arguments every host-form batch call starts with, after its context(s)."""
    return _array_ptr(frames), frames.nbytes, _array_ptr(offsets), _array_ptr(lengths), n


# The RX calls: (the device form's C function, the host form adds "_host"; the totals record; the
# arrays between `runs` and `run_of`, each with the totals field that counts its entries). The
# delivery call is the flow call with its socket arguments between `flags` and `payload`.
_RX = ("fs_coalesce_batch", TOTALS_DTYPE, ())
_RX_FLOWS = ("fs_coalesce_flows_batch", FLOW_TOTALS_DTYPE,
             ((FLOW_DTYPE, "n_flows"), (np.dtype(np.uint32), "n_accepted")))
_RX_DELIVER = ("fs_deliver_flows_batch", *_RX_FLOWS[1:])
_RX_RECV = ("fs_recv_flows_batch", *_RX_FLOWS[1:])  # (the delivery call with snd, snd_out and code behind delivered)
_RX_ACCEPT = ("fs_accept_flows_batch", *_RX_FLOWS[1:])  # (the receive call with the listening arguments behind code)
_RX_CLOSE = ("fs_close_flows_batch", *_RX_FLOWS[1:])  # (the accept call with the closing arguments behind synack_status)
_RX_CONNECT = ("fs_connect_flows_batch", *_RX_FLOWS[1:])  # (the close call with the opening arguments behind ctl_code)
_RX_UDP = ("fs_udp_flows_batch", *_RX_FLOWS[1:])  # (the connect call with the port arguments behind reply_status)
_RX_ARP = ("fs_arp_flows_batch", *_RX_FLOWS[1:])  # (the UDP call with the host and query arguments behind cell_of)


@dataclass
class Digest:
    """One frame's results (fs_digest + verdict)."""

    crc32: int
    ip_csum: int
    l4_csum: int
    verdict: int

    @property
    def err(self) -> Optional[str]:
        return None if self.verdict == 0 else VERDICTS.get(self.verdict, f"verdict {self.verdict}")


class _Handle:
    """Owner of one C handle: attribute `_attr` of the instance, destroyed by `lib.<_destroy>`."""

    _attr = _destroy = ""

    def close(self) -> None:
        h = getattr(self, self._attr, None)
        if h:
            getattr(self.lib, self._destroy)(h)
            setattr(self, self._attr, None)

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass


class Engine(_Handle):
    """One framesum context on one GPU (fs_ctx). Not thread-safe, like the C ctx."""

    _attr, _destroy = "_ctx", "fs_ctx_destroy"

    def __init__(self, device: int = 0, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        self.device = device
        ctx = _vp()
        st = self.lib.fs_ctx_create(device, ctypes.byref(ctx))
        if st != FS_SUCCESS:
            raise FramesumError(f"fs_ctx_create({device}) failed ({st}): {self.lib.fs_last_error(None).decode()}")
        self._ctx = ctx
        self._pinned: set[int] = set()

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            for addr in list(self._pinned):
                self.lib.fs_host_free(self._ctx, _vp(addr))
            self._pinned.clear()
        super().close()

    def _check(self, st: int, what: str) -> None:
        if st != FS_SUCCESS:
            raise FramesumError(f"{what} failed ({st}): {self.lib.fs_last_error(self._ctx).decode()}")

    # kernel variants (fs_ctx_set_kernel): results are identical, only the speed differs
    KERNEL_AUTO, KERNEL_MIXED, KERNEL_SEGMENTS, KERNEL_ONE_PASS, KERNEL_SMALL = 0, 2, 3, 4, 8

    def set_kernel(self, variant: int) -> None:
        """Which kernel this context's digest launches run (fs_ctx_set_kernel):

          0  KERNEL_AUTO      chosen from what the launches report (the default)
          2  KERNEL_MIXED     the mixed-length kernel: long frames of mixed tiles go in pieces
          3  KERNEL_SEGMENTS  the segment kernel: a tile's frames cut into equal chunks
          4  KERNEL_ONE_PASS  the one-pass kernel: block-aligned rows
          8  KERNEL_SMALL     the small-frame kernel (one lane per frame) preferred

        Any other value raises. include/framesum.h has the rules of the automatic choice, of
        variant 8 and of the host-staged calls; DESIGN.md §3.14 the segment kernel's cost."""
        self._check(self.lib.fs_ctx_set_kernel(self._ctx, int(variant)), "fs_ctx_set_kernel")

    def set_workgroups(self, workgroups: int) -> None:
        """fs_ctx_set_workgroups: 0 (default) one 16-wave workgroup per CU; k > 0 at most k
        workgroups per launch, each wave then streams several tiles back to back."""
        self._check(self.lib.fs_ctx_set_workgroups(self._ctx, int(workgroups)), "fs_ctx_set_workgroups")

    def last_kernel(self) -> int:
        """The variant (2, 3, 4 or 8, as set_kernel lists them) this context's latest launch ran;
        0 before its first launch. include/framesum.h (fs_ctx_last_kernel) says which one the
        automatic choice starts with and when it moves."""
        v = self.lib.fs_ctx_last_kernel(self._ctx)
        if v < 0:
            self._check(v, "fs_ctx_last_kernel")
        return int(v)

    # ---- device-resident path (torch tensors as device memory) -------------
    def _resident_args(self, frames, offsets, lengths, mtu, extra, out, status, stream):
        """The checked C arguments of a device-resident call over a batch: (ctx, frames, offsets,
        lengths, n, mtu, *extra, out, status, stream). This is every digest call's path, so the
        tensor pointers go as plain integers and the function's prototype converts them. Returns (args, out,
        status, stream) with the results allocated and the stream chosen where None came in."""
        import torch

        n = int(lengths.numel())
        assert frames.is_cuda and offsets.is_cuda and lengths.is_cuda, "device-resident path needs CUDA tensors"
        assert frames.dtype == torch.uint8 and offsets.dtype == torch.int64 and lengths.dtype == torch.int32
        assert offsets.numel() == n and frames.is_contiguous() and offsets.is_contiguous() and lengths.is_contiguous()
        if out is None or status is None:  # (a caller with result slots of its own skips the call)
            out, status = _result_tensors(n, frames.device, out, status)
        if stream is None:
            stream = torch.cuda.current_stream(frames.device)
        args = (self._ctx, frames.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n, mtu, *extra,
                out.data_ptr(), status.data_ptr(), stream.cuda_stream)
        return args, out, status, stream

    def _resident(self, name, frames, offsets, lengths, mtu, extra, out, status, stream):
        args, out, status, _ = self._resident_args(frames, offsets, lengths, mtu, extra, out, status, stream)
        st = getattr(self.lib, name)(*args)
        if st:
            self._check(st, name)
        return out, status

    def digest_device(self, frames, offsets, lengths, mtu: int = 0, out=None, status=None, stream=None):
        """Device-resident batch digest.

        frames: uint8 CUDA tensor; offsets: int64 CUDA tensor; lengths: int32
        CUDA tensor. Returns (out, status): out is an int32 tensor of shape
        (n, 2) holding the raw fs_digest words ([:,0] = crc32 bits,
        [:,1] = ip_csum | l4_csum << 16), status a uint8 tensor. Asynchronous
        on `stream` (default: torch's current stream).
        """
        return self._resident("fs_digest_batch", frames, offsets, lengths, mtu, (), out, status, stream)

    def fill_device(self, frames, offsets, lengths, mtu: int = 0, flags: int = FILL_CSUM, out=None, status=None,
                    stream=None):
        """TX fill IN PLACE on the device tensor `frames` (fs_fill_batch): FILL_CSUM writes the
        IPv4 and TCP/UDP checksums into every frame RecvEth would checksum, FCS_APPEND the
        CRC-32 after each frame (4 spare bytes needed there). Returns (out, status) as
        digest_device would report them for the written frames."""
        return self._resident("fs_fill_batch", frames, offsets, lengths, mtu, (flags,), out, status, stream)

    def digest_fcs_device(self, frames, offsets, lengths, mtu: int = 0, out=None, status=None, stream=None):
        """RX digest of wire frames with a trailing FCS (fs_digest_batch_fcs): lengths include
        the FCS; status FS_ERR_FCS (14) where it is missing or wrong."""
        return self._resident("fs_digest_batch_fcs", frames, offsets, lengths, mtu, (), out, status, stream)

    def prepare_digest(self, frames, offsets, lengths, mtu: int = 0, out=None, status=None, stream=None, op="digest",
                       flags: int = FILL_CSUM):
        """A prepared digest_device call: the tensors are checked and the C arguments built ONCE,
        and the returned callable enqueues the same fs_digest_batch (op "fcs": fs_digest_batch_fcs;
        op "fill": fs_fill_batch with `flags`) again on every call, with no per-call validation or
        marshalling. For a caller that digests a fixed set of resident batches into fixed result
        slots over and over (a NIC ring's buffers, the bench's rotated batches): the per-call host
        cost is the C call alone. The callable keeps the tensors alive and raises FramesumError on
        a failed call."""
        name = {"digest": "fs_digest_batch", "fcs": "fs_digest_batch_fcs", "fill": "fs_fill_batch"}[op]
        extra = (flags,) if op == "fill" else ()
        args, out, status, stream = self._resident_args(frames, offsets, lengths, mtu, extra, out, status, stream)
        fn = self.lib[name]  # a fresh function pointer with no argtypes: the ctypes objects go as built here
        args = tuple(a if isinstance(a, _vp) else ctype(a) for ctype, a in zip(PROTOTYPES[name][1], args))
        keep = (frames, offsets, lengths, out, status, stream)

        def call():
            if self._ctx is None:  # (the context was closed: its pointer in `args` is gone)
                raise FramesumError(f"{name}: the engine was closed")
            st = fn(*args)
            if st:
                self._check(st, name)
            return keep[3], keep[4]

        return call

    def deinterleave_device(self, gathered, nshards: int, n: int, out=None, status=None, stream=None):
        """Global frame order from nshards gathered round-robin slabs (fs_deinterleave):
        `gathered` is a uint8 CUDA tensor of nshards * shard_slab_bytes(n, nshards) bytes, slab k =
        shard k's digests then its verdicts. Returns (out (n, 2) int32, status (n,) uint8)."""
        import torch

        assert gathered.is_cuda and gathered.dtype == torch.uint8 and gathered.is_contiguous()
        assert gathered.numel() >= nshards * shard_slab_bytes(n, nshards)
        out, status = _result_tensors(n, gathered.device, out, status)
        if stream is None:
            stream = torch.cuda.current_stream(gathered.device)
        st = self.lib.fs_deinterleave(self._ctx, _tensor_ptr(gathered), nshards, n, _tensor_ptr(out),
                                      _tensor_ptr(status), _stream_ptr(stream))
        self._check(st, "fs_deinterleave")
        return out, status

    # ---- TX frame build -----------------------------------------------------
    def segment_device(self, sends: np.ndarray, payload, mtu: int = 0, flags: int = 0, align: int = 4, stream=None,
                       frames=None):
        """Build the frames of `sends` (a SEND_DTYPE array on the host) from the uint8 CUDA tensor
        `payload` (fs_segment_batch): TCP sends are cut into mss-sized segments, UDP sends make one
        frame, headers, both checksums and (flags FCS_APPEND) the FCS are written in one pass.
        `frames`: a uint8 CUDA tensor to build into (at least segment_layout's bytes; bytes between
        frames are left as they are), else a new one. Returns (frames, offsets int64, lengths int32,
        out (n, 2) int32, status uint8) device tensors; asynchronous on `stream`."""
        import torch

        sends = np.ascontiguousarray(sends, dtype=SEND_DTYPE)
        n_frames, nbytes = segment_layout(sends, flags, align)
        dev = payload.device
        assert payload.is_cuda and payload.dtype == torch.uint8 and payload.is_contiguous()
        if frames is None:
            frames = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous()
        offsets = torch.empty((n_frames,), dtype=torch.int64, device=dev)
        lengths = torch.empty((n_frames,), dtype=torch.int32, device=dev)
        out, status = _result_tensors(n_frames, dev, None, None)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        st = self.lib.fs_segment_batch(
            self._ctx, _array_ptr(sends), int(sends.size), _tensor_ptr(payload), int(payload.numel()), mtu, flags,
            align, _tensor_ptr(frames), int(frames.numel()), _tensor_ptr(offsets), _tensor_ptr(lengths),
            _tensor_ptr(out), _tensor_ptr(status), _stream_ptr(stream))
        self._check(st, "fs_segment_batch")
        return frames, offsets, lengths, out, status

    def segment_host(self, sends: np.ndarray, payload: np.ndarray, mtu: int = 0, flags: int = 0, align: int = 4,
                     frames: Optional[np.ndarray] = None):
        """segment_device from and to host memory (fs_segment_batch_host). `frames`: a writable uint8
        array to build into (pinned from host_empty, or pageable), else a new zeroed one. Returns
        (frames, offsets uint64, lengths uint32, digests, status) numpy arrays."""
        sends = np.ascontiguousarray(sends, dtype=SEND_DTYPE)
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        n_frames, nbytes = segment_layout(sends, flags, align)
        if frames is None:
            frames = np.zeros(nbytes, dtype=np.uint8)
        assert frames.dtype == np.uint8 and frames.flags["C_CONTIGUOUS"] and frames.flags["WRITEABLE"]
        offsets = np.zeros(n_frames, dtype=np.uint64)
        lengths = np.zeros(n_frames, dtype=np.uint32)
        out = np.zeros(n_frames, dtype=DIGEST_DTYPE)
        status = np.zeros(n_frames, dtype=np.uint8)
        st = self.lib.fs_segment_batch_host(
            self._ctx, _array_ptr(sends), int(sends.size), _array_ptr(payload), payload.nbytes, mtu, flags, align,
            _array_ptr(frames), frames.nbytes, _array_ptr(offsets), _array_ptr(lengths), _array_ptr(out),
            _array_ptr(status))
        self._check(st, "fs_segment_batch_host")
        return frames, offsets, lengths, out, status

    def segment_batch(self, headers: Sequence[bytes], payloads: Sequence[bytes], mss: int,
                      append_fcs: bool = False) -> list[list[bytes]]:
        """The reference's TX frame build for many sends (stacks/port_tcp.go:162-194 CalculateHeaders +
        PutHeaders + the payload cut of TCPConn.send): headers[i] is a 54-byte Ethernet + IPv4 + TCP
        template (or 42 bytes for UDP, which makes one frame whatever `mss`), payloads[i] its send data.
        Returns, per send, its finished frames (each with its FCS when `append_fcs`)."""
        assert len(headers) == len(payloads)
        sends = np.zeros(len(headers), dtype=SEND_DTYPE)
        at = 0
        for i, (h, p) in enumerate(zip(headers, payloads)):
            assert len(h) in (42, 54), "a header template is 54 bytes (TCP) or 42 bytes (UDP)"
            sends["hdr"][i, : len(h)] = np.frombuffer(bytes(h), dtype=np.uint8)
            sends["mss"][i] = 0 if len(h) == 42 else mss
            sends["payload_off"][i] = at
            sends["payload_len"][i] = len(p)
            at += len(p)
        if len(sends) == 0:
            return []
        flags = FCS_APPEND if append_fcs else 0
        payload = np.frombuffer(b"".join(bytes(p) for p in payloads) + b"\0", dtype=np.uint8)
        frames, off, ln, _, _ = self.segment_host(sends, payload[:at], 0, flags, 1)
        room = 4 if append_fcs else 0
        res, f = [], 0
        for s in sends:
            cnt = send_frames(int(s["mss"]), int(s["payload_len"]))
            res.append([bytes(frames[int(off[j]) : int(off[j]) + int(ln[j]) + room]) for j in range(f, f + cnt)])
            f += cnt
        return res

    # ---- RX coalesce (plain: _RX, flow-aware: _RX_FLOWS) ----------------------
    def _rx_device(self, rx, frames, offsets, lengths, mtu, flags, payload, stream, socks=()):
        """(payload, runs, *the call's further record tensors, run_of, totals, out, status). `socks`:
        the delivery call's arguments between `flags` and `payload`; only that call takes `payload`
        False (no packed copy: a null pointer and a cap of 0, and None comes back)."""
        import torch

        name, totals_dtype, between = rx
        n, dev = int(lengths.numel()), frames.device
        out, status = _result_tensors(n, dev, None, None)
        if payload is None:
            payload = torch.empty((frames.numel(),), dtype=torch.uint8, device=dev)
        if payload is False:
            payload_args = (None, 0)
        else:
            assert payload.is_cuda and payload.dtype == torch.uint8 and payload.is_contiguous()
            payload_args = (_tensor_ptr(payload), payload.numel())
        # a record array is (n, record bytes) uint8, a uint32 array int32 (-1 = NO_RUN)
        records = [torch.empty((n, d.itemsize), dtype=torch.uint8, device=dev) if d.fields else
                   torch.empty((n,), dtype=torch.int32, device=dev)
                   for d in (RUN_DTYPE, *(d for d, _ in between), np.dtype(np.uint32))]
        totals = torch.empty((totals_dtype.itemsize,), dtype=torch.uint8, device=dev)
        extra = (flags, *socks, *payload_args, *map(_tensor_ptr, records), _tensor_ptr(totals))
        self._resident(name, frames, offsets, lengths, mtu, extra, out, status, stream)
        return (None if payload is False else payload, *records, totals, out, status)

    def _rx_host(self, rx, frames, offsets, lengths, mtu, flags, payload, socks=()):
        """_rx_device's tuple as numpy arrays, each record array cut to its written entries and the
        totals as one scalar record."""
        name, totals_dtype, between = rx
        frames, offsets, lengths, n = _host_batch(frames, offsets, lengths)
        if payload is None:
            payload = np.zeros(int(lengths.sum(dtype=np.uint64)), dtype=np.uint8)
        if payload is False:
            payload_args = (None, 0)
        else:
            assert payload.dtype == np.uint8 and payload.flags["C_CONTIGUOUS"] and payload.flags["WRITEABLE"]
            payload_args = (_array_ptr(payload), payload.nbytes)
        runs, *more, run_of = [np.zeros(n, dtype=d) for d in (RUN_DTYPE, *(d for d, _ in between), np.uint32)]
        totals = np.zeros(1, dtype=totals_dtype)
        out = np.zeros(n, dtype=DIGEST_DTYPE)
        status = np.zeros(n, dtype=np.uint8)
        st = getattr(self.lib, name + "_host")(
            self._ctx, *_host_head(frames, offsets, lengths, n), mtu, flags, *socks, *payload_args,
            *map(_array_ptr, (runs, *more, run_of, totals, out, status)))
        self._check(st, name + "_host")
        t = totals[0]
        return (None if payload is False else payload, runs[: int(t["n_runs"])],
                *(a[: int(t[count])] for a, (_, count) in zip(more, between)),
                run_of, t, out, status)

    def coalesce_device(self, frames, offsets, lengths, mtu: int = 0, flags: int = 0, payload=None, stream=None):
        """Verify a device-resident batch and gather the payload of every accepted frame
        (fs_coalesce_batch): `payload` (a uint8 CUDA tensor, else a new one of the frame buffer's
        size) receives the payloads back to back; frames that would end past it are not copied.
        Returns (payload, runs, run_of, totals, out, status) device tensors: runs (n, 24) uint8 =
        RUN_DTYPE records of which the first totals' n_runs are written, run_of (n,) int32 (-1 =
        NO_RUN), totals (16,) uint8 = one TOTALS_DTYPE record; out and status as digest_device gives
        them (flags RX_FCS: as digest_fcs_device). Asynchronous on `stream`; split_runs() brings the
        runs and totals to the host."""
        return self._rx_device(_RX, frames, offsets, lengths, mtu, flags, payload, stream)

    def coalesce_host(self, frames: np.ndarray, offsets: np.ndarray, lengths: np.ndarray, mtu: int = 0, flags: int = 0,
                      payload: Optional[np.ndarray] = None):
        """coalesce_device from and to host memory (fs_coalesce_batch_host). `payload`: a writable
        uint8 array to gather into, else a new zeroed one as long as the frames together. Returns
        (payload, runs RUN_DTYPE[n_runs], run_of uint32, totals TOTALS_DTYPE scalar record, digests,
        status) numpy arrays."""
        return self._rx_host(_RX, frames, offsets, lengths, mtu, flags, payload)

    def coalesce_batch(self, frames: Sequence[bytes], mtu: int = 0) -> list:
        """The reference's RX delivery for many frames (the payload slices of stacks/portstack.go:217,
        :239, :301-303 and the in-order append of TCPConn.recv, stacks/tcpconn.go:347-369): one
        (first_frame, n_frames, tcp_flags, payload_bytes) per run of the accepted frames, TCP segments
        that continue each other delivered as one run."""
        if len(frames) == 0:
            return []
        buf, offsets, lengths = pack_frames(frames, 1)
        payload, runs, _, _, _, _ = self.coalesce_host(buf, offsets, lengths, mtu)
        return [(int(r["first_frame"]), int(r["n_frames"]), int(r["tcp_flags"]),
                 bytes(payload[int(r["payload_off"]) : int(r["payload_off"]) + int(r["payload_len"])])) for r in runs]

    def coalesce_flows_device(self, frames, offsets, lengths, mtu: int = 0, flags: int = 0, payload=None, stream=None):
        """coalesce_device for batches in which the segments of several flows interleave
        (fs_coalesce_flows_batch): the accepted frames are grouped by flow (protocol, addresses,
        ports), `payload` receives each flow's payload contiguously, flows in the order of their
        first frames, and the runs are found inside each flow. Returns (payload, runs, flows, order,
        run_of, totals, out, status) device tensors: runs (n, 24) uint8 = RUN_DTYPE records whose
        first_frame indexes `order`, flows (n, 32) uint8 = FLOW_DTYPE records, order (n,) int32 of
        which the first n_accepted are written (the batch indices in delivery order), run_of (n,)
        int32, totals (24,) uint8 = one FLOW_TOTALS_DTYPE record. Asynchronous on `stream`;
        split_flows() brings the records to the host."""
        return self._rx_device(_RX_FLOWS, frames, offsets, lengths, mtu, flags, payload, stream)

    def coalesce_flows_host(self, frames: np.ndarray, offsets: np.ndarray, lengths: np.ndarray, mtu: int = 0,
                            flags: int = 0, payload: Optional[np.ndarray] = None):
        """coalesce_flows_device from and to host memory (fs_coalesce_flows_batch_host). Returns
        (payload, runs RUN_DTYPE[n_runs], flows FLOW_DTYPE[n_flows], order uint32[n_accepted], run_of
        uint32, totals FLOW_TOTALS_DTYPE scalar record, digests, status) numpy arrays."""
        return self._rx_host(_RX_FLOWS, frames, offsets, lengths, mtu, flags, payload)

    def coalesce_flows_batch(self, frames: Sequence[bytes], mtu: int = 0) -> list:
        """The reference's RX demultiplexing and delivery for many frames (findPort,
        stacks/portstack.go:309 and :246; TCPConn.recv, stacks/tcpconn.go:347-369): per flow, in the
        order of the flows' first frames, (proto, src, dst, sport, dport, [(tcp_flags, payload_bytes)
        per run]) with src and dst the 4 address bytes."""
        if len(frames) == 0:
            return []
        buf, offsets, lengths = pack_frames(frames, 1)
        payload, runs, flows, order, _, _, _, _ = self.coalesce_flows_host(buf, offsets, lengths, mtu)
        res = []
        for fl in flows:
            f = frames[int(order[int(fl["first_frame"])])]
            l4 = 14 + 4 * (f[14] & 15)
            rs = runs[int(fl["first_run"]) : int(fl["first_run"]) + int(fl["n_runs"])]
            res.append((f[23], bytes(f[26:30]), bytes(f[30:34]), int.from_bytes(f[l4 : l4 + 2], "big"),
                        int.from_bytes(f[l4 + 2 : l4 + 4], "big"),
                        [(int(r["tcp_flags"]),
                          bytes(payload[int(r["payload_off"]) : int(r["payload_off"]) + int(r["payload_len"])])) for r in rs]))
        return res

    # ---- in-order TCP delivery into socket rings (include/framesum_deliver.h) ----
    def deliver_flows_device(self, frames, offsets, lengths, socks: np.ndarray, rings, mtu: int = 0, flags: int = 0,
                             payload=None, delivered: bool = True, stream=None):
        """coalesce_flows_device plus the delivery of every flow that belongs to a listed socket
        (fs_deliver_flows_batch): `socks` is a SOCK_DTYPE array on the host (key from sock_key(), the
        receive state, and where in `rings` the socket's ring lies); `rings` a uint8 CUDA tensor. The
        flow's data segments are admitted in order (Seq == rcv_nxt, inside the window, no ACK of
        unsent data, room in the ring) and their bytes go from the frames into the ring, wrapping at
        its end. `payload` False: no packed copy. Returns (socks_out, delivered, payload, runs, flows,
        order, run_of, totals, out, status) device tensors: socks_out (n_socks, 32) uint8 =
        SOCK_OUT_DTYPE records, delivered (n,) uint8 (1 admitted, 2 considered and not admitted, 0
        otherwise; None when `delivered` is False), the rest as coalesce_flows_device gives them.
        Asynchronous on `stream`; split_socks() brings socks_out to the host."""
        import torch

        socks = np.ascontiguousarray(socks, dtype=SOCK_DTYPE)
        n, dev = int(lengths.numel()), frames.device
        assert rings.is_cuda and rings.dtype == torch.uint8 and rings.is_contiguous()
        socks_out = torch.empty((int(socks.size), SOCK_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        marks = torch.empty((n,), dtype=torch.uint8, device=dev) if delivered else None
        args = (_array_ptr(socks), int(socks.size), _tensor_ptr(rings), rings.numel(), _tensor_ptr(socks_out),
                _tensor_ptr(marks) if delivered else None)
        return (socks_out, marks, *self._rx_device(_RX_DELIVER, frames, offsets, lengths, mtu, flags, payload, stream, args))

    def deliver_flows_host(self, frames: np.ndarray, offsets: np.ndarray, lengths: np.ndarray, socks: np.ndarray,
                           rings: np.ndarray, mtu: int = 0, flags: int = 0, payload=None, delivered: bool = True):
        """deliver_flows_device from and to host memory (fs_deliver_flows_batch_host): `rings` is a
        writable uint8 array, written in place inside the listed rings only. Returns (socks_out
        SOCK_OUT_DTYPE[n_socks], delivered uint8[n] or None, then coalesce_flows_host's tuple)."""
        socks = np.ascontiguousarray(socks, dtype=SOCK_DTYPE)
        assert isinstance(rings, np.ndarray) and rings.dtype == np.uint8 and rings.flags["C_CONTIGUOUS"]
        assert rings.flags["WRITEABLE"], "deliver_flows_host writes into `rings`"
        socks_out = np.zeros(int(socks.size), dtype=SOCK_OUT_DTYPE)
        marks = np.zeros(int(np.asarray(lengths).size), dtype=np.uint8) if delivered else None
        args = (_array_ptr(socks), int(socks.size), _array_ptr(rings), rings.nbytes, _array_ptr(socks_out),
                _array_ptr(marks) if delivered else None)
        return (socks_out, marks, *self._rx_host(_RX_DELIVER, frames, offsets, lengths, mtu, flags, payload, args))

    # ---- the receive call: the delivery plus each socket's ACKs and windows (include/framesum_recv.h) ----
    def recv_flows_device(self, frames, offsets, lengths, socks: np.ndarray, snd: np.ndarray, rings, mtu: int = 0,
                          flags: int = 0, payload=None, delivered: bool = True, code: bool = True, stream=None):
        """deliver_flows_device plus, for every listed socket, what ControlBlock.Recv does to the send
        side of an Established connection for each frame of its flow (fs_recv_flows_batch): `snd` is a
        SND_DTYPE array on the host, parallel to `socks` (snd.UNA and snd.WND before the batch). Returns
        (snd_out, code, then deliver_flows_device's tuple) device tensors: snd_out (n_socks, 32) uint8 =
        SND_OUT_DTYPE records (snd.UNA and snd.WND after the batch, the counts per code, RECV_ACK_OWED |
        RECV_FIN), code (n,) uint8 (RECV_TAKEN .. RECV_RING_FULL for the frames of a listed socket's
        flow before its stop, RECV_NONE otherwise; None when `code` is False). Asynchronous on `stream`;
        split_snd() brings snd_out to the host."""
        import torch

        socks = np.ascontiguousarray(socks, dtype=SOCK_DTYPE)
        snd = np.ascontiguousarray(snd, dtype=SND_DTYPE)
        assert snd.size == socks.size, "one send-side record per socket"
        n, dev = int(lengths.numel()), frames.device
        assert rings.is_cuda and rings.dtype == torch.uint8 and rings.is_contiguous()
        socks_out = torch.empty((int(socks.size), SOCK_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        snd_out = torch.empty((int(socks.size), SND_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        marks = torch.empty((n,), dtype=torch.uint8, device=dev) if delivered else None
        codes = torch.empty((n,), dtype=torch.uint8, device=dev) if code else None
        args = (_array_ptr(socks), int(socks.size), _tensor_ptr(rings), rings.numel(), _tensor_ptr(socks_out),
                _tensor_ptr(marks) if delivered else None, _array_ptr(snd), _tensor_ptr(snd_out),
                _tensor_ptr(codes) if code else None)
        return (snd_out, codes, socks_out, marks,
                *self._rx_device(_RX_RECV, frames, offsets, lengths, mtu, flags, payload, stream, args))

    def recv_flows_host(self, frames: np.ndarray, offsets: np.ndarray, lengths: np.ndarray, socks: np.ndarray,
                        snd: np.ndarray, rings: np.ndarray, mtu: int = 0, flags: int = 0, payload=None,
                        delivered: bool = True, code: bool = True):
        """recv_flows_device from and to host memory (fs_recv_flows_batch_host). Returns (snd_out
        SND_OUT_DTYPE[n_socks], code uint8[n] or None, then deliver_flows_host's tuple)."""
        socks = np.ascontiguousarray(socks, dtype=SOCK_DTYPE)
        snd = np.ascontiguousarray(snd, dtype=SND_DTYPE)
        assert snd.size == socks.size, "one send-side record per socket"
        assert isinstance(rings, np.ndarray) and rings.dtype == np.uint8 and rings.flags["C_CONTIGUOUS"]
        assert rings.flags["WRITEABLE"], "recv_flows_host writes into `rings`"
        n = int(np.asarray(lengths).size)
        socks_out = np.zeros(int(socks.size), dtype=SOCK_OUT_DTYPE)
        snd_out = np.zeros(int(socks.size), dtype=SND_OUT_DTYPE)
        marks = np.zeros(n, dtype=np.uint8) if delivered else None
        codes = np.zeros(n, dtype=np.uint8) if code else None
        args = (_array_ptr(socks), int(socks.size), _array_ptr(rings), rings.nbytes, _array_ptr(socks_out),
                _array_ptr(marks) if delivered else None, _array_ptr(snd), _array_ptr(snd_out),
                _array_ptr(codes) if code else None)
        return (snd_out, codes, socks_out, marks,
                *self._rx_host(_RX_RECV, frames, offsets, lengths, mtu, flags, payload, args))

    # ---- the accept call: the receive call plus the passive open (include/framesum_accept.h) ----
    def accept_flows_device(self, frames, offsets, lengths, socks: np.ndarray, snd: np.ndarray, rings,
                            listeners: np.ndarray, slots: np.ndarray, mtu: int = 0, flags: int = 0, synack_flags: int = 0,
                            payload=None, delivered: bool = True, code: bool = True, accept_of: bool = True,
                            synacks=None, synack_results: bool = True, stream=None, _closing=None):
        """recv_flows_device plus the passive open of every flow without a listed socket whose first
        frame is a SYN to a listener (fs_accept_flows_batch): `listeners` is a LISTENER_DTYPE array on the
        host (local address and port in wire order, the SYN-ACKs' source MAC, the listener's range of
        `slots`), `slots` an ACCEPT_SLOT_DTYPE array on the host (iss, rcv_wnd and the IPv4 ID seed of each
        free connection). A listener's candidates take its slots in ascending order of flow number.
        `synacks`: a uint8 CUDA tensor of n_slots * ACCEPT_STRIDE bytes (else a new zeroed one), of which
        only the 54 (58 with synack_flags FCS_APPEND) frame bytes of filled slots are written. Returns
        (conns, listeners_out, accept_of, synacks, synack_out, synack_status, then recv_flows_device's
        tuple) device tensors: conns (n_slots, 48) uint8 = ACCEPT_CONN_DTYPE records, listeners_out
        (n_listeners, 16) uint8 = LISTENER_OUT_DTYPE records, accept_of (n,) int32 per flow (the slot,
        -2 = ACCEPT_FULL, -1 = ACCEPT_NONE; None when `accept_of` is False), synack_out (n_slots, 2) int32
        and synack_status (n_slots,) uint8 as digest_device gives them, written for filled slots only
        (zeroed here first; None when `synack_results` is False; the caller's own pair of tensors when it
        is a tuple, whose other entries keep their values). Asynchronous on `stream`; split_accept()
        brings the records to the host."""
        import torch

        socks = np.ascontiguousarray(socks, dtype=SOCK_DTYPE)
        snd = np.ascontiguousarray(snd, dtype=SND_DTYPE)
        listeners = np.ascontiguousarray(listeners, dtype=LISTENER_DTYPE)
        slots = np.ascontiguousarray(slots, dtype=ACCEPT_SLOT_DTYPE)
        assert snd.size == socks.size, "one send-side record per socket"
        n, dev = int(lengths.numel()), frames.device
        n_slots, n_listeners = int(slots.size), int(listeners.size)
        assert rings.is_cuda and rings.dtype == torch.uint8 and rings.is_contiguous()
        if synacks is None:
            synacks = torch.zeros((n_slots * ACCEPT_STRIDE,), dtype=torch.uint8, device=dev)
        assert synacks.is_cuda and synacks.dtype == torch.uint8 and synacks.is_contiguous()
        assert synacks.numel() >= n_slots * ACCEPT_STRIDE, "synacks holds ACCEPT_STRIDE bytes per slot"
        socks_out = torch.empty((int(socks.size), SOCK_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        snd_out = torch.empty((int(socks.size), SND_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        marks = torch.empty((n,), dtype=torch.uint8, device=dev) if delivered else None
        codes = torch.empty((n,), dtype=torch.uint8, device=dev) if code else None
        conns = torch.empty((n_slots, ACCEPT_CONN_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        listeners_out = torch.empty((n_listeners, LISTENER_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        of = torch.empty((n,), dtype=torch.int32, device=dev) if accept_of else None
        if isinstance(synack_results, tuple):  # the caller's own (n_slots, 2) int32 and (n_slots,) uint8 tensors
            syn_out, syn_st = synack_results
            assert syn_out.is_cuda and syn_out.dtype == torch.int32 and syn_out.numel() == 2 * n_slots
            assert syn_st.is_cuda and syn_st.dtype == torch.uint8 and syn_st.numel() == n_slots
        else:
            syn_out = torch.zeros((n_slots, 2), dtype=torch.int32, device=dev) if synack_results else None
            syn_st = torch.zeros((n_slots,), dtype=torch.uint8, device=dev) if synack_results else None

        def ptr(t):
            return _tensor_ptr(t) if t is not None and t.numel() else None

        args = (_array_ptr(socks), int(socks.size), _tensor_ptr(rings), rings.numel(), _tensor_ptr(socks_out),
                ptr(marks), _array_ptr(snd), _tensor_ptr(snd_out), ptr(codes),
                _array_ptr(listeners), n_listeners, _array_ptr(slots), n_slots, synack_flags, ptr(conns), ptr(listeners_out),
                ptr(of), ptr(synacks), ptr(syn_out), ptr(syn_st))
        rx, mine = _RX_ACCEPT, ()
        if _closing is not None:  # close_flows_device: the closing arguments behind synack_status, its tensors in front
            closers, ctl = _closing[:2]
            closers_out = torch.empty((int(closers.size), CLOSE_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            socks_close = torch.empty((int(socks.size), CLOSE_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            ctl_code = torch.empty((n,), dtype=torch.uint8, device=dev) if ctl else None
            args += (_array_ptr(closers), int(closers.size), ptr(closers_out), ptr(socks_close), ptr(ctl_code))
            rx, mine = _RX_CLOSE, (closers_out, socks_close, ctl_code)
            if len(_closing) > 2:  # connect_flows_device: the opening arguments behind ctl_code, its tensors in front
                openers, reply_flags, replies, reply_results = _closing[2]
                n_open = int(openers.size)
                if replies is None:
                    replies = torch.zeros((n_open * ACCEPT_STRIDE,), dtype=torch.uint8, device=dev)
                assert replies.is_cuda and replies.dtype == torch.uint8 and replies.is_contiguous()
                assert replies.numel() >= n_open * ACCEPT_STRIDE, "replies holds ACCEPT_STRIDE bytes per opener"
                openers_out = torch.empty((n_open, CONNECT_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
                rep_out = torch.zeros((n_open, 2), dtype=torch.int32, device=dev) if reply_results else None
                rep_st = torch.zeros((n_open,), dtype=torch.uint8, device=dev) if reply_results else None
                args += (_array_ptr(openers), n_open, reply_flags, ptr(openers_out), ptr(replies), ptr(rep_out), ptr(rep_st))
                rx, mine = _RX_CONNECT, (openers_out, replies, rep_out, rep_st, *mine)
                if len(_closing) > 3:  # udp_flows_device: the port arguments behind reply_status, its tensors in front
                    ports, cells, want_port_of, want_cell_of = _closing[3]
                    assert cells.is_cuda and cells.dtype == torch.uint8 and cells.is_contiguous()
                    ports_out = torch.empty((int(ports.size), UDP_PORT_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
                    port_of = torch.empty((n,), dtype=torch.int32, device=dev) if want_port_of else None
                    cell_of = torch.empty((n,), dtype=torch.int32, device=dev) if want_cell_of else None
                    args += (_array_ptr(ports), int(ports.size), ptr(cells), cells.numel(), ptr(ports_out), ptr(port_of),
                             ptr(cell_of))
                    rx, mine = _RX_UDP, (ports_out, port_of, cell_of, *mine)
                    if len(_closing) > 4:  # arp_flows_device: the host and query arguments behind cell_of, its tensors in front
                        hosts, queries, n_reply, arp_flags, arp_frames, arp_results, want_code, want_of = _closing[4]
                        n_frames = n_reply + int(queries.size)
                        if arp_frames is None:
                            arp_frames = torch.zeros((n_frames * ACCEPT_STRIDE,), dtype=torch.uint8, device=dev)
                        assert arp_frames.is_cuda and arp_frames.dtype == torch.uint8 and arp_frames.is_contiguous()
                        assert arp_frames.numel() >= n_frames * ACCEPT_STRIDE, "arp_frames holds ACCEPT_STRIDE bytes per slot"
                        hosts_out = torch.empty((int(hosts.size), ARP_HOST_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
                        queries_out = torch.empty((int(queries.size), ARP_QUERY_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
                        if isinstance(arp_results, tuple):  # the caller's own (slots, 2) int32 and (slots,) uint8 tensors
                            arp_out, arp_st = arp_results
                            assert arp_out.is_cuda and arp_out.dtype == torch.int32 and arp_out.numel() == 2 * n_frames
                            assert arp_st.is_cuda and arp_st.dtype == torch.uint8 and arp_st.numel() == n_frames
                        else:
                            arp_out = torch.zeros((n_frames, 2), dtype=torch.int32, device=dev) if arp_results else None
                            arp_st = torch.zeros((n_frames,), dtype=torch.uint8, device=dev) if arp_results else None
                        arp_code = torch.empty((n,), dtype=torch.uint8, device=dev) if want_code else None
                        arp_of = torch.empty((n,), dtype=torch.int32, device=dev) if want_of else None
                        args += (_array_ptr(hosts), int(hosts.size), _array_ptr(queries), int(queries.size), n_reply, arp_flags,
                                 ptr(hosts_out), ptr(queries_out), ptr(arp_frames), ptr(arp_out), ptr(arp_st), ptr(arp_code),
                                 ptr(arp_of))
                        rx, mine = _RX_ARP, (hosts_out, queries_out, arp_frames, arp_out, arp_st, arp_code, arp_of, *mine)
        return (*mine, conns, listeners_out, of, synacks, syn_out, syn_st, snd_out, codes, socks_out, marks,
                *self._rx_device(rx, frames, offsets, lengths, mtu, flags, payload, stream, args))

    def accept_flows_host(self, frames: np.ndarray, offsets: np.ndarray, lengths: np.ndarray, socks: np.ndarray,
                          snd: np.ndarray, rings: np.ndarray, listeners: np.ndarray, slots: np.ndarray, mtu: int = 0,
                          flags: int = 0, synack_flags: int = 0, payload=None, delivered: bool = True, code: bool = True,
                          accept_of: bool = True, synacks=None, synack_results: bool = True, _closing=None):
        """accept_flows_device from and to host memory (fs_accept_flows_batch_host). `synacks`: a
        writable uint8 array of n_slots * ACCEPT_STRIDE bytes (else a new zeroed one), written in place in
        the frame bytes of filled slots only. Returns (conns ACCEPT_CONN_DTYPE[n_slots], listeners_out
        LISTENER_OUT_DTYPE[n_listeners], accept_of uint32[n] or None, synacks, synack_out
        DIGEST_DTYPE[n_slots] or None, synack_status uint8[n_slots] or None, then recv_flows_host's
        tuple)."""
        socks = np.ascontiguousarray(socks, dtype=SOCK_DTYPE)
        snd = np.ascontiguousarray(snd, dtype=SND_DTYPE)
        listeners = np.ascontiguousarray(listeners, dtype=LISTENER_DTYPE)
        slots = np.ascontiguousarray(slots, dtype=ACCEPT_SLOT_DTYPE)
        assert snd.size == socks.size, "one send-side record per socket"
        assert isinstance(rings, np.ndarray) and rings.dtype == np.uint8 and rings.flags["C_CONTIGUOUS"]
        assert rings.flags["WRITEABLE"], "accept_flows_host writes into `rings`"
        n = int(np.asarray(lengths).size)
        n_slots, n_listeners = int(slots.size), int(listeners.size)
        if synacks is None:
            synacks = np.zeros(n_slots * ACCEPT_STRIDE, dtype=np.uint8)
        assert isinstance(synacks, np.ndarray) and synacks.dtype == np.uint8 and synacks.flags["C_CONTIGUOUS"]
        assert synacks.flags["WRITEABLE"] and synacks.size >= n_slots * ACCEPT_STRIDE
        socks_out = np.zeros(int(socks.size), dtype=SOCK_OUT_DTYPE)
        snd_out = np.zeros(int(socks.size), dtype=SND_OUT_DTYPE)
        marks = np.zeros(n, dtype=np.uint8) if delivered else None
        codes = np.zeros(n, dtype=np.uint8) if code else None
        conns = np.zeros(n_slots, dtype=ACCEPT_CONN_DTYPE)
        listeners_out = np.zeros(n_listeners, dtype=LISTENER_OUT_DTYPE)
        of = np.full(n, ACCEPT_NONE, dtype=np.uint32) if accept_of else None
        if isinstance(synack_results, tuple):  # the caller's own DIGEST_DTYPE[n_slots] and uint8[n_slots] arrays
            syn_out, syn_st = synack_results
            assert syn_out.dtype == DIGEST_DTYPE and syn_out.size == n_slots and syn_out.flags["C_CONTIGUOUS"]
            assert syn_st.dtype == np.uint8 and syn_st.size == n_slots and syn_st.flags["C_CONTIGUOUS"]
        else:
            syn_out = np.zeros(n_slots, dtype=DIGEST_DTYPE) if synack_results else None
            syn_st = np.zeros(n_slots, dtype=np.uint8) if synack_results else None

        def ptr(a):
            return _array_ptr(a) if a is not None and a.size else None

        args = (_array_ptr(socks), int(socks.size), _array_ptr(rings), rings.nbytes, _array_ptr(socks_out),
                ptr(marks), _array_ptr(snd), _array_ptr(snd_out), ptr(codes),
                _array_ptr(listeners), n_listeners, _array_ptr(slots), n_slots, synack_flags, ptr(conns), ptr(listeners_out),
                ptr(of), ptr(synacks), ptr(syn_out), ptr(syn_st))
        rx, mine = _RX_ACCEPT, ()
        if _closing is not None:  # close_flows_host
            closers, ctl = _closing[:2]
            closers_out = np.zeros(int(closers.size), dtype=CLOSE_OUT_DTYPE)
            socks_close = np.zeros(int(socks.size), dtype=CLOSE_OUT_DTYPE)
            ctl_code = np.zeros(n, dtype=np.uint8) if ctl else None
            args += (_array_ptr(closers), int(closers.size), ptr(closers_out), ptr(socks_close), ptr(ctl_code))
            rx, mine = _RX_CLOSE, (closers_out, socks_close, ctl_code)
            if len(_closing) > 2:  # connect_flows_host
                openers, reply_flags, replies, reply_results = _closing[2]
                n_open = int(openers.size)
                if replies is None:
                    replies = np.zeros(n_open * ACCEPT_STRIDE, dtype=np.uint8)
                assert isinstance(replies, np.ndarray) and replies.dtype == np.uint8 and replies.flags["C_CONTIGUOUS"]
                assert replies.flags["WRITEABLE"] and replies.size >= n_open * ACCEPT_STRIDE
                openers_out = np.zeros(n_open, dtype=CONNECT_OUT_DTYPE)
                rep_out = np.zeros(n_open, dtype=DIGEST_DTYPE) if reply_results else None
                rep_st = np.zeros(n_open, dtype=np.uint8) if reply_results else None
                args += (_array_ptr(openers), n_open, reply_flags, ptr(openers_out), ptr(replies), ptr(rep_out), ptr(rep_st))
                rx, mine = _RX_CONNECT, (openers_out, replies, rep_out, rep_st, *mine)
                if len(_closing) > 3:  # udp_flows_host
                    ports, cells, want_port_of, want_cell_of = _closing[3]
                    assert isinstance(cells, np.ndarray) and cells.dtype == np.uint8 and cells.flags["C_CONTIGUOUS"]
                    assert cells.flags["WRITEABLE"], "udp_flows_host writes into `cells`"
                    ports_out = np.zeros(int(ports.size), dtype=UDP_PORT_OUT_DTYPE)
                    port_of = np.full(n, UDP_NONE, dtype=np.uint32) if want_port_of else None
                    cell_of = np.full(n, UDP_NONE, dtype=np.uint32) if want_cell_of else None
                    args += (_array_ptr(ports), int(ports.size), ptr(cells), cells.nbytes, ptr(ports_out), ptr(port_of),
                             ptr(cell_of))
                    rx, mine = _RX_UDP, (ports_out, port_of, cell_of, *mine)
                    if len(_closing) > 4:  # arp_flows_host
                        hosts, queries, n_reply, arp_flags, arp_frames, arp_results, want_code, want_of = _closing[4]
                        n_frames = n_reply + int(queries.size)
                        if arp_frames is None:
                            arp_frames = np.zeros(n_frames * ACCEPT_STRIDE, dtype=np.uint8)
                        assert isinstance(arp_frames, np.ndarray) and arp_frames.dtype == np.uint8
                        assert arp_frames.flags["C_CONTIGUOUS"] and arp_frames.flags["WRITEABLE"]
                        assert arp_frames.size >= n_frames * ACCEPT_STRIDE, "arp_frames holds ACCEPT_STRIDE bytes per slot"
                        hosts_out = np.zeros(int(hosts.size), dtype=ARP_HOST_OUT_DTYPE)
                        queries_out = np.zeros(int(queries.size), dtype=ARP_QUERY_OUT_DTYPE)
                        if isinstance(arp_results, tuple):  # the caller's own DIGEST_DTYPE[slots] and uint8[slots] arrays
                            arp_out, arp_st = arp_results
                            assert arp_out.dtype == DIGEST_DTYPE and arp_out.size == n_frames and arp_out.flags["C_CONTIGUOUS"]
                            assert arp_st.dtype == np.uint8 and arp_st.size == n_frames and arp_st.flags["C_CONTIGUOUS"]
                        else:
                            arp_out = np.zeros(n_frames, dtype=DIGEST_DTYPE) if arp_results else None
                            arp_st = np.zeros(n_frames, dtype=np.uint8) if arp_results else None
                        arp_code = np.zeros(n, dtype=np.uint8) if want_code else None
                        arp_of = np.full(n, ARP_NONE, dtype=np.uint32) if want_of else None
                        args += (_array_ptr(hosts), int(hosts.size), _array_ptr(queries), int(queries.size), n_reply, arp_flags,
                                 ptr(hosts_out), ptr(queries_out), ptr(arp_frames), ptr(arp_out), ptr(arp_st), ptr(arp_code),
                                 ptr(arp_of))
                        rx, mine = _RX_ARP, (hosts_out, queries_out, arp_frames, arp_out, arp_st, arp_code, arp_of, *mine)
        return (*mine, conns, listeners_out, of, synacks, syn_out, syn_st, snd_out, codes, socks_out, marks,
                *self._rx_host(rx, frames, offsets, lengths, mtu, flags, payload, args))

    # ---- the close call: the accept call plus the closing states and the RST (include/framesum_close.h) ----
    def close_flows_device(self, frames, offsets, lengths, socks: np.ndarray, snd: np.ndarray, rings,
                           listeners: np.ndarray, slots: np.ndarray, closers: np.ndarray, ctl_code: bool = True, **kw):
        """accept_flows_device plus the receive side of the closing states and of an RST
        (fs_close_flows_batch): `closers` is a CLOSER_DTYPE array on the host, the sockets whose
        ControlBlock is in ST_FIN_WAIT_1 .. ST_LAST_ACK (key, state, rcv_nxt, rcv_wnd, snd_una, snd_nxt,
        snd_wnd; a closer has no ring). Every closer's flow is walked under the rule of the header, and
        every socket of `socks` goes on from where the receive call's walk ended at an admitted FIN or
        at an RST. Further keyword arguments are accept_flows_device's. Returns (closers_out,
        socks_close, ctl_code, then accept_flows_device's tuple) device tensors: closers_out (n_closers,
        32) and socks_close (n_socks, 32) uint8 = CLOSE_OUT_DTYPE records (the state, rcv.NXT, snd.UNA and
        snd.WND behind the walk, the counts, the walk's stop, CLOSE_ACK_OWED | CLOSE_FIN | CLOSE_RESET),
        ctl_code (n,) uint8 (CLOSE_TAKEN .. CLOSE_EXPECTED for the frames a control walk handled,
        CLOSE_NONE otherwise; None when `ctl_code` is False). Asynchronous on `stream`; split_close()
        brings the records to the host."""
        closers = np.ascontiguousarray(closers, dtype=CLOSER_DTYPE)
        return self.accept_flows_device(frames, offsets, lengths, socks, snd, rings, listeners, slots,
                                        _closing=(closers, ctl_code), **kw)

    def close_flows_host(self, frames: np.ndarray, offsets: np.ndarray, lengths: np.ndarray, socks: np.ndarray,
                         snd: np.ndarray, rings: np.ndarray, listeners: np.ndarray, slots: np.ndarray,
                         closers: np.ndarray, ctl_code: bool = True, **kw):
        """close_flows_device from and to host memory (fs_close_flows_batch_host). Returns (closers_out
        CLOSE_OUT_DTYPE[n_closers], socks_close CLOSE_OUT_DTYPE[n_socks], ctl_code uint8[n] or None, then
        accept_flows_host's tuple)."""
        closers = np.ascontiguousarray(closers, dtype=CLOSER_DTYPE)
        return self.accept_flows_host(frames, offsets, lengths, socks, snd, rings, listeners, slots,
                                      _closing=(closers, ctl_code), **kw)

    # ---- the connect call: the close call plus the active open (include/framesum_connect.h) ----
    def connect_flows_device(self, frames, offsets, lengths, socks: np.ndarray, snd: np.ndarray, rings,
                             listeners: np.ndarray, slots: np.ndarray, closers: np.ndarray, openers: np.ndarray,
                             reply_flags: int = 0, replies=None, reply_results: bool = True, ctl_code: bool = True, **kw):
        """close_flows_device plus the receive side of SynSent (fs_connect_flows_batch): `openers` is an
        OPENER_DTYPE array on the host, the connections that have sent or are about to send their SYN (key,
        CN_SEND_SYN or 0, the two MACs, iss, rcv_wnd, the IPv4 ID seed). Every opener's flow is walked under
        the rule of the header, and the control frame the opener owes is built. `replies`: a uint8 CUDA
        tensor of n_openers * ACCEPT_STRIDE bytes (else a new zeroed one), of which only the 54 (58 with
        reply_flags FCS_APPEND) frame bytes of openers with a reply are written. Further keyword arguments
        are accept_flows_device's. Returns (openers_out, replies, reply_out, reply_status, then
        close_flows_device's tuple) device tensors: openers_out (n_openers, 48) uint8 = CONNECT_OUT_DTYPE
        records, reply_out (n_openers, 2) int32 and reply_status (n_openers,) uint8 as digest_device gives
        them, written for openers with a reply only (zeroed here first; None when `reply_results` is
        False). Asynchronous on `stream`; split_connect() brings the records to the host."""
        closers = np.ascontiguousarray(closers, dtype=CLOSER_DTYPE)
        openers = np.ascontiguousarray(openers, dtype=OPENER_DTYPE)
        return self.accept_flows_device(frames, offsets, lengths, socks, snd, rings, listeners, slots,
                                        _closing=(closers, ctl_code, (openers, reply_flags, replies, reply_results)), **kw)

    def connect_flows_host(self, frames: np.ndarray, offsets: np.ndarray, lengths: np.ndarray, socks: np.ndarray,
                           snd: np.ndarray, rings: np.ndarray, listeners: np.ndarray, slots: np.ndarray,
                           closers: np.ndarray, openers: np.ndarray, reply_flags: int = 0, replies=None,
                           reply_results: bool = True, ctl_code: bool = True, **kw):
        """connect_flows_device from and to host memory (fs_connect_flows_batch_host). `replies`: a writable
        uint8 array of n_openers * ACCEPT_STRIDE bytes (else a new zeroed one), written in place. Returns
        (openers_out CONNECT_OUT_DTYPE[n_openers], replies, reply_out DIGEST_DTYPE[n_openers] or None,
        reply_status uint8[n_openers] or None, then close_flows_host's tuple)."""
        closers = np.ascontiguousarray(closers, dtype=CLOSER_DTYPE)
        openers = np.ascontiguousarray(openers, dtype=OPENER_DTYPE)
        return self.accept_flows_host(frames, offsets, lengths, socks, snd, rings, listeners, slots,
                                      _closing=(closers, ctl_code, (openers, reply_flags, replies, reply_results)), **kw)

    # ---- the UDP call: the connect call plus the datagrams' delivery into port queues (include/framesum_udp.h) ----
    def udp_flows_device(self, frames, offsets, lengths, socks: np.ndarray, snd: np.ndarray, rings,
                         listeners: np.ndarray, slots: np.ndarray, closers: np.ndarray, openers: np.ndarray,
                         ports: np.ndarray, cells, port_of: bool = True, cell_of: bool = True, reply_flags: int = 0,
                         replies=None, reply_results: bool = True, ctl_code: bool = True, **kw):
        """connect_flows_device plus the UDP half of RecvEth (fs_udp_flows_batch): `ports` is a UDP_PORT_DTYPE
        array on the host (udp_port() makes one row), `cells` the uint8 CUDA tensor the ports' queues lie in.
        Every accepted UDP frame whose destination a port lists goes to the port's next free cell, in batch
        order: a 32-byte UDP_CELL_DTYPE header, then the payload, cut to the cell's room. Further keyword
        arguments are accept_flows_device's. Returns (ports_out, port_of, cell_of, then connect_flows_device's
        tuple) device tensors: ports_out (n_ports, 32) uint8 = UDP_PORT_OUT_DTYPE records, port_of and cell_of
        (n,) int32 (-1 = UDP_NONE, -2 = UDP_FULL; None when the flag is False). Asynchronous on `stream`;
        split_dgrams() brings the datagrams to the host."""
        closers = np.ascontiguousarray(closers, dtype=CLOSER_DTYPE)
        openers = np.ascontiguousarray(openers, dtype=OPENER_DTYPE)
        ports = np.ascontiguousarray(ports, dtype=UDP_PORT_DTYPE)
        return self.accept_flows_device(frames, offsets, lengths, socks, snd, rings, listeners, slots,
                                        _closing=(closers, ctl_code, (openers, reply_flags, replies, reply_results),
                                                  (ports, cells, port_of, cell_of)), **kw)

    def udp_flows_host(self, frames: np.ndarray, offsets: np.ndarray, lengths: np.ndarray, socks: np.ndarray,
                       snd: np.ndarray, rings: np.ndarray, listeners: np.ndarray, slots: np.ndarray, closers: np.ndarray,
                       openers: np.ndarray, ports: np.ndarray, cells: np.ndarray, port_of: bool = True, cell_of: bool = True,
                       reply_flags: int = 0, replies=None, reply_results: bool = True, ctl_code: bool = True, **kw):
        """udp_flows_device from and to host memory (fs_udp_flows_batch_host). `cells`: a writable uint8
        array, written in place in the cells that take a datagram. Returns (ports_out
        UDP_PORT_OUT_DTYPE[n_ports], port_of uint32[n] or None, cell_of uint32[n] or None, then
        connect_flows_host's tuple)."""
        closers = np.ascontiguousarray(closers, dtype=CLOSER_DTYPE)
        openers = np.ascontiguousarray(openers, dtype=OPENER_DTYPE)
        ports = np.ascontiguousarray(ports, dtype=UDP_PORT_DTYPE)
        return self.accept_flows_host(frames, offsets, lengths, socks, snd, rings, listeners, slots,
                                      _closing=(closers, ctl_code, (openers, reply_flags, replies, reply_results),
                                                (ports, cells, port_of, cell_of)), **kw)

    # ---- the ARP call: the UDP call plus the ARP branch of RecvEth (include/framesum_arp.h) ----
    def arp_flows_device(self, frames, offsets, lengths, socks: np.ndarray, snd: np.ndarray, rings,
                         listeners: np.ndarray, slots: np.ndarray, closers: np.ndarray, openers: np.ndarray,
                         ports: np.ndarray, cells, hosts: np.ndarray, queries: np.ndarray, n_reply_slots: int = None,
                         arp_flags: int = 0, arp_frames=None, arp_results=True, arp_code: bool = True, arp_of: bool = True,
                         port_of: bool = True, cell_of: bool = True, reply_flags: int = 0, replies=None,
                         reply_results: bool = True, ctl_code: bool = True, **kw):
        """udp_flows_device plus the ARP branch of RecvEth (fs_arp_flows_batch): `hosts` is an ARP_HOST_DTYPE
        array on the host (arp_host() makes one row: a local interface, its range of reply slots), `queries`
        an ARP_QUERY_DTYPE array on the host (arp_query(): a resolution in progress, or with ARP_SEND_REQUEST
        one whose who-has frame is to be built). Every ARP request for a host's address is answered in the
        host's next free slot, in batch order; every ARP reply resolves the query it matches. `n_reply_slots`:
        the reply slots in `arp_frames` (the end of the hosts' ranges unless given); query q's request goes to
        slot n_reply_slots + q. `arp_frames`: a uint8 CUDA tensor of ACCEPT_STRIDE bytes per slot (else a new
        zeroed one), of which only the built frames' bytes are written. Further keyword arguments are
        accept_flows_device's. Returns (hosts_out, queries_out, arp_frames, arp_out, arp_status, arp_code, arp_of,
        then udp_flows_device's tuple) device tensors: hosts_out (n_hosts, 16) and queries_out (n_queries, 16)
        uint8 = ARP_HOST_OUT_DTYPE / ARP_QUERY_OUT_DTYPE records, arp_out (slots, 2) int32 and arp_status
        (slots,) uint8 as digest_device gives them, written for built frames only (zeroed here first; None when
        `arp_results` is False; the caller's own pair when it is a tuple), arp_code (n,) uint8 and arp_of (n,)
        int32 (-1 = ARP_NONE; None when the flag is False). Asynchronous on `stream`; split_arp() brings
        the results to the host."""
        closers = np.ascontiguousarray(closers, dtype=CLOSER_DTYPE)
        openers = np.ascontiguousarray(openers, dtype=OPENER_DTYPE)
        ports = np.ascontiguousarray(ports, dtype=UDP_PORT_DTYPE)
        hosts = np.ascontiguousarray(hosts, dtype=ARP_HOST_DTYPE)
        queries = np.ascontiguousarray(queries, dtype=ARP_QUERY_DTYPE)
        if n_reply_slots is None:
            n_reply_slots = arp_reply_slots(hosts)
        return self.accept_flows_device(frames, offsets, lengths, socks, snd, rings, listeners, slots,
                                        _closing=(closers, ctl_code, (openers, reply_flags, replies, reply_results),
                                                  (ports, cells, port_of, cell_of),
                                                  (hosts, queries, int(n_reply_slots), arp_flags, arp_frames, arp_results,
                                                   arp_code, arp_of)), **kw)

    def arp_flows_host(self, frames: np.ndarray, offsets: np.ndarray, lengths: np.ndarray, socks: np.ndarray,
                       snd: np.ndarray, rings: np.ndarray, listeners: np.ndarray, slots: np.ndarray, closers: np.ndarray,
                       openers: np.ndarray, ports: np.ndarray, cells: np.ndarray, hosts: np.ndarray, queries: np.ndarray,
                       n_reply_slots: int = None, arp_flags: int = 0, arp_frames=None, arp_results=True,
                       arp_code: bool = True, arp_of: bool = True, port_of: bool = True, cell_of: bool = True,
                       reply_flags: int = 0, replies=None, reply_results: bool = True, ctl_code: bool = True, **kw):
        """arp_flows_device from and to host memory (fs_arp_flows_batch_host). `arp_frames`: a writable uint8
        array of ACCEPT_STRIDE bytes per slot (else a new zeroed one), written in place in the built frames'
        bytes only. Returns (hosts_out ARP_HOST_OUT_DTYPE[n_hosts], queries_out ARP_QUERY_OUT_DTYPE[n_queries],
        arp_frames, arp_out DIGEST_DTYPE[slots] or None, arp_status uint8[slots] or None, arp_code uint8[n] or
        None, arp_of uint32[n] or None, then udp_flows_host's tuple)."""
        closers = np.ascontiguousarray(closers, dtype=CLOSER_DTYPE)
        openers = np.ascontiguousarray(openers, dtype=OPENER_DTYPE)
        ports = np.ascontiguousarray(ports, dtype=UDP_PORT_DTYPE)
        hosts = np.ascontiguousarray(hosts, dtype=ARP_HOST_DTYPE)
        queries = np.ascontiguousarray(queries, dtype=ARP_QUERY_DTYPE)
        if n_reply_slots is None:
            n_reply_slots = arp_reply_slots(hosts)
        return self.accept_flows_host(frames, offsets, lengths, socks, snd, rings, listeners, slots,
                                      _closing=(closers, ctl_code, (openers, reply_flags, replies, reply_results),
                                                (ports, cells, port_of, cell_of),
                                                (hosts, queries, int(n_reply_slots), arp_flags, arp_frames, arp_results,
                                                 arp_code, arp_of)), **kw)

    # ---- TCP segments from socket TX rings (include/framesum_send.h) ------------
    @staticmethod
    def send_rings_layout(socks: np.ndarray, flags: int = 0, align: int = 1):
        """(n_frames, frames_bytes, socks_out) of a batch of sockets (fs_send_rings_layout): host-only
        arithmetic, see the module's send_rings_layout."""
        return send_rings_layout(socks, flags, align)

    def _send_rings(self, host: bool, socks, rings, mtu, flags, align, frames, stream):
        """The one path of send_rings_device and send_rings_host: the layout, the frame buffer and
        the four arrays (tensors on rings' device, or numpy arrays), and the call."""
        socks = np.ascontiguousarray(socks, dtype=TX_SOCK_DTYPE)
        n_frames, nbytes, _ = send_rings_layout(socks, flags, align)
        socks_out = np.zeros(int(socks.size), dtype=TX_SOCK_OUT_DTYPE)
        if host:
            rings = np.ascontiguousarray(rings, dtype=np.uint8)
            if frames is None:
                frames = np.zeros(nbytes, dtype=np.uint8)
            assert isinstance(frames, np.ndarray) and frames.dtype == np.uint8 and frames.flags["C_CONTIGUOUS"]
            assert frames.flags["WRITEABLE"], "send_rings_host writes into `frames`"
            arrays = [np.zeros(n_frames, dtype=d) for d in (np.uint64, np.uint32, DIGEST_DTYPE, np.uint8)]
            ptr, size, tail = _array_ptr, (lambda a: a.nbytes), ()
        else:
            import torch

            dev = rings.device
            assert rings.is_cuda and rings.dtype == torch.uint8 and rings.is_contiguous()
            if frames is None:
                frames = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            assert frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous()
            arrays = [torch.empty((n_frames,), dtype=torch.int64, device=dev),
                      torch.empty((n_frames,), dtype=torch.int32, device=dev), *_result_tensors(n_frames, dev, None, None)]
            if stream is None:
                stream = torch.cuda.current_stream(dev)
            ptr, size, tail = _tensor_ptr, (lambda t: int(t.numel())), (_stream_ptr(stream),)
        name = "fs_send_rings_batch_host" if host else "fs_send_rings_batch"
        st = getattr(self.lib, name)(self._ctx, _array_ptr(socks), int(socks.size), ptr(rings), size(rings), mtu, flags, align,
                                     ptr(frames), size(frames), *map(ptr, arrays), _array_ptr(socks_out), *tail)
        self._check(st, name)
        return (frames, *arrays, socks_out)

    def send_rings_device(self, socks: np.ndarray, rings, mtu: int = 0, flags: int = 0, align: int = 1, stream=None,
                          frames=None):
        """Build the TCP segments of `socks` (a TX_SOCK_DTYPE array on the host: header template,
        mss, where in `rings` the socket's TX ring lies, its read position and buffered bytes, and
        the connection state) straight from the uint8 CUDA tensor `rings` (fs_send_rings_batch): per
        socket min(buffered, window room, max_frames * mss) bytes go out in mss-sized frames whose
        payload is read across the ring's end, with Seq = snd_nxt + k mss, Ack = rcv_nxt, Window =
        rcv_wnd, the TX_* flags, both checksums and (flags FCS_APPEND) the FCS. `frames`: a uint8
        CUDA tensor to build into, else a new one. Returns (frames, offsets int64, lengths int32,
        out (n, 2) int32, status uint8) device tensors and socks_out, a TX_SOCK_OUT_DTYPE numpy
        array that is complete when the call returns; the rest is asynchronous on `stream`."""
        return self._send_rings(False, socks, rings, mtu, flags, align, frames, stream)

    def send_rings_host(self, socks: np.ndarray, rings: np.ndarray, mtu: int = 0, flags: int = 0, align: int = 1,
                        frames: Optional[np.ndarray] = None):
        """send_rings_device from and to host memory (fs_send_rings_batch_host). `frames`: a writable
        uint8 array to build into, else a new zeroed one. Returns (frames, offsets uint64, lengths
        uint32, digests, status, socks_out) numpy arrays."""
        return self._send_rings(True, socks, rings, mtu, flags, align, frames, None)

    # ---- the ring send from device-resident sockets (include/framesum_send_resident.h) ----
    def send_rings_resident(self, socks, rings, frames_cap: int, frames=None, frames_bytes: Optional[int] = None,
                            rx_socks_out=None, rx_snd_out=None, rx_index=None, writeback: bool = False, mtu: int = 0,
                            flags: int = 0, align: int = 1, stream=None, offsets=None, lengths=None, out=None, status=None,
                            socks_out=None, totals=None):
        """The ring send with its socket table on the device (fs_send_rings_resident). `socks`: an (n, 104)
        uint8 CUDA tensor of TX_SOCK_DTYPE records (tx_socks_tensor makes one), only read unless
        `writeback` (TX_WRITEBACK), which writes every built socket's state after the call back into it.
        `rx_socks_out`, `rx_snd_out`: the socks_out and snd_out tensors of an RX call (recv_flows_device, ...)
        passed straight in: rcv_nxt, rcv_wnd, snd_una, snd_wnd and the owed ACK are taken from them on the
        device, socket i from record rx_index[i] (an int32 / uint32 tensor; TX_NO_RX: none) or i. The
        checks, the rule and the layout run in kernels: an invalid socket is reported in its record
        (TX_INVALID | reason << 16), and sockets whose frames no longer fit `frames_cap` frames or
        `frames_bytes` bytes (default: all of `frames`) are TX_DEFERRED: call again for them. `frames`: a
        uint8 CUDA tensor to build into (required unless frames_bytes is given: then a new one of that
        size). offsets, lengths, out, status: False leaves one out, None makes a new tensor of frames_cap
        entries. Returns (frames, offsets int64, lengths int32, out (n, 2) int32, status uint8, socks_out
        (n, 32) uint8, totals (40,) uint8) device tensors; split_tx brings the last two to the host.
        Asynchronous on `stream`: nothing is read back."""
        import torch

        dev = rings.device
        assert socks.is_cuda and socks.dtype == torch.uint8 and socks.is_contiguous() and socks.dim() == 2 and \
            socks.shape[1] == TX_SOCK_DTYPE.itemsize, "socks is an (n, 104) uint8 CUDA tensor"
        assert rings.is_cuda and rings.dtype == torch.uint8 and rings.is_contiguous()
        n = int(socks.shape[0])
        if frames is None:
            assert frames_bytes is not None, "pass `frames`, or frames_bytes for a new buffer"
            frames = torch.empty((int(frames_bytes),), dtype=torch.uint8, device=dev)
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous()
        if frames_bytes is None:
            frames_bytes = int(frames.numel())
        assert frames_bytes <= int(frames.numel())
        cap = int(frames_cap)
        made = {"offsets": lambda: torch.empty((cap,), dtype=torch.int64, device=dev),
                "lengths": lambda: torch.empty((cap,), dtype=torch.int32, device=dev),
                "out": lambda: torch.empty((cap, 2), dtype=torch.int32, device=dev),
                "status": lambda: torch.empty((cap,), dtype=torch.uint8, device=dev)}
        arrays = []
        for name, given in (("offsets", offsets), ("lengths", lengths), ("out", out), ("status", status)):
            t = made[name]() if given is None else (None if given is False else given)
            assert t is None or (t.is_cuda and t.is_contiguous() and t.shape[0] >= cap), name
            arrays.append(t)
        if socks_out is None:
            socks_out = torch.empty((n, TX_SOCK_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        if totals is None:
            totals = torch.empty((TX_TOTALS_DTYPE.itemsize,), dtype=torch.uint8, device=dev)
        assert socks_out.is_cuda and socks_out.is_contiguous() and socks_out.numel() * socks_out.element_size() >= 32 * n
        assert totals.is_cuda and totals.is_contiguous() and totals.numel() * totals.element_size() >= 40
        n_rx = 0
        for t in (rx_socks_out, rx_snd_out, rx_index):
            assert t is None or (t.is_cuda and t.is_contiguous())
        if rx_socks_out is not None:
            n_rx = int(rx_socks_out.numel() * rx_socks_out.element_size()) // SOCK_OUT_DTYPE.itemsize
            assert rx_snd_out is None or rx_snd_out.numel() * rx_snd_out.element_size() >= n_rx * SND_OUT_DTYPE.itemsize
        if rx_index is not None:
            assert rx_index.element_size() == 4 and rx_index.numel() >= n
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        opt = lambda t: None if t is None else _tensor_ptr(t)  # noqa: E731
        st = self.lib.fs_send_rings_resident(
            self._ctx, _tensor_ptr(socks), n, opt(rx_socks_out), opt(rx_snd_out), opt(rx_index), n_rx, _tensor_ptr(rings),
            int(rings.numel()), mtu, flags | (TX_WRITEBACK if writeback else 0), align, _tensor_ptr(frames), frames_bytes, cap,
            *map(opt, arrays), _tensor_ptr(socks_out), _tensor_ptr(totals), _stream_ptr(stream))
        self._check(st, "fs_send_rings_resident")
        return (frames, *arrays, socks_out, totals)

    # ---- host-staged path (numpy in, numpy out) -----------------------------
    def host_empty(self, shape, dtype=np.uint8) -> np.ndarray:
        """A numpy array in pinned host memory (fs_host_alloc), freed with the array."""
        import weakref

        dtype = np.dtype(dtype)
        nbytes = max(1, int(np.prod(shape)) * dtype.itemsize)
        ptr = _vp()
        self._check(self.lib.fs_host_alloc(self._ctx, _u64(nbytes), ctypes.byref(ptr)), "fs_host_alloc")
        raw = (ctypes.c_uint8 * nbytes).from_address(ptr.value)
        arr = np.frombuffer(raw, dtype=np.uint8, count=nbytes)[: int(np.prod(shape)) * dtype.itemsize]
        arr = arr.view(dtype).reshape(shape)
        # freed when the array goes away, or by close() (arrays must not outlive the engine)
        self._pinned.add(ptr.value)
        weakref.finalize(raw, Engine._free_pinned, weakref.ref(self), ptr.value)
        return arr

    @staticmethod
    def _free_pinned(engine_ref, addr: int) -> None:
        eng = engine_ref()
        if eng is not None and getattr(eng, "_ctx", None) and addr in eng._pinned:
            eng._pinned.discard(addr)
            eng.lib.fs_host_free(eng._ctx, _vp(addr))

    def digest_host(self, frames: np.ndarray, offsets: np.ndarray, lengths: np.ndarray, mtu: int = 0,
                    out: Optional[np.ndarray] = None, status: Optional[np.ndarray] = None):
        """Host buffers in, host results out (fs_digest_batch_host): chunked H2D / kernel / D2H
        pipeline over the context's streams. Returns (digests, status)."""
        frames, offsets, lengths, n = _host_batch(frames, offsets, lengths)
        if out is None:
            out = np.zeros(n, dtype=DIGEST_DTYPE)
        if status is None:
            status = np.zeros(n, dtype=np.uint8)
        assert out.dtype == DIGEST_DTYPE and out.size >= n and status.dtype == np.uint8 and status.size >= n
        assert out.flags["C_CONTIGUOUS"] and status.flags["C_CONTIGUOUS"], "out / status are written in place"
        if n == 0:
            return out, status
        st = self.lib.fs_digest_batch_host(self._ctx, *_host_head(frames, offsets, lengths, n), mtu, _array_ptr(out),
                                           _array_ptr(status))
        self._check(st, "fs_digest_batch_host")
        return out, status

    def fill_host(self, frames: np.ndarray, offsets: np.ndarray, lengths: np.ndarray, mtu: int = 0,
                  flags: int = FILL_CSUM):
        """TX fill IN PLACE on a writable host uint8 array (fs_fill_batch_host). Returns
        (digests, status) of the frames as written."""
        frames, offsets, lengths, n = _host_batch(frames, offsets, lengths, writable=True)
        out = np.zeros(n, dtype=DIGEST_DTYPE)
        status = np.zeros(n, dtype=np.uint8)
        if n == 0:
            return out, status
        st = self.lib.fs_fill_batch_host(self._ctx, *_host_head(frames, offsets, lengths, n), mtu, flags,
                                         _array_ptr(out), _array_ptr(status))
        self._check(st, "fs_fill_batch_host")
        return out, status

    # ---- reference-shaped surface -------------------------------------------
    def digest_batch(self, frames: Sequence[bytes], mtu: int = 0) -> list[Digest]:
        """Batched equivalent of RecvEth's checksum work for each frame (host lists)."""
        buf, offsets, lengths = pack_frames(frames)
        dig, st = self.digest_host(buf, offsets, lengths, mtu)
        return [Digest(int(d["crc32"]), int(d["ip_csum"]), int(d["l4_csum"]), int(s)) for d, s in zip(dig, st)]

    def recv_eth_batch(self, frames: Sequence[bytes], mtu: int = 0) -> list[Optional[str]]:
        """Per-frame RecvEth error class (None = checksum OK), like RecvEth's return."""
        return [d.err for d in self.digest_batch(frames, mtu)]

    def calculate_headers_batch(self, frames: Sequence[bytes], mtu: int = 0, append_fcs: bool = False) -> list[bytes]:
        """The checksum part of the reference's TX header calculation (stacks/port_tcp.go:178,
        :193; dhcp_client.go:479, :486) for many frames: each frame with its IPv4 and TCP/UDP
        checksum fields filled (frames RecvEth would not checksum come back unchanged), and
        with its FCS appended when `append_fcs`."""
        room = 4 if append_fcs else 0
        buf, offsets, lengths = pack_frames([bytes(f) + bytes(room) for f in frames])
        lengths = lengths - np.uint32(room)
        self.fill_host(buf, offsets, lengths, mtu, FILL_CSUM | (FCS_APPEND if append_fcs else 0))
        return [bytes(buf[int(o) : int(o) + int(l) + room]) for o, l in zip(offsets, lengths)]


def digest_host_multi(engines: Sequence["Engine"], frames: np.ndarray, offsets: np.ndarray, lengths: np.ndarray,
                      mtu: int = 0):
    """Host buffers in, host results out, over several contexts at once (fs_digest_batch_multi):
    contiguous byte-balanced blocks of frames, one per engine (one per GPU), each on its own
    host thread and H2D / kernel / D2H pipeline. Returns (digests, status) in batch order."""
    assert len(engines) > 0 and len({id(e) for e in engines}) == len(engines), "engines must be distinct"
    lib = engines[0].lib
    frames, offsets, lengths, n = _host_batch(frames, offsets, lengths)
    out = np.zeros(n, dtype=DIGEST_DTYPE)
    status = np.zeros(n, dtype=np.uint8)
    if n == 0:
        return out, status
    ctxs = (_vp * len(engines))(*[e._ctx for e in engines])
    st = lib.fs_digest_batch_multi(ctxs, len(engines), *_host_head(frames, offsets, lengths, n), mtu, _array_ptr(out),
                                   _array_ptr(status))
    if st != FS_SUCCESS:
        # every entry point clears its context's message first: only failing contexts hold one
        msgs = "; ".join(f"ctx {k}: {m}" for k, e in enumerate(engines)
                         if (m := e.lib.fs_last_error(e._ctx).decode()))
        raise FramesumError(f"fs_digest_batch_multi failed ({st}): {msgs}")
    return out, status


def send_frames(mss: int, payload_len: int) -> int:
    """Frames one send makes: 1 when mss is 0 or the payload is empty, else ceil(payload_len / mss)."""
    return 1 if mss == 0 or payload_len == 0 else -(-payload_len // mss)


def segment_layout(sends: np.ndarray, flags: int = 0, align: int = 4):
    """(n_frames, frames_bytes) a batch of sends (SEND_DTYPE) needs (fs_segment_layout, host-only
    arithmetic: no device is touched). Raises FramesumError for an invalid send, flags or align."""
    sends = np.ascontiguousarray(sends, dtype=SEND_DTYPE)
    lib = load_library()
    n, nbytes = _u64(), _u64()
    st = lib.fs_segment_layout(_array_ptr(sends), int(sends.size), flags, align, ctypes.byref(n), ctypes.byref(nbytes))
    if st != FS_SUCCESS:
        raise FramesumError(f"fs_segment_layout failed ({st}): {lib.fs_last_error(None).decode()}")
    return int(n.value), int(nbytes.value)


def send_rings_layout(socks: np.ndarray, flags: int = 0, align: int = 1):
    """(n_frames, frames_bytes, socks_out) a batch of sockets (TX_SOCK_DTYPE) needs and gives
    (fs_send_rings_layout, host-only arithmetic: no device is touched): socks_out is the
    TX_SOCK_OUT_DTYPE array the batch call writes. Raises FramesumError for an invalid socket, flags
    or align."""
    socks = np.ascontiguousarray(socks, dtype=TX_SOCK_DTYPE)
    lib = load_library()
    n, nbytes = _u64(), _u64()
    socks_out = np.zeros(int(socks.size), dtype=TX_SOCK_OUT_DTYPE)
    st = lib.fs_send_rings_layout(_array_ptr(socks), int(socks.size), flags, align, ctypes.byref(n), ctypes.byref(nbytes),
                                  _array_ptr(socks_out))
    if st != FS_SUCCESS:
        raise FramesumError(f"fs_send_rings_layout failed ({st}): {lib.fs_last_error(None).decode()}")
    return int(n.value), int(nbytes.value), socks_out


def tx_sock_from(sock_out, tx=None, snd_out=None, **fields) -> np.ndarray:
    """TX_SOCK_DTYPE record(s) whose receive side is what a delivery left: rcv_nxt and rcv_wnd (=
    ring_free, the room of the RX ring) come from `sock_out`, the SOCK_OUT_DTYPE record(s) of
    deliver_flows_device / deliver_flows_host. `tx`: the record(s) to start from (the socket's
    template, TX ring and send state), else zeros; `fields` set further fields, e.g. flags=TX_ACK
    for the ACK that answers the delivery. `snd_out`: the SND_OUT_DTYPE record(s) of recv_flows_device
    / recv_flows_host for the same sockets; snd_una and snd_wnd then come from them, and TX_ACK is
    or-ed into flags where RECV_ACK_OWED is set."""
    sock_out = np.atleast_1d(np.asarray(sock_out, dtype=SOCK_OUT_DTYPE))
    res = np.zeros(sock_out.size, dtype=TX_SOCK_DTYPE) if tx is None else \
        np.atleast_1d(np.array(tx, dtype=TX_SOCK_DTYPE, copy=True))
    assert res.size == sock_out.size, "one TX record per delivery record"
    res["rcv_nxt"], res["rcv_wnd"] = sock_out["rcv_nxt"], sock_out["ring_free"]
    for name, value in fields.items():
        res[name] = value
    if snd_out is not None:
        snd_out = np.atleast_1d(np.asarray(snd_out, dtype=SND_OUT_DTYPE))
        assert res.size == snd_out.size, "one TX record per receive record"
        res["snd_una"], res["snd_wnd"] = snd_out["snd_una"], snd_out["snd_wnd"]
        res["flags"] |= np.where(snd_out["flags"] & RECV_ACK_OWED, TX_ACK, 0).astype(np.uint32)
    return res


def tx_socks_tensor(socks: np.ndarray, device):
    """A TX_SOCK_DTYPE array as the (n, 104) uint8 tensor on `device` that send_rings_resident takes."""
    import torch

    socks = np.ascontiguousarray(socks, dtype=TX_SOCK_DTYPE).reshape(-1)
    raw = socks.view(np.uint8).reshape(socks.size, TX_SOCK_DTYPE.itemsize)
    return torch.from_numpy(raw.copy()).to(device)


def split_tx(socks_out, totals, socks=None):
    """The host view of send_rings_resident's `socks_out` and `totals` tensors (this waits for them):
    (TX_SOCK_OUT_DTYPE[n_socks], the TX_TOTALS_DTYPE record), and with `socks` (the table's tensor) the
    TX_SOCK_DTYPE array it holds as a third."""
    res = (_records(socks_out, TX_SOCK_OUT_DTYPE), _records(totals, TX_TOTALS_DTYPE)[0])
    return res if socks is None else (*res, _records(socks, TX_SOCK_DTYPE))


def _records(t, dtype) -> np.ndarray:
    """A device tensor of records (or of uint32 held as int32) as a host array of `dtype`; a host array as it is."""
    if isinstance(t, np.ndarray):
        return np.ascontiguousarray(t).reshape(-1).view(dtype)
    return np.ascontiguousarray(t.cpu().numpy()).reshape(-1).view(dtype)


def split_runs(runs, totals):
    """The host view of coalesce_device's `runs` and `totals` tensors (this waits for them):
    (RUN_DTYPE[n_runs], payload_bytes, n_runs)."""
    t = _records(totals, TOTALS_DTYPE)[0]
    k = int(t["n_runs"])
    return _records(runs[:k], RUN_DTYPE), int(t["payload_bytes"]), k


def split_flows(runs, flows, order, totals):
    """The host view of coalesce_flows_device's `runs`, `flows`, `order` and `totals` tensors (this
    waits for them): (RUN_DTYPE[n_runs], FLOW_DTYPE[n_flows], order uint32[n_accepted], the
    FLOW_TOTALS_DTYPE record)."""
    t = _records(totals, FLOW_TOTALS_DTYPE)[0]
    return (_records(runs[: int(t["n_runs"])], RUN_DTYPE), _records(flows[: int(t["n_flows"])], FLOW_DTYPE),
            _records(order[: int(t["n_accepted"])], np.uint32), t)


def split_socks(socks_out) -> np.ndarray:
    """The host view of deliver_flows_device's `socks_out` tensor (this waits for it): SOCK_OUT_DTYPE[n_socks]."""
    return _records(socks_out, SOCK_OUT_DTYPE)


def split_snd(snd_out) -> np.ndarray:
    """The host view of recv_flows_device's `snd_out` tensor (this waits for it): SND_OUT_DTYPE[n_socks]."""
    return _records(snd_out, SND_OUT_DTYPE)


def split_accept(conns, listeners_out, accept_of=None):
    """The host view of accept_flows_device's `conns`, `listeners_out` and `accept_of` tensors (this waits
    for them): (ACCEPT_CONN_DTYPE[n_slots], LISTENER_OUT_DTYPE[n_listeners], uint32[n] or None)."""
    return (_records(conns, ACCEPT_CONN_DTYPE), _records(listeners_out, LISTENER_OUT_DTYPE),
            None if accept_of is None else _records(accept_of, np.uint32))


def split_close(closers_out, socks_close, ctl_code=None):
    """The host view of close_flows_device's `closers_out`, `socks_close` and `ctl_code` tensors (this waits
    for them): (CLOSE_OUT_DTYPE[n_closers], CLOSE_OUT_DTYPE[n_socks], uint8[n] or None)."""
    return (_records(closers_out, CLOSE_OUT_DTYPE), _records(socks_close, CLOSE_OUT_DTYPE),
            None if ctl_code is None else _records(ctl_code, np.uint8))


def split_connect(openers_out, reply_out=None, reply_status=None):
    """The host view of connect_flows_device's `openers_out`, `reply_out` and `reply_status` tensors (this
    waits for them): (CONNECT_OUT_DTYPE[n_openers], DIGEST_DTYPE[n_openers] or None, uint8[n_openers] or
    None)."""
    return (_records(openers_out, CONNECT_OUT_DTYPE), None if reply_out is None else _records(reply_out, DIGEST_DTYPE),
            None if reply_status is None else _records(reply_status, np.uint8))


def udp_port(local_ip, local_port: int, n_cells: int, cell_size: int, cells_off: int = 0, wcell: int = 0, free=None):
    """One UDP_PORT_DTYPE row: a port that takes the datagrams to `local_ip` (4 bytes, a dotted string or
    an integer; 0.0.0.0: any destination address) and `local_port`, with a queue of `n_cells` cells of
    `cell_size` bytes at `cells_off`. `free`: the cells the consumer has handed back (all of them unless
    given)."""
    row = np.zeros(1, dtype=UDP_PORT_DTYPE)
    row["local"][0] = sock_key(0, 0, local_ip, local_port)[[5, 6, 7, 8, 11, 12]]
    row["n_cells"], row["cell_size"], row["cells_off"], row["wcell"] = n_cells, cell_size, cells_off, wcell
    row["free"] = n_cells if free is None else free
    return row


def split_dgrams(cells, ports, ports_out):
    """The datagrams a UDP call admitted, per port in arrival order: a list (one entry per port) of lists of
    (header, payload) with `header` one UDP_CELL_DTYPE record and `payload` its `stored` bytes. `cells`: the
    call's uint8 tensor or array (a tensor is waited for and brought to the host), `ports` the rows the call
    was given, `ports_out` its records."""
    cells = _records(cells, np.uint8).reshape(-1)
    ports = np.atleast_1d(np.asarray(ports, dtype=UDP_PORT_DTYPE))
    outs = np.atleast_1d(_records(ports_out, UDP_PORT_OUT_DTYPE))
    assert ports.size == outs.size, "one out record per port"
    res = []
    for p, o in zip(ports, outs):
        got = []
        for r in range(int(o["n_admitted"])):
            at = int(p["cells_off"]) + ((int(p["wcell"]) + r) % int(p["n_cells"])) * int(p["cell_size"])
            h = cells[at : at + UDP_CELL_HEADER].view(UDP_CELL_DTYPE)[0]
            got.append((h, bytes(cells[at + UDP_CELL_HEADER : at + UDP_CELL_HEADER + int(h["stored"])])))
        res.append(got)
    return res


def ports_after(ports, ports_out, consumed=None):
    """The port list for the next call: `ports` with the state `ports_out` reports, and `consumed` cells per
    port (one number for all, or an array; every admitted datagram unless given) handed back."""
    nxt = np.atleast_1d(np.asarray(ports, dtype=UDP_PORT_DTYPE)).copy()
    outs = np.atleast_1d(_records(ports_out, UDP_PORT_OUT_DTYPE))
    assert nxt.size == outs.size, "one out record per port"
    nxt["wcell"] = outs["wcell"]
    free = outs["free"].astype(np.uint64) + (np.asarray(consumed, dtype=np.uint64) if consumed is not None
                                             else outs["n_admitted"].astype(np.uint64))
    assert (free <= nxt["n_cells"]).all(), "more cells handed back than the queue has in use"
    nxt["free"] = free
    return nxt


def _ip4(ip) -> np.ndarray:
    """An IPv4 address (4 bytes, a dotted string or an integer) as its 4 wire bytes."""
    return sock_key(0, 0, ip, 1)[5:9].copy()


def _mac6(mac) -> np.ndarray:
    """A MAC address (6 bytes, or a colon-separated string) as its 6 wire bytes."""
    if isinstance(mac, str):
        mac = bytes(int(x, 16) for x in mac.split(":"))
    m = np.frombuffer(bytes(mac), dtype=np.uint8)
    assert m.size == 6, "a MAC address has 6 bytes"
    return m


def arp_host(ip, mac, slot0: int = 0, free: int = 1):
    """One ARP_HOST_DTYPE row: a local interface with address `ip` (4 bytes, a dotted string or an integer) and
    `mac` (6 bytes or aa:bb:cc:dd:ee:ff), which may emit `free` replies in a call, into the reply slots from
    `slot0` on."""
    row = np.zeros(1, dtype=ARP_HOST_DTYPE)
    row["ip"][0], row["mac"][0] = _ip4(ip), _mac6(mac)
    row["slot0"], row["free"] = slot0, free
    return row


def arp_query(host: int, target, send: bool = False):
    """One ARP_QUERY_DTYPE row: host number `host` resolves `target`. With `send` the call builds the who-has
    frame (and the query takes no reply in that call); without, the query waits for its reply."""
    row = np.zeros(1, dtype=ARP_QUERY_DTYPE)
    row["host"], row["target"][0], row["flags"] = host, _ip4(target), ARP_SEND_REQUEST if send else 0
    return row


def arp_reply_slots(hosts) -> int:
    """The reply slots a host list needs: the end of its last range."""
    hosts = np.atleast_1d(np.asarray(hosts, dtype=ARP_HOST_DTYPE))
    return int((hosts["slot0"].astype(np.uint64) + hosts["free"]).max()) if hosts.size else 0


def split_arp(hosts, queries, hosts_out, queries_out, arp_frames, n_reply_slots=None, arp_flags: int = 0):
    """What an ARP call produced, as Python values: (replies, requests, resolutions). `replies`: per host the
    list of its built reply frames (bytes, the FCS included when arp_flags has FCS_APPEND) in the order of the
    requests they answer; `requests`: {query number: who-has frame} of the queries flagged ARP_SEND_REQUEST;
    `resolutions`: {query number: (mac bytes, batch index of the reply)} of the queries that came back done.
    Tensors are waited for and brought to the host."""
    hosts = np.atleast_1d(np.asarray(hosts, dtype=ARP_HOST_DTYPE))
    queries = np.atleast_1d(np.asarray(queries, dtype=ARP_QUERY_DTYPE))
    h_out = np.atleast_1d(_records(hosts_out, ARP_HOST_OUT_DTYPE))
    q_out = np.atleast_1d(_records(queries_out, ARP_QUERY_OUT_DTYPE))
    assert hosts.size == h_out.size and queries.size == q_out.size, "one out record per host and per query"
    buf = _records(arp_frames, np.uint8).reshape(-1)
    if n_reply_slots is None:
        n_reply_slots = arp_reply_slots(hosts)
    size = (ARP_FRAME_PADDED if arp_flags & ARP_PAD else ARP_FRAME) + (4 if arp_flags & FCS_APPEND else 0)

    def frame(slot):
        return bytes(buf[slot * ACCEPT_STRIDE : slot * ACCEPT_STRIDE + size])

    replies = [[frame(int(h["slot0"]) + r) for r in range(int(o["n_answered"]))] for h, o in zip(hosts, h_out)]
    requests = {q: frame(n_reply_slots + q) for q in range(queries.size) if int(q_out[q]["state"]) == ARP_Q_SENT}
    resolutions = {q: (bytes(q_out[q]["mac"]), int(q_out[q]["frame"])) for q in range(queries.size)
                   if int(q_out[q]["state"]) == ARP_Q_DONE}
    return replies, requests, resolutions


def hosts_after(hosts, hosts_out=None, free=None):
    """The host list for the next call: `hosts` with `free` replies each again (one number for all, or an
    array; what each host had before the call unless given -- the caller has sent the built replies)."""
    nxt = np.atleast_1d(np.asarray(hosts, dtype=ARP_HOST_DTYPE)).copy()
    if hosts_out is not None:
        outs = np.atleast_1d(_records(hosts_out, ARP_HOST_OUT_DTYPE))
        assert nxt.size == outs.size, "one out record per host"
        assert (outs["free"].astype(np.uint64) + outs["n_answered"] == nxt["free"]).all(), "hosts_out is not these hosts'"
    if free is not None:
        nxt["free"] = free
    return nxt


def socks_from_connect(openers, out, ring_off=0, ring_size=0, mss: int = 1460):
    """How the openers that left SynSent in a connect call are listed for the next calls: the counterpart
    of socks_from_accept. `openers`: the OPENER_DTYPE rows the call was given, `out` its CONNECT_OUT_DTYPE
    records for them (host array); `ring_off` and `ring_size`: per opener (an array of n_openers entries,
    or one value for all) where the connection's RX ring lies in `rings`. Returns (idx, socks, snd, tx)
    for the openers that came back ST_ESTABLISHED or ST_SYN_RCVD, in opener order: idx their indices; socks
    SOCK_DTYPE rows (key, rcv_nxt, rcv_wnd, snd_nxt = iss + 1: the reply has gone out, a SYN-ACK's SYN
    included; an empty ring); snd SND_DTYPE rows {snd_una, snd_wnd} of the record (a SynRcvd row's snd_una
    is iss, so that the peer's ACK is code 1 with snd_una == iss + 1, as behind an accept call); tx
    TX_SOCK_DTYPE rows whose 54-byte header template is the reply's (the two MACs, addresses and ports
    swapped from the key, the ID seed advanced past the reply, mss = the peer's or `mss` when its SYN had
    none, the send state snd_una = snd_nxt = iss + 1)."""
    openers = np.atleast_1d(np.asarray(openers, dtype=OPENER_DTYPE))
    out = np.atleast_1d(np.asarray(out, dtype=CONNECT_OUT_DTYPE))
    assert openers.size == out.size, "one connect record per opener"
    idx = np.flatnonzero((out["state"] == ST_ESTABLISHED) | (out["state"] == ST_SYN_RCVD))
    ring_off = np.broadcast_to(np.asarray(ring_off, dtype=np.uint64), (openers.size,))[idx]
    ring_size = np.broadcast_to(np.asarray(ring_size, dtype=np.uint32), (openers.size,))[idx]
    s, o = openers[idx], out[idx]
    nxt = s["iss"] + np.uint32(1)
    socks = np.zeros(idx.size, dtype=SOCK_DTYPE)
    socks["key"], socks["rcv_nxt"], socks["rcv_wnd"], socks["snd_nxt"] = s["key"], o["rcv_nxt"], s["rcv_wnd"], nxt
    socks["ring_size"], socks["ring_off"], socks["ring_wpos"], socks["ring_free"] = ring_size, ring_off, 0, ring_size
    snd = np.zeros(idx.size, dtype=SND_DTYPE)
    snd["snd_una"], snd["snd_wnd"] = o["snd_una"], o["snd_wnd"]
    tx = np.zeros(idx.size, dtype=TX_SOCK_DTYPE)
    hdr = tx["hdr"]
    hdr[:, 0:6], hdr[:, 6:12] = s["remote_mac"], s["local_mac"]
    hdr[:, 12], hdr[:, 14], hdr[:, 22], hdr[:, 23], hdr[:, 46] = 0x08, 0x45, 64, 6, 0x50
    for k in range(idx.size):  # the ID the connection's next frame carries: two steps past the seed
        nid = _prand16(_prand16(int(s["ip_id"][k])))
        hdr[k, 18], hdr[k, 19] = nid >> 8, nid & 0xFF
    hdr[:, 26:30], hdr[:, 30:34] = s["key"][:, 5:9], s["key"][:, 1:5]
    hdr[:, 34:36], hdr[:, 36:38] = s["key"][:, 11:13], s["key"][:, 9:11]
    tx["mss"] = np.minimum(np.where(o["peer_mss"] != 0, o["peer_mss"], mss), 65495)  # (the ring send's largest chunk)
    tx["snd_una"] = tx["snd_nxt"] = nxt
    tx["snd_wnd"], tx["rcv_nxt"], tx["rcv_wnd"] = o["snd_wnd"], o["rcv_nxt"], s["rcv_wnd"]
    return idx, socks, snd, tx


def closers_from(socks, socks_close) -> tuple:
    """How the sockets that left Established in a close call are listed for the next calls. `socks`: the
    SOCK_DTYPE rows the call was given, `socks_close` its CLOSE_OUT_DTYPE records for them (host array).
    Returns (idx, closers): idx the rows whose state is no longer ST_ESTABLISHED, closers their
    CLOSER_DTYPE records (key, rcv_wnd and snd_nxt from the row; state, rcv_nxt, snd_una and snd_wnd from
    the record). A row that came back ST_CLOSED or ST_TIME_WAIT is in idx too: the host drops it, or lists
    it as a closer whose frames are then ignored."""
    socks = np.atleast_1d(np.asarray(socks, dtype=SOCK_DTYPE))
    out = np.atleast_1d(np.asarray(socks_close, dtype=CLOSE_OUT_DTYPE))
    assert socks.size == out.size, "one close record per socket"
    idx = np.flatnonzero(out["state"] != ST_ESTABLISHED)
    closers = np.zeros(idx.size, dtype=CLOSER_DTYPE)
    closers["key"], closers["rcv_wnd"], closers["snd_nxt"] = socks["key"][idx], socks["rcv_wnd"][idx], socks["snd_nxt"][idx]
    for name in ("state", "rcv_nxt", "snd_una", "snd_wnd"):
        closers[name] = out[name][idx]
    return idx, closers


def state_after_send(state: int, sent: int) -> int:
    """Send's state changes (control_user.go:118-137) for a connection in `state` (the reference's number)
    after a ring send whose fs_tx_sock_out.sent is `sent`: ST_ESTABLISHED + TX_FIN -> ST_FIN_WAIT_1,
    ST_CLOSE_WAIT + TX_FIN -> ST_LAST_ACK, ST_CLOSING + TX_ACK -> ST_TIME_WAIT; every other pair keeps the
    state."""
    if sent & TX_FIN and state == ST_ESTABLISHED:
        return ST_FIN_WAIT_1
    if sent & TX_FIN and state == ST_CLOSE_WAIT:
        return ST_LAST_ACK
    if sent & TX_ACK and state == ST_CLOSING:
        return ST_TIME_WAIT
    return state


def socks_from_accept(conns, slots, listeners, ring_off, ring_size, mss: int = 1460):
    """How the connections an accept call opened are listed for the next calls. `conns`: the
    ACCEPT_CONN_DTYPE records of the call (host array), `slots` and `listeners` the lists it was given;
    `ring_off` and `ring_size`: per slot (an array of n_slots entries, or one value for all) where the
    connection's RX ring lies in `rings`. Returns (idx, socks, snd, tx) for the filled slots, in slot
    order: idx their slot numbers; socks SOCK_DTYPE rows (key, rcv_nxt, rcv_wnd = the slot's, snd_nxt =
    iss + 1, an empty ring); snd SND_DTYPE rows {iss, the SYN's window}: the handshake's third ACK is then
    code 1 with snd_una == iss + 1; tx TX_SOCK_DTYPE rows whose 54-byte header template answers the peer
    (addresses and ports swapped, the listener's MAC, the ID seed advanced past the SYN-ACK, mss = the
    peer's or `mss` when the SYN had none, the send state snd_una = snd_nxt = iss + 1)."""
    conns = np.atleast_1d(np.asarray(conns, dtype=ACCEPT_CONN_DTYPE))
    slots = np.atleast_1d(np.asarray(slots, dtype=ACCEPT_SLOT_DTYPE))
    listeners = np.atleast_1d(np.asarray(listeners, dtype=LISTENER_DTYPE))
    assert conns.size == slots.size, "one connection record per slot"
    idx = np.flatnonzero(conns["used"])
    ring_off = np.broadcast_to(np.asarray(ring_off, dtype=np.uint64), (slots.size,))[idx]
    ring_size = np.broadcast_to(np.asarray(ring_size, dtype=np.uint32), (slots.size,))[idx]
    c, s = conns[idx], slots[idx]
    # a slot's listener: the one whose range holds it
    owner = np.full(slots.size, -1, dtype=np.int64)
    for k, l in enumerate(listeners):
        owner[int(l["slot_first"]) : int(l["slot_first"]) + int(l["n_slots"])] = k
    assert (owner[idx] >= 0).all(), "a filled slot belongs to a listener"
    lis = listeners[owner[idx]]
    socks = np.zeros(idx.size, dtype=SOCK_DTYPE)
    socks["key"], socks["rcv_nxt"], socks["rcv_wnd"], socks["snd_nxt"] = c["key"], c["rcv_nxt"], s["rcv_wnd"], c["snd_nxt"]
    socks["ring_size"], socks["ring_off"], socks["ring_wpos"], socks["ring_free"] = ring_size, ring_off, 0, ring_size
    snd = np.zeros(idx.size, dtype=SND_DTYPE)
    snd["snd_una"], snd["snd_wnd"] = s["iss"], c["snd_wnd"]
    tx = np.zeros(idx.size, dtype=TX_SOCK_DTYPE)
    hdr = tx["hdr"]
    hdr[:, 0:6], hdr[:, 6:12] = c["remote_mac"], lis["mac"]
    hdr[:, 12], hdr[:, 14], hdr[:, 22], hdr[:, 23], hdr[:, 46] = 0x08, 0x45, 64, 6, 0x50
    for k in range(idx.size):  # the ID the connection's next frame carries: two steps past the seed
        nxt = _prand16(_prand16(int(s["ip_id"][k])))
        hdr[k, 18], hdr[k, 19] = nxt >> 8, nxt & 0xFF
    hdr[:, 26:30], hdr[:, 30:34] = c["key"][:, 5:9], c["key"][:, 1:5]
    hdr[:, 34:36], hdr[:, 36:38] = c["key"][:, 11:13], c["key"][:, 9:11]
    tx["mss"] = np.minimum(np.where(c["peer_mss"] != 0, c["peer_mss"], mss), 65495)  # (the ring send's largest chunk)
    tx["snd_una"] = tx["snd_nxt"] = c["snd_nxt"]
    tx["snd_wnd"], tx["rcv_nxt"], tx["rcv_wnd"] = c["snd_wnd"], c["rcv_nxt"], s["rcv_wnd"]
    return idx, socks, snd, tx


def _prand16(x: int) -> int:
    """The reference's IPv4 ID generator (stacks/port_tcp.go:197-203)."""
    x ^= (x << 7) & 0xFFFF
    x ^= x >> 9
    x ^= (x << 8) & 0xFFFF
    return x


def shard_count(n: int, nshards: int, shard: int) -> int:
    """Frames of shard `shard` when n global frames go round-robin over nshards shards (C ABI)."""
    return int(load_library().fs_shard_count(n, nshards, shard))


def shard_slab_bytes(n: int, nshards: int) -> int:
    """Bytes of one shard's gathered slab: ceil(n/N) digests then ceil(n/N) verdicts, 256-B aligned."""
    return int(load_library().fs_shard_slab_bytes(n, nshards))


class Group(_Handle):
    """One host process driving several GPUs (fs_group): a context, a stream and an RCCL
    communicator per device. `digest_sharded` runs fs_digest_batch_sharded: every device digests
    its round-robin shard chunk by chunk, grouped ncclSend/ncclRecv bring each chunk's digests to
    the first device, a de-interleave kernel restores global order there."""

    _attr, _destroy = "_g", "fs_group_destroy"

    def __init__(self, devices: Sequence[int], lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        self.devices = [int(d) for d in devices]
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        g = _vp()
        st = self.lib.fs_group_create(arr, len(self.devices), ctypes.byref(g))
        if st != FS_SUCCESS:
            raise FramesumError(f"fs_group_create({self.devices}) failed ({st}): "
                                f"{self.lib.fs_group_last_error(None).decode()}")
        self._g = g

    def digest_sharded(self, shards, n: int, mtu: int = 0, out=None, status=None):
        """shards[k] = (frames, offsets int64, lengths int32) CUDA tensors on devices[k] holding
        shard k (fs_shard_count(n, N, k) frames). Returns (out (n, 2) int32, status (n,) uint8)
        on devices[0], in global frame order (synchronous)."""
        import torch

        N = len(self.devices)
        assert len(shards) == N
        fr, of, ln = (_vp * N)(), (_vp * N)(), (_vp * N)()
        for k, (f, o, l) in enumerate(shards):
            assert f.dtype == torch.uint8 and o.dtype == torch.int64 and l.dtype == torch.int32
            assert f.is_contiguous() and o.is_contiguous() and l.is_contiguous()
            assert l.numel() == shard_count(n, N, k) and o.numel() == l.numel()
            assert f.device.index == self.devices[k]
            fr[k], of[k], ln[k] = f.data_ptr(), o.data_ptr(), l.data_ptr()
        out, status = _result_tensors(n, torch.device("cuda", self.devices[0]), out, status)
        st = self.lib.fs_digest_batch_sharded(self._g, fr, of, ln, n, mtu, _tensor_ptr(out), _tensor_ptr(status))
        if st != FS_SUCCESS:
            raise FramesumError(f"fs_digest_batch_sharded failed ({st}): {self.lib.fs_group_last_error(self._g).decode()}")
        return out, status


def pack_frames(frames: Sequence[bytes], align: int = 4):
    """Pack a list of frames into one buffer (each frame at an `align`-aligned offset)."""
    lengths = np.fromiter((len(f) for f in frames), dtype=np.uint32, count=len(frames))
    step = (lengths.astype(np.uint64) + np.uint64(align - 1)) // np.uint64(align) * np.uint64(align)
    offsets = np.zeros(len(frames), dtype=np.uint64)
    if len(frames) > 1:
        offsets[1:] = np.cumsum(step[:-1])
    total = int(offsets[-1] + step[-1]) if len(frames) else 0
    buf = np.zeros(total + 16, dtype=np.uint8)
    for f, o in zip(frames, offsets):
        buf[int(o) : int(o) + len(f)] = np.frombuffer(f, dtype=np.uint8)
    return buf, offsets, lengths


def split_digests(out_words: np.ndarray):
    """(n,2) int32 raw digest words -> (crc32 u32, ip_csum u16, l4_csum u16) numpy arrays."""
    w = np.ascontiguousarray(out_words).view(np.uint32).reshape(-1, 2)
    return w[:, 0].copy(), (w[:, 1] & 0xFFFF).astype(np.uint16), (w[:, 1] >> 16).astype(np.uint16)
