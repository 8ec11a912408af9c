"""The receive call (fs_recv_flows_batch / fs_recv_flows_batch_host) without a GPU: the arithmetic of
seqs_amd/csrc/framesum_recv.h under ASan + UBSan (a stand-alone program run as a child process), the
fourth header against the binding's table and record layouts, the argument checks through ctypes,
what the Python methods hand to the C ABI (tests/test_deliver_host.py's recording stand-in),
tx_sock_from with and without snd_out, and the agreement of the two restatements of
tests/recv_ref.py over a grid of segments."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # (before the stand-in replaces ctypes.CDLL: torch loads its own libraries through it)

from seqs_amd import abi, framesum
from seqs_amd.framesum import (DIGEST_DTYPE, FLOW_TOTALS_DTYPE, SND_DTYPE, SND_OUT_DTYPE, SOCK_DTYPE, SOCK_OUT_DTYPE,
                               TX_SOCK_DTYPE, FramesumError)

import recv_ref as ref
from test_deliver_host import MESSAGE, SAN, TOTALS, StandInFunction, StandInLibrary, plain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tests", "csrc")
HEADER = open(os.path.join(ROOT, "include", "framesum_recv.h")).read()
BODY = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
DELIVER_BODY = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "framesum_deliver.h")).read(), flags=re.S)
M32 = ref.M32
ACK, PSH, FIN, NS = ref.ACK, ref.PSH, ref.FIN, ref.NS


def test_recv_arithmetic_under_asan_ubsan():
    out = os.path.join(CSRC, "build", "test_recv")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *SAN, "-o", out, os.path.join(CSRC, "test_recv.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "recv checks OK" in r.stdout


# ---- the fourth header and the binding's tables ------------------------------------------------------

def params_of(body, name):
    p = body[body.index(name + "(") + len(name) + 1 :]
    return [x.strip() for x in p[: p.index(")")].split(",")]


def test_recv_prototypes_are_the_headers():
    names = ["fs_recv_flows_batch", "fs_recv_flows_batch_host"]
    assert re.findall(r"^fs_status\s+(fs_\w+)\s*\(", BODY, flags=re.M) == list(abi.RECV_PROTOTYPES) == names
    others = set(abi.PROTOTYPES) | set(abi.DELIVER_PROTOTYPES) | set(abi.SEND_RINGS_PROTOTYPES)
    assert not set(abi.RECV_PROTOTYPES) & others and '#include "framesum_deliver.h"' in HEADER
    for name, (restype, argtypes) in abi.RECV_PROTOTYPES.items():
        params = params_of(BODY, name)
        assert restype is ctypes.c_int32 and len(params) == len(argtypes) == 26, name
        for p, t in zip(params, argtypes):
            want = ctypes.c_void_p if "*" in p else {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}[p.split()[0]]
            assert t is want, (name, p)
        # every parameter of the delivery call up to and including `delivered`, the three new ones, the rest
        theirs = params_of(DELIVER_BODY, name.replace("recv", "deliver"))
        at = theirs.index("uint8_t* delivered") + 1
        assert params == theirs[:at] + ["const fs_rx_snd* snd", "fs_rx_snd_out* snd_out", "uint8_t* code"] + theirs[at:]
    lib = framesum.load_library()
    for name, (restype, argtypes) in abi.RECV_PROTOTYPES.items():
        assert getattr(lib, name).restype is restype and getattr(lib, name).argtypes == argtypes


def test_snd_dtypes_and_constants_are_the_headers():
    for name, dtype, size in (("fs_rx_snd", SND_DTYPE, 8), ("fs_rx_snd_out", SND_OUT_DTYPE, 32)):
        body = BODY[BODY.index("typedef struct " + name + " {") : BODY.index("} " + name + ";")]
        fields = [nm.strip() for _, names in re.findall(r"(uint32_t)\s+([a-z_, ]+);", body) for nm in names.split(",")]
        assert fields == list(dtype.names) and dtype.itemsize == size
        assert [dtype.fields[f][1] for f in fields] == list(range(0, size, 4))
    defines = dict(re.findall(r"#define (FS_RECV_\w+) (\d+)u", HEADER))
    assert (int(defines["FS_RECV_ACK_OWED"]), int(defines["FS_RECV_FIN"])) == (abi.RECV_ACK_OWED, abi.RECV_FIN) == (1, 2)
    assert (abi.RECV_NONE, abi.RECV_TAKEN, abi.RECV_DUPLICATE, abi.RECV_UNSENT, abi.RECV_REJECTED, abi.RECV_KEEPALIVE,
            abi.RECV_RING_FULL) == (0, ref.TAKEN, ref.DUPLICATE, ref.UNSENT, ref.REJECTED, ref.KEEPALIVE, ref.RING_FULL)
    # the header states both differences from the reference
    text = " ".join(HEADER.split())
    assert "never clears FS_RECV_ACK_OWED" in text.replace("* ", "") and "ring is full" in text.replace("* ", "")


def test_argument_checks_need_no_device():
    lib = framesum.load_library()
    none = ctypes.c_void_p()
    some = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    assert lib.fs_recv_flows_batch(None, some, some, some, 1, 0, 0, some, 1, some, 64, some, none, some, some, none, some, 8,
                                   some, some, some, none, some, none, none, none) == -1
    assert lib.fs_recv_flows_batch_host(None, some, 64, some, some, 1, 0, 0, some, 1, some, 64, some, none, some, some, none,
                                        some, 8, some, some, some, none, some, none, none) == -1


# ---- the binding: what the methods hand to the C ABI ---------------------------------------------------

class RecvFunction(StandInFunction):
    """The recording stand-in's function, which also fills the totals of the receive call's host form."""

    def __call__(self, *args):
        res = super().__call__(*args)
        if self.name == "fs_recv_flows_batch_host" and res == 0:
            raw = (ctypes.c_uint8 * FLOW_TOTALS_DTYPE.itemsize).from_address(args[23].value)
            t = np.frombuffer(raw, dtype=FLOW_TOTALS_DTYPE, count=1)
            for field in t.dtype.names:
                t[field] = TOTALS.get(field, 0)
        return res


class RecvStandIn(StandInLibrary):
    def __getattr__(self, name):
        if not name.startswith("fs_") or name in abi.OPTIONAL_PROTOTYPES:
            raise AttributeError(name)
        fn = RecvFunction(self, name)
        setattr(self, name, fn)
        return fn


@pytest.fixture
def eng(monkeypatch, tmp_path):
    product = tmp_path / "libframesum.so"
    product.write_bytes(b"")
    monkeypatch.setattr(ctypes, "CDLL", RecvStandIn)
    monkeypatch.setattr(abi, "_LIB_PATH", str(product))
    monkeypatch.setattr(abi, "_lib", None)
    monkeypatch.setattr(abi, "_libs", {})
    e = framesum.Engine(0)
    for name, (restype, argtypes) in abi.RECV_PROTOTYPES.items():  # the loader set the fourth table too
        assert getattr(e.lib, name).restype is restype and getattr(e.lib, name).argtypes == argtypes
    e.lib.calls.clear()
    yield e
    e.close()


def test_recv_flows_host_marshals(eng):
    lengths = np.array([60, 61, 1514], dtype=np.uint32)
    offsets = np.array([0, 60, 124], dtype=np.uint64)
    frames = np.arange(1640, dtype=np.uint32).astype(np.uint8)
    socks = np.zeros(2, dtype=SOCK_DTYPE)
    snd = ref.snd_of((5, 100), (6, 200))
    rings = np.zeros(500, dtype=np.uint8)
    res = eng.recv_flows_host(frames, offsets, lengths, socks, snd, rings, 1500, 1)
    snd_out, code, socks_out, delivered, payload, runs, flows, order, run_of, totals, out, status = res
    (call,) = eng.lib.calls
    name, args = call
    want = [eng._ctx.value, frames, frames.nbytes, offsets, lengths, 3, 1500, 1, socks, 2, rings, 500, socks_out, delivered, snd,
            snd_out, code, payload, 60 + 61 + 1514, None, None, None, run_of, None, out, status]
    assert name == "fs_recv_flows_batch_host" and len(args) == len(want) == 26
    for k, (a, w) in enumerate(zip(args, want)):
        if w is not None:
            assert plain(a) == (w.ctypes.data if isinstance(w, np.ndarray) else w), f"argument {k}"
    assert snd_out.dtype == SND_OUT_DTYPE and snd_out.shape == (2,) and code.dtype == np.uint8 and code.shape == (3,)
    assert socks_out.dtype == SOCK_OUT_DTYPE and delivered.shape == (3,) and runs.shape == (TOTALS["n_runs"],)
    assert flows.shape == (TOTALS["n_flows"],) and order.shape == (TOTALS["n_accepted"],) and out.dtype == DIGEST_DTYPE
    # no packed copy, no delivered array, no code array: null pointers and a cap of 0
    res = eng.recv_flows_host(frames, offsets, lengths, socks, snd, rings, payload=False, delivered=False, code=False)
    args = eng.lib.calls[1][1]
    assert res[1] is None and res[3] is None and res[4] is None
    assert [plain(args[k]) for k in (13, 16, 17, 18)] == [None, None, None, 0]
    # one send-side record per socket; the rings a writable uint8 array
    with pytest.raises(AssertionError):
        eng.recv_flows_host(frames, offsets, lengths, socks, snd[:1], rings)
    frozen = rings.copy()
    frozen.flags.writeable = False
    with pytest.raises(AssertionError):
        eng.recv_flows_host(frames, offsets, lengths, socks, snd, frozen)
    assert len(eng.lib.calls) == 2
    eng.lib.fail["fs_recv_flows_batch_host"] = -1
    with pytest.raises(FramesumError) as err:
        eng.recv_flows_host(frames, offsets, lengths, socks, snd, rings)
    assert str(err.value) == f"fs_recv_flows_batch_host failed (-1): {MESSAGE.decode()}"


class OnDevice:
    """A CPU tensor that says it is a CUDA tensor: the binding takes only its pointer and its size."""

    def __init__(self, t):
        self.t, self.is_cuda, self.dtype, self.device = t, True, t.dtype, t.device

    def numel(self):
        return self.t.numel()

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self.t.data_ptr()


class Stream:
    cuda_stream = 0x77


def test_recv_flows_device_marshals(eng):
    frames = OnDevice(torch.zeros(1640, dtype=torch.uint8))
    offsets = OnDevice(torch.tensor([0, 60, 124], dtype=torch.int64))
    lengths = OnDevice(torch.tensor([60, 61, 1514], dtype=torch.int32))
    rings = OnDevice(torch.zeros(500, dtype=torch.uint8))
    socks, snd = np.zeros(2, dtype=SOCK_DTYPE), ref.snd_of((5, 100), (6, 200))
    res = eng.recv_flows_device(frames, offsets, lengths, socks, snd, rings, 1500, 1, payload=False, stream=Stream())
    snd_out, code, socks_out, delivered, payload, runs, flows, order, run_of, totals, out, status = res
    (call,) = eng.lib.calls
    name, args = call
    want = [eng._ctx.value, frames, offsets, lengths, 3, 1500, 1, socks, 2, rings, 500, socks_out, delivered, snd, snd_out, code,
            None, 0, runs, flows, order, run_of, totals, out, status, 0x77]
    assert name == "fs_recv_flows_batch" and len(args) == len(want) == 26 and payload is None
    for k, (a, w) in enumerate(zip(args, want)):
        w = w.ctypes.data if isinstance(w, np.ndarray) else w.data_ptr() if hasattr(w, "data_ptr") else w
        assert plain(a) == w, f"argument {k}"
    assert tuple(snd_out.shape) == (2, 32) and tuple(socks_out.shape) == (2, 32) and snd_out.dtype == torch.uint8
    assert tuple(code.shape) == (3,) and code.dtype == torch.uint8 and tuple(delivered.shape) == (3,)
    res = eng.recv_flows_device(frames, offsets, lengths, socks, snd, rings, payload=False, delivered=False, code=False,
                                stream=Stream())
    args = eng.lib.calls[1][1]
    assert res[1] is None and res[3] is None and [plain(args[k]) for k in (12, 15)] == [None, None]
    with pytest.raises(AssertionError):
        eng.recv_flows_device(frames, offsets, lengths, socks, snd[:1], rings, stream=Stream())


def test_a_library_without_the_symbol_raises(monkeypatch, tmp_path):
    class Older(StandInLibrary):
        def __getattr__(self, name):
            if name == "fs_recv_flows_batch":
                raise AttributeError(name)
            return super().__getattr__(name)

    product = tmp_path / "libframesum.so"
    product.write_bytes(b"")
    monkeypatch.setattr(ctypes, "CDLL", Older)
    monkeypatch.setattr(abi, "_LIB_PATH", str(product))
    monkeypatch.setattr(abi, "_lib", None)
    monkeypatch.setattr(abi, "_libs", {})
    with pytest.raises(AttributeError, match="fs_recv_flows_batch"):
        framesum.load_library()


def test_tx_sock_from_with_and_without_snd_out():
    so = np.zeros(3, dtype=SOCK_OUT_DTYPE)
    so["rcv_nxt"], so["ring_free"] = [10, 20, 30], [100, 200, 300]
    tx = np.zeros(3, dtype=TX_SOCK_DTYPE)
    tx["snd_una"], tx["snd_nxt"], tx["snd_wnd"], tx["flags"] = [1, 2, 3], [7, 8, 9], [11, 12, 13], [0, framesum.TX_PSH, 0]
    plain_res = framesum.tx_sock_from(so, tx)
    assert plain_res.tobytes() == framesum.tx_sock_from(so, tx, snd_out=None).tobytes()
    assert list(plain_res["snd_una"]) == [1, 2, 3] and list(plain_res["flags"]) == [0, framesum.TX_PSH, 0]
    snd_out = np.zeros(3, dtype=SND_OUT_DTYPE)
    snd_out["snd_una"], snd_out["snd_wnd"] = [4, 5, 6], [1000, 0, 65535]
    snd_out["flags"] = [abi.RECV_ACK_OWED, abi.RECV_ACK_OWED | abi.RECV_FIN, abi.RECV_FIN]
    res = framesum.tx_sock_from(so, tx, snd_out=snd_out)
    assert list(res["snd_una"]) == [4, 5, 6] and list(res["snd_wnd"]) == [1000, 0, 65535] and list(res["snd_nxt"]) == [7, 8, 9]
    assert list(res["flags"]) == [framesum.TX_ACK, framesum.TX_PSH | framesum.TX_ACK, 0]
    assert list(res["rcv_nxt"]) == [10, 20, 30] and list(res["rcv_wnd"]) == [100, 200, 300]
    # everything else is the record without snd_out
    for name in TX_SOCK_DTYPE.names:
        if name not in ("snd_una", "snd_wnd", "flags"):
            assert res[name].tobytes() == plain_res[name].tobytes()
    assert list(framesum.tx_sock_from(so, tx, snd_out=snd_out, flags=framesum.TX_FIN)["flags"]) == [3, 3, 2]
    with pytest.raises(AssertionError):
        framesum.tx_sock_from(so, tx, snd_out=snd_out[:2])


# ---- the two restatements agree ------------------------------------------------------------------------

HALF = 1 << 31
FLAG_SETS = [0, ACK, ACK | PSH, PSH, FIN | ACK, NS | ACK]


def grid(una, snd_nxt, nxt):
    acks = [una - 1, una, una + 1, snd_nxt - 1, snd_nxt, snd_nxt + 1, snd_nxt - HALF, snd_nxt - HALF - 1, snd_nxt - HALF + 1]
    for dseq, ack, flags9, length in itertools.product((-2, -1, 0, 1), acks, FLAG_SETS, (0, 1)):
        yield ((nxt + dseq) % M32, ack % M32, 4242, flags9, length)


STATES = [(una % M32, snd % M32, nxt % M32) for una, snd in ((990, 1000), (1000, 1000), (M32 - 3, 5), (M32 - 20, M32 - 10),
                                                             (2, 4), (1000 - HALF, 1000))
          for nxt in (5000, M32 - 1, 0)]


def bare_fin_at_zero_window(seg, nxt, rcv_wnd):
    return rcv_wnd == 0 and seg[4] == 0 and bool(seg[3] & FIN) and seg[0] == nxt


@pytest.mark.parametrize("rcv_wnd", [0, 1, 65535])
def test_the_two_restatements_agree_on_single_segments(rcv_wnd):
    seen, zero_window_fins = set(), 0
    for una, snd_nxt, nxt in STATES:
        for seg in grid(una, snd_nxt, nxt):
            codes_go, tcb = ref.go_walk([seg], una, 777, nxt, snd_nxt, rcv_wnd)
            # without a ring, the delivery admits what passes (a) to (c): the reference's acceptance
            seq, ack, window, flags9, length = seg
            considered = length != 0 or flags9 & FIN
            admitted = bool(considered) and codes_go == [ref.TAKEN]
            if bare_fin_at_zero_window(seg, nxt, rcv_wnd):
                # the delivery's rule (b) admits nothing at a zero window; the reference's zeroWindowOK lets
                # a FIN without data pass its window checks (control.go:291). Stated, and asserted here.
                codes, una2, wnd2, flags = ref.contract([seg], [False], una, 777, nxt, snd_nxt, rcv_wnd)
                assert codes == [ref.REJECTED] and (una2, wnd2, flags) == (una, 777, 0)
                assert codes_go[0] in (ref.TAKEN, ref.UNSENT)
                zero_window_fins += 1
                continue
            codes, una2, wnd2, flags = ref.contract([seg], [admitted], una, 777, nxt, snd_nxt, rcv_wnd)
            assert codes == codes_go, (una, snd_nxt, nxt, seg, codes, codes_go)
            assert (una2, wnd2) == (tcb.snd_UNA, tcb.snd_WND), (una, snd_nxt, nxt, seg)
            assert bool(flags & ref.ACK_OWED) == bool(tcb.pending0 & ACK)  # (one segment: no duplicate after data)
            assert bool(flags & ref.FIN_SEEN) == (not tcb.established)
            seen.add(codes[0])
    assert seen == {ref.TAKEN, ref.DUPLICATE, ref.UNSENT, ref.REJECTED, ref.KEEPALIVE}
    assert (zero_window_fins > 0) == (rcv_wnd == 0)


def test_the_two_restatements_agree_on_sequences():
    """Random sequences drawn from the grid, rcv.NXT and snd.UNA moving: codes and state agree; the ACK
    owed differs exactly where the reference's duplicate has cleared a pending ACK."""
    rng = np.random.default_rng(2031)
    cleared = 0
    for round_ in range(600):
        una, snd_nxt, nxt = STATES[round_ % len(STATES)]
        rcv_wnd = (0, 1, 65535, 65535)[round_ % 4]
        segs, k_nxt, k_una = [], nxt, una
        for _ in range(int(rng.integers(1, 12))):
            pool = list(grid(k_una, snd_nxt, k_nxt))
            seg = pool[int(rng.integers(0, len(pool)))]
            if seg[3] & FIN and (rng.integers(0, 4) or bare_fin_at_zero_window(seg, k_nxt, rcv_wnd)):
                continue  # (a FIN ends the walk: keep most sequences going; the zero-window FIN is the test above's)
            segs.append(seg)
            c, tcb = ref.go_walk(segs, una, 777, nxt, snd_nxt, rcv_wnd)
            k_nxt, k_una = tcb.rcv_NXT, tcb.snd_UNA
        codes_go, tcb = ref.go_walk(segs, una, 777, nxt, snd_nxt, rcv_wnd)
        segs = segs[: len(codes_go)]  # (the walk stops behind an accepted FIN)
        admitted = [bool(s[4] != 0 or s[3] & FIN) and c == ref.TAKEN for s, c in zip(segs, codes_go)]
        codes, una2, wnd2, flags = ref.contract(segs, admitted, una, 777, nxt, snd_nxt, rcv_wnd)
        assert codes == codes_go and (una2, wnd2) == (tcb.snd_UNA, tcb.snd_WND), (round_, segs)
        # the stated difference: sticky here, cleared by a later duplicate there
        owed_go = bool(tcb.pending0 & ACK)
        owed = bool(flags & ref.ACK_OWED)
        last_dup = max((k for k, c in enumerate(codes) if c == ref.DUPLICATE), default=-1)
        sticky = any(c == ref.UNSENT or (c == ref.TAKEN and a) for c, a in zip(codes, admitted))
        after = any(c == ref.UNSENT or (c == ref.TAKEN and a) for c, a in list(zip(codes, admitted))[last_dup + 1 :])
        assert owed == sticky and owed_go == after
        cleared += owed and not owed_go
    assert cleared > 10


def test_ring_full_and_sticky_ack_explicitly():
    # a data segment that passes (a) to (c) and is not admitted: code 6, nothing taken, rcv.NXT stays,
    # so the retransmission behind it is in order
    segs = [(5000, 1000, 111, ACK, 10), (5000, 1000, 222, ACK, 10), (5010, 1000, 333, ACK, 0)]
    codes, una, wnd, flags = ref.contract(segs, [False, True, False], 990, 777, 5000, 1000, 65535)
    # (the third is a duplicate, Ack == una: its window 333 is not taken)
    assert codes == [ref.RING_FULL, ref.TAKEN, ref.DUPLICATE] and (una, wnd) == (1000, 222) and flags == ref.ACK_OWED
    # data, then a duplicate ACK: the ACK stays owed here, the reference has cleared it
    segs = [(5000, 1000, 111, ACK, 10), (5010, 1000, 222, ACK, 0)]
    codes, una, wnd, flags = ref.contract(segs, [True, False], 990, 777, 5000, 1000, 65535)
    codes_go, tcb = ref.go_walk(segs, 990, 777, 5000, 1000, 65535)
    assert codes == codes_go == [ref.TAKEN, ref.DUPLICATE] and flags & ref.ACK_OWED and not tcb.pending0 & ACK
    assert (una, wnd) == (tcb.snd_UNA, tcb.snd_WND) == (1000, 111)
    # an accepted data segment sets una even backwards
    segs = [(5000, 900, 111, ACK, 10)]
    assert ref.contract(segs, [True], 990, 777, 5000, 1000, 65535)[1:3] == (900, 111)
    assert ref.go_walk(segs, 990, 777, 5000, 1000, 65535)[1].snd_UNA == 900
