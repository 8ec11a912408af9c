"""The in-order TCP delivery (fs_deliver_flows_batch / fs_deliver_flows_batch_host) without a GPU: the
arithmetic of seqs_amd/csrc/framesum_deliver.h under ASan + UBSan (a stand-alone program run as a child
process), the second header against the binding's table and record layouts, the argument checks
through ctypes, the sequential restatement of tests/deliver_ref.py on hand-written cases against a
byte-by-byte model of the reference ring's Write, and what the Python methods hand to the C ABI
(a recording stand-in for the library)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from seqs_amd import abi, framesum
from seqs_amd.framesum import (DIGEST_DTYPE, FLOW_DTYPE, FLOW_TOTALS_DTYPE, RUN_DTYPE, SOCK_DTYPE, SOCK_OUT_DTYPE, Engine,
                               FramesumError)

import deliver_ref as ref
import flows_ref as fref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tests", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
HEADER = open(os.path.join(ROOT, "include", "framesum_deliver.h")).read()
ACK, FIN = fref.ACK, fref.FIN


def test_deliver_arithmetic_under_asan_ubsan():
    out = os.path.join(CSRC, "build", "test_deliver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *SAN, "-o", out, os.path.join(CSRC, "test_deliver.cpp")],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "deliver checks OK" in r.stdout


# ---- the second header and the binding's tables ----------------------------------------------------

def header_functions():
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    return re.findall(r"^fs_status\s+(fs_\w+)\s*\(", body, flags=re.M)


def test_deliver_prototypes_are_the_headers():
    assert header_functions() == list(abi.DELIVER_PROTOTYPES) == ["fs_deliver_flows_batch", "fs_deliver_flows_batch_host"]
    assert not set(abi.DELIVER_PROTOTYPES) & set(abi.PROTOTYPES) and '#include "framesum.h"' in HEADER
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name, (restype, argtypes) in abi.DELIVER_PROTOTYPES.items():
        params = body[body.index(name + "(") + len(name) + 1 :]
        params = [p.strip() for p in params[: params.index(")")].split(",")]
        assert restype is ctypes.c_int32 and len(params) == len(argtypes), name
        for p, t in zip(params, argtypes):
            want = ctypes.c_void_p if "*" in p else {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}[p.split()[0]]
            assert t is want, (name, p)
    lib = framesum.load_library()
    for name, (restype, argtypes) in abi.DELIVER_PROTOTYPES.items():
        assert getattr(lib, name).restype is restype and getattr(lib, name).argtypes == argtypes


def struct_fields(name):
    body = HEADER[HEADER.index("typedef struct " + name) : HEADER.index("} " + name + ";")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for ctype, names in re.findall(r"(uint\d+_t)\s+([a-z_, \[\]0-9]+);", body):
        out += [(ctype, nm.strip()) for nm in names.split(",")]
    return out


def test_sock_dtypes_are_the_c_structs():
    for name, dtype, size in (("fs_rx_sock", SOCK_DTYPE, 48), ("fs_rx_sock_out", SOCK_OUT_DTYPE, 32)):
        fields = struct_fields(name)
        assert [re.sub(r"\[\d+\]", "", nm) for _, nm in fields] == list(dtype.names) and dtype.itemsize == size
        at = 0
        for ctype, nm in fields:
            count = int(m.group(1)) if (m := re.search(r"\[(\d+)\]", nm)) else 1
            width = int(ctype[4:-2]) // 8
            assert dtype.fields[re.sub(r"\[\d+\]", "", nm)][1] == at, nm
            at += width * count
        assert at == size
    assert abi.DELIVER_MAX_SOCKS == int(re.search(r"#define FS_DELIVER_MAX_SOCKS (\d+)u", HEADER).group(1))


def test_sock_key():
    k = framesum.sock_key("10.0.0.1", 40000, bytes([10, 0, 0, 2]), 80)
    assert k.dtype == np.uint8 and bytes(k) == bytes([6, 10, 0, 0, 1, 10, 0, 0, 2, 0x9C, 0x40, 0, 80])
    assert bytes(framesum.sock_key(0x0A000001, 40000, "10.0.0.2", 80)) == bytes(k)
    # ... which is the key of a frame the socket receives
    hdr = bytearray(fref.flow_header(np.random.default_rng(1), 40000))
    hdr[26:34] = bytes([10, 0, 0, 1, 10, 0, 0, 2])
    assert fref.flow_key(bytes(hdr)) == bytes(k)
    with pytest.raises(AssertionError):
        framesum.sock_key(b"\x01\x02\x03", 1, "1.2.3.4", 2)


def test_argument_checks_need_no_device():
    lib = framesum.load_library()
    none = ctypes.c_void_p()
    some = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    assert lib.fs_deliver_flows_batch(None, some, some, some, 1, 0, 0, some, 1, some, 64, some, none, some, 8, some, some,
                                      some, none, some, none, none, none) == -1
    assert lib.fs_deliver_flows_batch_host(None, some, 64, some, some, 1, 0, 0, some, 1, some, 64, some, none, some, 8,
                                           some, some, some, none, some, none, none) == -1


# ---- the restatement on hand-written cases -----------------------------------------------------------

class ModelRing:
    """A byte-by-byte model of where the reference's ring (stacks/ring.go:17-40) places a write: the
    ring holds `used` bytes ending at the write position `end`; a write of more than the free bytes
    is refused whole, else byte j lands at (end + j) mod size, and never on a byte still buffered."""

    def __init__(self, size, read_pos, used):
        self.buf, self.size = bytearray(size), size
        self.live = {(read_pos + j) % size for j in range(used)}
        self.end = (read_pos + used) % size

    def free(self):
        return self.size - len(self.live)

    def write(self, data: bytes) -> int:
        if len(data) > self.free():
            return 0
        for j, c in enumerate(data):
            at = (self.end + j) % self.size
            assert at not in self.live, "a write over buffered bytes"
            self.buf[at] = c
            self.live.add(at)
        self.end = (self.end + len(data)) % self.size
        return len(data)


@pytest.mark.parametrize("size,read_pos,used,lens", [
    (64, 0, 0, [10, 20, 30, 4]),        # an empty ring filled to its last byte
    (64, 40, 10, [10, 4, 30, 6]),       # the tail, then across the wrap, then the middle
    (64, 50, 24, [20, 20]),             # wrapped already: the middle only
    (4096, 3000, 1000, [100, 100, 100]),
    (7, 3, 3, [1, 3]),                  # a write that ends exactly at the ring's end, then one from its start
])
def test_ring_write_is_the_references(size, read_pos, used, lens):
    rng = np.random.default_rng(size + read_pos)
    model = ModelRing(size, read_pos, used)
    mine = np.zeros(size, dtype=np.uint8)
    wpos, free = model.end, model.free()
    for ln in lens:
        data = rng.integers(1, 256, ln, dtype=np.uint8).tobytes()
        assert ln <= free and model.write(data) == ln
        wpos = ref.ring_write(mine, wpos, data)
        free -= ln
        assert bytes(model.buf) == mine.tobytes() and wpos == model.end and free == model.free()
    assert model.write(bytes(free + 1)) == 0  # more than the free bytes: refused whole (rule (d))


def hand_case():
    """Two interleaved flows and a UDP datagram; flow A has a socket whose ring wraps, flow B none."""
    rng = np.random.default_rng(5)
    ha, hb = fref.flow_header(rng, 0xA000), fref.flow_header(rng, 0xB000)
    a = [fref.tcp_frame(ha, 1000, b"0123456789"), fref.tcp_frame(ha, 1010, b""),          # data, a pure ACK
         fref.tcp_frame(ha, 1011, b"skipped one"),                                        # nxt + 1
         fref.tcp_frame(ha, 1010, b"abcdef"), fref.tcp_frame(ha, 1016, b"XY", flags=ACK | FIN),
         fref.tcp_frame(ha, 1019, b"behind the FIN")]
    b = fref.segments(rng, hb, 7, [5, 5])
    frames = fref.finish([a[0], b[0], a[1], a[2], fref.udp_frame(rng, b"udp"), a[3], b[1], a[4], a[5]])
    return ha, frames


def test_restatement_on_the_hand_computed_case():
    ha, frames = hand_case()
    buf, off, ln = fref.pack(frames, lead=3)
    snd = int.from_bytes(ha[42:46], "big")
    noise = np.zeros(int(ln.sum()), dtype=np.uint8)
    # free 16: 10 + 6 bytes are admitted, the FIN frame's 2 bytes are not (rule (d)); nxt stays, no FIN seen
    socks = ref.socks_of(ref.sock(ref.key_of_header(ha), 1000, 4, 16, snd_nxt=snd, ring_wpos=12, ring_free=16))
    rings = np.full(24, 0xEE, dtype=np.uint8)
    e = ref.expected(buf, off, ln, 0, 0, noise, 0, None, socks, rings)
    assert list(e["delivered"]) == [1, 0, 0, 2, 0, 1, 0, 2, 2]
    o = e["socks_out"][0]
    assert [int(o[k]) for k in o.dtype.names] == [1016, 12, 0, 16, 2, 3, 0, 6]
    want = b"0123456789abcdef"
    ring = bytearray(16)
    for j, c in enumerate(want):
        ring[(12 + j) % 16] = c
    assert e["rings"].tobytes() == b"\xEE" * 4 + bytes(ring) + b"\xEE" * 4
    # Ack one above snd_nxt: nothing of the flow is admitted, the ring stays as it was
    socks["snd_nxt"] = (snd - 1) % (1 << 32)
    e = ref.expected(buf, off, ln, 0, 0, noise, 0, None, socks, rings)
    assert int(e["socks_out"]["n_delivered"][0]) == 0 and np.array_equal(e["rings"], rings)
    # a socket for nobody
    socks = ref.socks_of(ref.sock(bytes([6]) + bytes(12), 1, 0, 8))
    e = ref.expected(buf, off, ln, 0, 0, noise, 0, None, socks, rings)
    assert int(e["socks_out"]["flow"][0]) == ref.NONE and not e["delivered"].any() and np.array_equal(e["rings"], rings)


# ---- the binding: what the methods hand to the C ABI -------------------------------------------------

TOTALS = {"payload_bytes": 3000, "n_runs": 2, "n_flows": 1, "n_accepted": 3}
MESSAGE = b"the stand-in says no"


class StandInFunction:
    def __init__(self, lib, name):
        self.lib, self.name, self.restype, self.argtypes = lib, name, None, None

    def __call__(self, *args):
        self.lib.calls.append((self.name, args))
        if self.name == "fs_last_error":
            return MESSAGE
        if self.name in self.lib.fail:
            return self.lib.fail[self.name]
        if self.name == "fs_ctx_create":
            args[1]._obj.value = 0x5000
        elif self.name == "fs_deliver_flows_batch_host":
            raw = (ctypes.c_uint8 * FLOW_TOTALS_DTYPE.itemsize).from_address(args[20].value)
            t = np.frombuffer(raw, dtype=FLOW_TOTALS_DTYPE, count=1)
            for field in t.dtype.names:
                t[field] = TOTALS.get(field, 0)
        return 0


class StandInLibrary:
    def __init__(self, path):
        self.path, self.calls, self.fail = path, [], {}

    def __getattr__(self, name):
        if not name.startswith("fs_") or name in abi.OPTIONAL_PROTOTYPES:
            raise AttributeError(name)
        fn = StandInFunction(self, name)
        setattr(self, name, fn)
        return fn


@pytest.fixture
def eng(monkeypatch, tmp_path):
    product = tmp_path / "libframesum.so"
    product.write_bytes(b"")
    monkeypatch.setattr(ctypes, "CDLL", StandInLibrary)
    monkeypatch.setattr(abi, "_LIB_PATH", str(product))
    monkeypatch.setattr(abi, "_lib", None)
    monkeypatch.setattr(abi, "_libs", {})
    e = Engine(0)
    for name, (restype, argtypes) in abi.DELIVER_PROTOTYPES.items():  # the loader set the second table too
        assert getattr(e.lib, name).restype is restype and getattr(e.lib, name).argtypes == argtypes
    e.lib.calls.clear()
    yield e
    e.close()


def plain(a):
    return getattr(a, "value", a)


def test_deliver_flows_host_marshals(eng):
    lengths = np.array([60, 61, 1514], dtype=np.uint32)
    offsets = np.array([0, 60, 124], dtype=np.uint64)
    frames = np.arange(1640, dtype=np.uint32).astype(np.uint8)
    socks = np.zeros(2, dtype=SOCK_DTYPE)
    rings = np.zeros(500, dtype=np.uint8)
    res = eng.deliver_flows_host(frames, offsets, lengths, socks, rings, 1500, 1)
    socks_out, delivered, payload, runs, flows, order, run_of, totals, out, status = res
    (call,) = eng.lib.calls
    name, args = call
    want = [eng._ctx.value, frames, frames.nbytes, offsets, lengths, 3, 1500, 1, socks, 2, rings, 500, socks_out, delivered,
            payload, 60 + 61 + 1514, None, None, None, run_of, None, out, status]
    assert name == "fs_deliver_flows_batch_host" and len(args) == len(want) == 23
    for k, (a, w) in enumerate(zip(args, want)):
        if w is not None:
            assert plain(a) == (w.ctypes.data if isinstance(w, np.ndarray) else w), f"argument {k}"
    assert socks_out.dtype == SOCK_OUT_DTYPE and socks_out.shape == (2,) and delivered.dtype == np.uint8
    assert delivered.shape == (3,) and runs.dtype == RUN_DTYPE and runs.shape == (TOTALS["n_runs"],)
    assert flows.dtype == FLOW_DTYPE and flows.shape == (TOTALS["n_flows"],) and order.shape == (TOTALS["n_accepted"],)
    assert totals.dtype == FLOW_TOTALS_DTYPE and int(totals["n_accepted"]) == 3 and out.dtype == DIGEST_DTYPE
    # no packed copy, no delivered array: null pointers and a cap of 0
    res = eng.deliver_flows_host(frames, offsets, lengths, socks, rings, payload=False, delivered=False)
    args = eng.lib.calls[1][1]
    assert res[1] is None and res[2] is None
    assert [plain(args[k]) for k in (13, 14, 15)] == [None, None, 0] and [plain(args[k]) for k in (6, 7)] == [0, 0]
    # the rings are written in place: never copied, so they must be a writable uint8 array already
    frozen = rings.copy()
    frozen.flags.writeable = False
    for bad in (frozen, list(rings), rings.astype(np.int8), rings[::2]):
        with pytest.raises(AssertionError):
            eng.deliver_flows_host(frames, offsets, lengths, socks, bad)
    assert len(eng.lib.calls) == 2
    eng.lib.fail["fs_deliver_flows_batch_host"] = -1
    with pytest.raises(FramesumError) as err:
        eng.deliver_flows_host(frames, offsets, lengths, socks, rings)
    assert str(err.value) == f"fs_deliver_flows_batch_host failed (-1): {MESSAGE.decode()}"


def test_a_library_without_the_symbol_raises(monkeypatch, tmp_path):
    class Older(StandInLibrary):
        def __getattr__(self, name):
            if name == "fs_deliver_flows_batch":
                raise AttributeError(name)
            return super().__getattr__(name)

    product = tmp_path / "libframesum.so"
    product.write_bytes(b"")
    monkeypatch.setattr(ctypes, "CDLL", Older)
    monkeypatch.setattr(abi, "_LIB_PATH", str(product))
    monkeypatch.setattr(abi, "_lib", None)
    monkeypatch.setattr(abi, "_libs", {})
    with pytest.raises(AttributeError, match="fs_deliver_flows_batch"):
        framesum.load_library()
