"""The ring send (fs_send_rings_layout / fs_send_rings_batch / fs_send_rings_batch_host) without a GPU:
the arithmetic of seqs_amd/csrc/framesum_send.h under ASan + UBSan (a stand-alone program run as a
child process), the third header against the binding's table and record layouts, the per-socket rule
of the loaded library (fs_send_rings_layout needs no device) against tests/send_ref.py on every batch
of the GPU suite, the frames that reference expects through the C oracle, every FS_E_INVALID, and what
the Python methods hand to the C ABI (a recording stand-in for the library)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import coracle
from seqs_amd import abi, framesum
from seqs_amd.framesum import (DIGEST_DTYPE, SOCK_OUT_DTYPE, TX_SOCK_DTYPE, TX_SOCK_OUT_DTYPE, Engine, FramesumError,
                               send_rings_layout, tx_sock_from)

import segment_ref as sref
import send_cases as cases
import send_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tests", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
HEADER = open(os.path.join(ROOT, "include", "framesum_send.h")).read()
BODY = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
NAMES = ["fs_send_rings_layout", "fs_send_rings_batch", "fs_send_rings_batch_host"]


def test_send_arithmetic_under_asan_ubsan():
    out = os.path.join(CSRC, "build", "test_send")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *SAN, "-o", out, os.path.join(CSRC, "test_send.cpp")],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "send checks OK" in r.stdout


# ---- the third header and the binding's tables -------------------------------------------------------

def test_send_prototypes_are_the_headers():
    assert re.findall(r"^fs_status\s+(fs_\w+)\s*\(", BODY, flags=re.M) == list(abi.SEND_RINGS_PROTOTYPES) == NAMES
    assert not set(abi.SEND_RINGS_PROTOTYPES) & (set(abi.PROTOTYPES) | set(abi.DELIVER_PROTOTYPES))
    assert '#include "framesum.h"' in HEADER
    for name, (restype, argtypes) in abi.SEND_RINGS_PROTOTYPES.items():
        params = BODY[BODY.index(name + "(") + len(name) + 1 :]
        params = [p.strip() for p in params[: params.index(")")].split(",")]
        assert restype is ctypes.c_int32 and len(params) == len(argtypes), name
        for p, t in zip(params, argtypes):
            if "*" not in p:
                want = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}[p.split()[0]]
            elif p.startswith("uint64_t*") and name.endswith("_layout"):
                want = ctypes.POINTER(ctypes.c_uint64)
            else:
                want = ctypes.c_void_p
            assert t is want, (name, p)
    lib = framesum.load_library()
    for name, (restype, argtypes) in abi.SEND_RINGS_PROTOTYPES.items():
        assert getattr(lib, name).restype is restype and getattr(lib, name).argtypes == argtypes
    out = subprocess.run(["nm", "-D", "--defined-only", framesum.lib_path()], capture_output=True, text=True, check=True)
    assert set(NAMES) <= {l.split()[-1] for l in out.stdout.splitlines() if l.strip()}


def struct_fields(name):
    body = HEADER[HEADER.index("typedef struct " + name) : HEADER.index("} " + name + ";")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for ctype, names in re.findall(r"(uint\d+_t)\s+([a-z_, \[\]0-9]+);", body):
        out += [(ctype, nm.strip()) for nm in names.split(",")]
    return out


def test_tx_sock_dtypes_are_the_c_structs():
    for name, dtype, size in (("fs_tx_sock", TX_SOCK_DTYPE, 104), ("fs_tx_sock_out", TX_SOCK_OUT_DTYPE, 32)):
        fields = struct_fields(name)
        assert [re.sub(r"\[\d+\]", "", nm) for _, nm in fields] == list(dtype.names) and dtype.itemsize == size
        at = 0
        for ctype, nm in fields:
            count = int(m.group(1)) if (m := re.search(r"\[(\d+)\]", nm)) else 1
            width = int(ctype[4:-2]) // 8
            assert dtype.fields[re.sub(r"\[\d+\]", "", nm)][1] == at, nm
            at += width * count
        assert at == size
    defines = dict(re.findall(r"#define (FS_\w+) (\w+)u", HEADER))
    assert abi.SEND_MAX_SOCKS == int(defines["FS_SEND_MAX_SOCKS"]) and abi.SEND_NONE == int(defines["FS_SEND_NONE"], 16)
    assert (abi.TX_ACK, abi.TX_FIN, abi.TX_PSH) == tuple(int(defines[k]) for k in ("FS_TX_ACK", "FS_TX_FIN", "FS_TX_PSH"))
    assert (ref.TX_ACK, ref.TX_FIN, ref.TX_PSH, ref.NONE) == (abi.TX_ACK, abi.TX_FIN, abi.TX_PSH, abi.SEND_NONE)


# ---- the rule of the loaded library, and the reference's frames ---------------------------------------

@pytest.fixture(scope="module")
def batches():
    return list(cases.oracle_cases()) + [cases.rejected_frames()]


def test_layout_is_the_references_rule(batches):
    for socks, rings in batches:
        frames, outs = ref.frames_of(socks, rings)
        for flags, align in ((0, 1), (ref.FCS_APPEND, 1), (0, 64), (ref.FCS_APPEND, 4096)):
            n, nbytes, got = send_rings_layout(ref.socks_of(socks), flags, align)
            assert n == len(frames) and nbytes == sref.layout([len(f) for f in frames], flags, align)[1]
            assert got.dtype == TX_SOCK_OUT_DTYPE and np.array_equal(got, outs), np.flatnonzero(got != outs)[:5]


def test_reference_frames_pass_the_oracle():
    for socks, rings in cases.oracle_cases():
        frames, _ = ref.frames_of(socks, rings)
        big = sum(len(f) + 4 for f in frames) + 64
        buf, off, ln, dig, st, _ = ref.expected(socks, rings, 0, ref.FCS_APPEND, 1, np.zeros(big, dtype=np.uint8))
        assert ln.size == len(frames) > 0 and (st == 0).all()
        # ... as received frames: checksums and FCS verify, and each carries the state the rule names
        _, st2 = coracle.digest_fcs_batch(buf, off, ln + np.uint32(4), 0)
        assert (st2 == 0).all()
        f = 0
        for s in socks:
            r = ref.rule(s)
            for k in range(r["S"]):
                fr = buf[int(off[f]) : int(off[f]) + int(ln[f])].tobytes()
                assert int.from_bytes(fr[38:42], "big") == (s["snd_nxt"] + k * s["mss"]) & ref.M32
                assert int.from_bytes(fr[42:46], "big") == s["rcv_nxt"] and fr[47] & 0x10
                assert bool(fr[47] & 0x01) == (r["fin"] and k == r["S"] - 1) and len(fr) - 54 <= s["mss"]
                f += 1
        assert f == len(frames)


def test_derived_sends_make_the_references_frames():
    # what tests/test_gpu_send_rings.py hands to fs_segment_batch for the same bytes
    for socks, rings in cases.both_entry_point_cases():
        specs, payload = ref.segment_sends(socks, rings)
        frames, outs = ref.frames_of(socks, rings)
        assert len(specs) == int((outs["n_frames"] > 0).sum()) > 0 and payload.size == int(outs["bytes"].sum())
        pb = payload.tobytes()
        mine = [f for hdr, off, ln, mss in specs for f in sref.send_frames(hdr, pb[off : off + ln], mss)]
        assert mine == frames and len(frames) >= 10
        for flags, align in ((ref.FCS_APPEND, 1), (0, 64)):
            noise = np.random.default_rng(5).integers(0, 256, sref.layout([len(f) for f in frames], flags, align)[1] + 64,
                                                      dtype=np.uint8)
            a, b = sref.expected(specs, payload, 0, flags, align, noise), ref.expected(socks, rings, 0, flags, align, noise)
            assert all(np.array_equal(x, y) for x, y in zip(a, b[:5]))
        sends = sref.make_sends(specs)
        assert np.array_equal(sends["mss"], [s["mss"] for s in socks if ref.rule(s)["S"]]) and (sends["hdr"][:, 23] == 6).all()


def test_hand_computed_socket():
    # ring "0123456789abcdef" read from 'c': 10 bytes in frames of 4 -> "cdef" "0123" "45"
    rings = np.frombuffer(b"..0123456789abcdef", dtype=np.uint8)
    rng = np.random.default_rng(1)
    s = ref.sock(sref.tcp_header(rng, ident=1), 4, 2, 16, 12, 11, snd_una=90, snd_nxt=100, snd_wnd=20, rcv_nxt=7,
                 rcv_wnd=70000, flags=ref.TX_FIN | ref.TX_PSH)
    frames, outs = ref.frames_of([s], rings)
    assert [f[54:] for f in frames] == [b"cdef", b"0123", b"45"]
    assert [int.from_bytes(f[38:42], "big") for f in frames] == [100, 104, 108]
    assert [f[47] for f in frames] == [0x10, 0x10, 0x18] and frames[0][48:50] == b"\xff\xff"  # the FIN waits for byte 11
    assert [int.from_bytes(f[18:20], "big") for f in frames] == [1, 0x8181, sref.prand16(0x8181)]
    assert [int(outs[0][k]) for k in outs.dtype.names] == [110, 6, 1, 10, 3, 0, sref.prand16(sref.prand16(0x8181)), 0]
    n, nbytes, got = send_rings_layout(ref.socks_of([s]), 0, 8)
    assert (n, nbytes) == (3, 64 + 64 + 56) and np.array_equal(got, outs)


# ---- FS_E_INVALID ---------------------------------------------------------------------------------------

def good(**kw):
    return ref.sock(sref.tcp_header(np.random.default_rng(3)), 100, 0, 4096, 0, 10, **kw)


def edit_hdr(at, value):
    s = good()
    h = bytearray(s["hdr"])
    h[at] = value
    return dict(s, hdr=bytes(h))


INVALID = {
    "EtherType": edit_hdr(13, 0x06),
    "IHL": edit_hdr(14, 0x46),
    "protocol 17": edit_hdr(23, 17),
    "protocol 1": edit_hdr(23, 1),
    "data offset": edit_hdr(46, 0x60),
    "mss 0": dict(good(), mss=0),
    "mss above 65495": dict(good(), mss=65496),
    "unknown flags": dict(good(), flags=8),
    "max_frames": dict(good(), max_frames=4097),
    "ring_size 0": dict(good(), ring_size=0, ring_buffered=0),
    "ring_size above 2^31": dict(good(), ring_size=(1 << 31) + 1),
    "ring_rpos": dict(good(), ring_rpos=4096),
    "ring_buffered": dict(good(), ring_buffered=4097),
}


def test_layout_accepts_the_boundaries():
    for s in (good(), dict(good(), mss=65495), dict(good(), flags=7), dict(good(), max_frames=4096),
              dict(good(), ring_size=1 << 31), dict(good(), ring_rpos=4095, ring_buffered=4096),
              dict(good(), ring_off=(1 << 64) - 4096)):  # (the layout call has no rings_bytes to bound it with)
        send_rings_layout(ref.socks_of([s]))
    assert send_rings_layout(ref.socks_of([]))[:2] == (0, 0)


@pytest.mark.parametrize("what", list(INVALID))
def test_invalid_sockets_are_rejected_without_a_device(what):
    socks = ref.socks_of([good(), INVALID[what], good()])
    with pytest.raises(FramesumError, match=r"\(-1\): fs_send_rings_layout: socket 1: "):
        send_rings_layout(socks)


def test_invalid_calls_are_rejected_without_a_device():
    lib = framesum.load_library()
    socks = ref.socks_of([good()])
    p = socks.ctypes.data_as(ctypes.c_void_p)
    n, b = ctypes.c_uint64(), ctypes.c_uint64()
    ok = lambda *a: lib.fs_send_rings_layout(*a, ctypes.byref(n), ctypes.byref(b), None)  # noqa: E731
    assert ok(p, 1, 0, 1) == 0 and (n.value, b.value) == (1, 64)
    assert ok(p, 1, 4, 1) == -1 and ok(p, 1, 1, 1) == -1          # flags other than FS_FCS_APPEND
    assert ok(p, 1, 0, 3) == -1 and ok(p, 1, 0, 0) == -1 and ok(p, 1, 0, 8192) == -1
    assert ok(None, 1, 0, 1) == -1 and ok(None, 0, 0, 1) == 0
    many = np.zeros(abi.SEND_MAX_SOCKS + 1, dtype=TX_SOCK_DTYPE)
    many[:] = socks[0]
    mp = many.ctypes.data_as(ctypes.c_void_p)
    assert ok(mp, abi.SEND_MAX_SOCKS + 1, 0, 1) == -1 and b"FS_SEND_MAX_SOCKS" in lib.fs_last_error(None)
    assert ok(mp, abi.SEND_MAX_SOCKS, 0, 1) == 0 and n.value == abi.SEND_MAX_SOCKS
    # a null context: before anything else
    some = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(4096)))
    assert lib.fs_send_rings_batch(None, p, 1, some, 4096, 0, 0, 1, some, 4096, None, None, None, None, None, None) == -1
    assert lib.fs_send_rings_batch_host(None, p, 1, some, 4096, 0, 0, 1, some, 4096, None, None, None, None, None) == -1


# ---- the binding -------------------------------------------------------------------------------------------

def test_tx_sock_from_a_delivery():
    outs = np.zeros(2, dtype=SOCK_OUT_DTYPE)
    outs["rcv_nxt"], outs["ring_free"], outs["ring_wpos"] = [5000, 0xFFFFFFFF], [300, 70000], [9, 9]
    tx = ref.socks_of([good(snd_nxt=11), good(snd_nxt=12)])
    got = tx_sock_from(outs, tx, flags=abi.TX_ACK)
    assert got.dtype == TX_SOCK_DTYPE and got is not tx and int(tx["rcv_nxt"][0]) == 0
    assert list(got["rcv_nxt"]) == [5000, 0xFFFFFFFF] and list(got["rcv_wnd"]) == [300, 70000]
    assert list(got["flags"]) == [1, 1] and list(got["snd_nxt"]) == [11, 12] and np.array_equal(got["hdr"], tx["hdr"])
    one = tx_sock_from(outs[1], mss=7)
    assert one.shape == (1,) and int(one["rcv_wnd"][0]) == 70000 and int(one["mss"][0]) == 7
    with pytest.raises(AssertionError):
        tx_sock_from(outs, tx[:1])


class StandInFunction:
    def __init__(self, lib, name):
        self.lib, self.name, self.restype, self.argtypes = lib, name, None, None

    def __call__(self, *args):
        self.lib.calls.append((self.name, args))
        if self.name == "fs_last_error":
            return b"the stand-in says no"
        if self.name in self.lib.fail:
            return self.lib.fail[self.name]
        if self.name == "fs_ctx_create":
            args[1]._obj.value = 0x5000
        elif self.name == "fs_send_rings_layout":
            args[4]._obj.value, args[5]._obj.value = 3, 200
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


def stand_in(monkeypatch, tmp_path, cls):
    product = tmp_path / "libframesum.so"
    product.write_bytes(b"")
    monkeypatch.setattr(ctypes, "CDLL", cls)
    monkeypatch.setattr(abi, "_LIB_PATH", str(product))
    monkeypatch.setattr(abi, "_lib", None)
    monkeypatch.setattr(abi, "_libs", {})


def plain(a):
    return getattr(a, "value", a)


def test_send_rings_host_marshals(monkeypatch, tmp_path):
    stand_in(monkeypatch, tmp_path, StandInLibrary)
    eng = Engine(0)
    for name, (restype, argtypes) in abi.SEND_RINGS_PROTOTYPES.items():  # the loader set the third table too
        assert getattr(eng.lib, name).restype is restype and getattr(eng.lib, name).argtypes == argtypes
    eng.lib.calls.clear()
    socks = np.zeros(2, dtype=TX_SOCK_DTYPE)
    rings = np.zeros(500, dtype=np.uint8)
    frames, off, ln, dig, st, outs = eng.send_rings_host(socks, rings, 1500, 2, 8)
    (lname, largs), (name, args) = eng.lib.calls
    assert lname == "fs_send_rings_layout" and [plain(a) for a in largs[:4]] == [socks.ctypes.data, 2, 2, 8]
    want = [eng._ctx.value, socks, 2, rings, 500, 1500, 2, 8, frames, 200, off, ln, dig, st, outs]
    assert name == "fs_send_rings_batch_host" and len(args) == len(want) == 15
    for k, (a, w) in enumerate(zip(args, want)):
        assert plain(a) == (w.ctypes.data if isinstance(w, np.ndarray) else w), f"argument {k}"
    assert frames.shape == (200,) and off.dtype == np.uint64 and ln.dtype == np.uint32 and dig.dtype == DIGEST_DTYPE
    assert off.shape == ln.shape == dig.shape == st.shape == (3,) and st.dtype == np.uint8
    assert outs.dtype == TX_SOCK_OUT_DTYPE and outs.shape == (2,)
    frozen = np.zeros(200, dtype=np.uint8)
    frozen.flags.writeable = False
    with pytest.raises(AssertionError):
        eng.send_rings_host(socks, rings, frames=frozen)
    eng.lib.fail["fs_send_rings_batch_host"] = -1
    with pytest.raises(FramesumError) as err:
        eng.send_rings_host(socks, rings)
    assert str(err.value) == "fs_send_rings_batch_host failed (-1): the stand-in says no"
    eng.close()


def test_a_library_without_the_symbol_raises(monkeypatch, tmp_path):
    class Older(StandInLibrary):
        def __getattr__(self, name):
            if name == "fs_send_rings_batch":
                raise AttributeError(name)
            return super().__getattr__(name)

    stand_in(monkeypatch, tmp_path, Older)
    with pytest.raises(AttributeError, match="fs_send_rings_batch"):
        framesum.load_library()
