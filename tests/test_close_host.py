"""The close call (fs_close_flows_batch / fs_close_flows_batch_host) without a GPU: the agreement of the two
restatements of tests/close_ref.py over a grid of one-frame cases, except on the differences the header
states, each of which the grid is shown to reach; the derivation of rule 5 against the literal window
checks; the arithmetic of seqs_amd/csrc/framesum_close.h under ASan + UBSan (a stand-alone program run as a
child process, which also goes through every rejection of the closer list); the sixth header against the
binding's table, record layouts and constants; the entry points' null-context path; what the Python methods
hand to the C ABI; closers_from and state_after_send."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 (before the stand-in replaces ctypes.CDLL: torch loads its own libraries through it)

from seqs_amd import abi, framesum
from seqs_amd.framesum import CLOSE_OUT_DTYPE, CLOSER_DTYPE, SOCK_DTYPE

import accept_cases as acases
import accept_ref
import close_ref as ref
import recv_ref
from test_deliver_host import SAN, plain
from test_recv_host import RecvStandIn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tests", "csrc")
HEADER = open(os.path.join(ROOT, "include", "framesum_close.h")).read()
BODY = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
ACCEPT_BODY = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "framesum_accept.h")).read(), flags=re.S)
TEXT = " ".join(HEADER.replace("*", " ").split())
M32 = ref.M32
FIN, SYN, RST, ACK = ref.FIN, ref.SYN, ref.RST, ref.ACK


# ---- the two restatements agree --------------------------------------------------------------------------

STATES = (4, 5, 6, 7, 8, 9, 10)
FLAGS = [f | s | r | a for f in (0, FIN) for s in (0, SYN) for r in (0, RST) for a in (0, ACK)]
# the sequence numbers cross 2^32: nxt - 1 = 2^32 - 1, snd_nxt + 1 = 0
BASES = ((0, M32 - 1), (M32 - 1, 5000), (1000, 0))
# the differences include/framesum_close.h names, and what the grid leaves to another call
NAMED = {"data": "(a) data in a closing state", "closed numbers": "(b) the numbers of a Closed record",
         "syn": "(c) a frame with SYN ends the walk"}
SCOPE = "Every other frame of an Established socket is the receive call's"


def go_outcome(state, nxt, una, snd_nxt, rcv_wnd, seg):
    tcb = ref.GoTCB(state, una, snd_nxt, 77, nxt, rcv_wnd)
    err = ref.go_recv(tcb, recv_ref.Segment(*seg))
    return err, tcb


@pytest.mark.parametrize("nxt, snd_nxt", BASES)
def test_the_two_restatements_agree_on_one_frame(nxt, snd_nxt):
    una = (snd_nxt - 7) % M32
    seen = dict(agree=0, data=0, closed_numbers=0, syn=0, scope=0)
    reached = set()
    go_alone = 0  # cases in which the reference changes a connection and the contract's words do not cover why
    for state, flags9, length, ds, da, rcv_wnd in itertools.product(STATES, FLAGS, (0, 1), (-1, 0, 1), (-1, 0, 1, "una"),
                                                                    (0, 1, 65535)):
        seq = (nxt + ds) % M32
        ack = una if da == "una" else (snd_nxt + da) % M32
        seg = (seq, ack, 4321, flags9, length)
        err, tcb = go_outcome(state, nxt, una, snd_nxt, rcv_wnd, seg)
        go_changed = (tcb.state, tcb.rcv_NXT, tcb.snd_UNA, tcb.snd_WND) != (state, nxt, una, 77)
        if state == 4 and (not flags9 & RST or flags9 & SYN):
            seen["scope"] += 1  # the receive call's frames (include/framesum_recv.h), not this call's
            continue
        c = ref.Ctl(state, nxt, una, 77)
        code = ref.code_of(state, nxt, snd_nxt, rcv_wnd, seg)
        if code == ref.ENDS:
            # difference (c): left to the host, whatever the reference makes of it
            assert flags9 & SYN and state not in (ref.TIME_WAIT, ref.CLOSED)
            seen["syn"] += 1
            continue
        ref.step(c, code, snd_nxt, seg)
        mine = (c.state, c.nxt, c.una, c.wnd)
        if code == ref.DATA:
            # difference (a): a frame with data changes nothing here
            assert length > 0 and mine == (state, nxt, una, 77) and c.flags == 0
            seen["data"] += 1
            reached.add("data:changed" if go_changed else "data:refused")
            continue
        if code == ref.TAKEN and c.state == ref.CLOSED:
            # difference (b): LastAck's ACK. The reference closes and then goes on to control_user.go:212-217
            assert state == ref.LAST_ACK and flags9 & ACK and err is None and tcb.state == ref.CLOSED
            assert (tcb.snd_WND, tcb.snd_UNA, tcb.rcv_NXT) == (4321, ack, 1 if flags9 & FIN else 0)
            assert c.record(0)[1:4] == (0, 0, 0)
            seen["closed_numbers"] += 1
            continue
        # everywhere else: the same connection behind the frame, the same verdict, the same pending ACK
        theirs = (tcb.state, tcb.rcv_NXT, tcb.snd_UNA, tcb.snd_WND)
        if code == ref.RESET_CODE:
            assert err == "ErrClosed" and tcb.state == ref.CLOSED and c.record(0)[:4] == (0, 0, 0, 0) == theirs
            assert not tcb.challengeAck and c.flags == ref.RESET
        else:
            assert mine == theirs, (state, seg, rcv_wnd, code, err)
            assert (code == ref.TAKEN) == (err is None)
            assert (code == ref.IGNORED) == (err == "EOF:closed") and (code == ref.KEEPALIVE) == (err == "keepalive")
            if code == ref.EXPECTED:
                assert err in ("errFinwaitExpectedACK", "errFinwaitExpectedFinack")
            if code == ref.REJECTED:
                assert err in ("errSeqNotInWindow", "errLastNotInWindow", "errRequireSequential") and ds != 0
                assert not tcb.challengeAck  # an RST with another Seq owes nothing
            assert bool(c.flags & ref.ACK_OWED) == bool(tcb.pending[0] & ACK)
            assert bool(c.flags & ref.FIN_TAKEN) == (err is None and bool(flags9 & FIN))
            if not (code == ref.TAKEN) and go_changed:
                go_alone += 1
        seen["agree"] += 1
        reached.add((state, code, c.state))
    # every stated difference is reached, in both of (a)'s forms; nothing else is left out; and outside the
    # named classes the reference never moves a connection the contract leaves alone
    assert seen["data"] and seen["closed_numbers"] and seen["syn"] and {"data:changed", "data:refused"} <= reached
    total = len(STATES) * len(FLAGS) * 2 * 3 * 4 * 3
    assert sum(seen.values()) == total and go_alone == 0
    assert seen["scope"] == 12 * 2 * 3 * 4 * 3                   # state 4: the 12 flag sets without RST or with SYN
    # rule 1 comes before rule 2, so TimeWait's SYNs are code 8: the SYN class is states 5, 6, 7, 9 and 10
    assert seen["syn"] == 5 * 8 * 2 * 3 * 4 * 3


def test_every_transition_and_code_is_reached():
    """The grid above reaches each code and each transition of the header's table."""
    reached = set()
    for nxt, snd_nxt in BASES[:1]:
        una = (snd_nxt - 7) % M32
        for state, flags9, length, ds, da in itertools.product(STATES, FLAGS, (0, 1), (-1, 0, 1), (-1, 0, 1)):
            if state == 4 and (not flags9 & RST or flags9 & SYN):
                continue
            seg = ((nxt + ds) % M32, (snd_nxt + da) % M32, 1, flags9, length)
            code = ref.code_of(state, nxt, snd_nxt, 65535, seg)
            c = ref.Ctl(state, nxt, una, 77)
            if code != ref.ENDS:
                ref.step(c, code, snd_nxt, seg)
            reached.add((state, code, c.state))
    codes = {r[1] for r in reached}
    assert codes == {1, 4, 5, 7, 8, 9, 10, ref.ENDS}
    for edge in ((5, 1, 8), (5, 1, 7), (5, 1, 6), (5, 10, 5), (6, 1, 8), (6, 10, 6), (7, 1, 8), (7, 1, 7), (9, 1, 9), (10, 1, 0),
                 (10, 1, 10), (4, 9, 0), (4, 4, 4), (4, 7, 4), (5, 9, 0), (9, 9, 0), (8, 8, 8)):
        assert edge in reached, edge


def test_the_header_names_the_differences_the_grid_leaves_out():
    for words in NAMED.values():
        assert words in TEXT, words
    assert SCOPE in TEXT
    for words in ("(d) the failed RST of an Established socket ends that socket's walk", "A closer has no ring",
                  "errRequireSequential (:308-311) comes first", "never writes a ring byte",
                  "a frame without data passes iff Seq == nxt", "The accept stage does not know the list of closers"):
        assert words in TEXT, words


# ---- rule 5 ------------------------------------------------------------------------------------------------

def literal_seq_checks(seq, nxt, rcv_wnd, fin):
    """control.go:299-311 for DATALEN 0, case by case, with the reference's own helpers."""
    seg = recv_ref.Segment(seq, 0, 0, FIN if fin else 0, 0)
    zeroWindowOK = rcv_wnd == 0 and seg.DATALEN == 0 and seg.SEQ == nxt
    if rcv_wnd == 0 and seg.DATALEN > 0 and seg.SEQ == nxt:
        return "errZeroWindow"
    if not recv_ref.go_in_window(seg.SEQ, nxt, rcv_wnd) and not zeroWindowOK:
        return "errSeqNotInWindow"
    if not recv_ref.go_in_window(seg.Last(), nxt, rcv_wnd) and not zeroWindowOK:
        return "errLastNotInWindow"
    if seg.SEQ != nxt:
        return "errRequireSequential"
    return None


def test_rule5_is_seq_equals_nxt():
    hits = set()
    for nxt in (0, 1, 1000, (1 << 31) - 1, 1 << 31, M32 - 1):
        for rcv_wnd in (0, 1, 2, 65535, 65536, 1 << 31, M32 - 1):
            for d in (-65536, -2, -1, 0, 1, 2, 65534, 65535, 65536, 1 << 31):
                for fin in (False, True):
                    err = literal_seq_checks((nxt + d) % M32, nxt, rcv_wnd, fin)
                    assert (err is None) == (d == 0), (nxt, rcv_wnd, d, fin)
                    hits.add(err)
                    if d == 0 and rcv_wnd == 0 and fin:
                        assert err is None  # the bare FIN at a zero window: zeroWindowOK covers it
    # :305 never fires alone (Last == Seq), :299 never fires (no data)
    assert hits == {None, "errSeqNotInWindow", "errRequireSequential"}


# ---- the stand-alone sanitizer build -----------------------------------------------------------------------

def test_close_arithmetic_under_asan_ubsan():
    out = os.path.join(CSRC, "build", "test_close")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *SAN, "-o", out, os.path.join(CSRC, "test_close.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "close checks OK" in r.stdout


# ---- the sixth header and the binding's tables -------------------------------------------------------------

def params_of(body, name):
    p = body[body.index(name + "(") + len(name) + 1 :]
    return [" ".join(x.split()) for x in p[: p.index(")")].split(",")]


NEW_PARAMS = ["const fs_cl_sock* closers", "uint32_t n_closers", "fs_cl_out* closers_out", "fs_cl_out* socks_close",
              "uint8_t* ctl_code"]


def test_close_prototypes_are_the_headers():
    names = ["fs_close_flows_batch", "fs_close_flows_batch_host"]
    assert re.findall(r"^fs_status\s+(fs_\w+)\s*\(", BODY, flags=re.M) == list(abi.CLOSE_PROTOTYPES) == names
    others = (set(abi.PROTOTYPES) | set(abi.DELIVER_PROTOTYPES) | set(abi.SEND_RINGS_PROTOTYPES) | set(abi.RECV_PROTOTYPES) |
              set(abi.ACCEPT_PROTOTYPES))
    assert not set(abi.CLOSE_PROTOTYPES) & others and '#include "framesum_accept.h"' in HEADER
    for name, (restype, argtypes) in abi.CLOSE_PROTOTYPES.items():
        params = params_of(BODY, name)
        assert restype is ctypes.c_int32 and len(params) == len(argtypes) == 42, name
        for p, t in zip(params, argtypes):
            want = ctypes.c_void_p if "*" in p else {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}[p.split()[0]]
            assert t is want, (name, p)
        # every parameter of the accept call up to and including `synack_status`, the five new ones, the rest
        theirs = params_of(ACCEPT_BODY, name.replace("close", "accept"))
        at = theirs.index("uint8_t* synack_status") + 1
        assert params == theirs[:at] + NEW_PARAMS + theirs[at:]
    lib = framesum.load_library()
    for name, (restype, argtypes) in abi.CLOSE_PROTOTYPES.items():
        assert getattr(lib, name).restype is restype and getattr(lib, name).argtypes == argtypes


C_TYPES = {"uint8_t": ("u1", 1), "uint16_t": ("<u2", 2), "uint32_t": ("<u4", 4)}


def test_close_dtypes_and_constants_are_the_headers():
    for name, dtype, size in (("fs_cl_sock", CLOSER_DTYPE, 40), ("fs_cl_out", CLOSE_OUT_DTYPE, 32)):
        body = BODY[BODY.index("typedef struct " + name + " {") : BODY.index("} " + name + ";")]
        at, fields = 0, []
        for ctype, decl in re.findall(r"(uint8_t|uint16_t|uint32_t)\s+([^;]+);", body):
            for item in decl.split(","):
                m = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", item)
                count = int(m.group(2) or 1)
                fields.append((m.group(1), at, C_TYPES[ctype][1] * count))
                assert at % C_TYPES[ctype][1] == 0, (name, m.group(1))  # no padding: every field naturally aligned
                at += C_TYPES[ctype][1] * count
        assert at == size == dtype.itemsize, name
        assert [(f, dtype.fields[f][1], dtype.fields[f][0].itemsize) for f in dtype.names] == fields, name
        assert f"{size} bytes" in HEADER[HEADER.index("typedef struct " + name + " {") :].split("\n")[0]
    defines = {k: int(v) for k, v in re.findall(r"#define (FS_\w+) (\d+)u", HEADER)}
    states = dict(CLOSED=0, ESTABLISHED=4, FIN_WAIT_1=5, FIN_WAIT_2=6, CLOSING=7, TIME_WAIT=8, CLOSE_WAIT=9, LAST_ACK=10)
    for k, v in states.items():
        assert defines["FS_ST_" + k] == getattr(abi, "ST_" + k) == getattr(ref, k) == v
    codes = dict(TAKEN=1, REJECTED=4, KEEPALIVE=5, DATA=7, IGNORED=8, RST=9, EXPECTED=10)
    for k, v in codes.items():
        assert defines["FS_CL_" + k] == getattr(abi, "CLOSE_" + k) == v
    assert (ref.TAKEN, ref.REJECTED, ref.KEEPALIVE, ref.DATA, ref.IGNORED, ref.RESET_CODE, ref.EXPECTED) == tuple(codes.values())
    assert (defines["FS_CL_ACK_OWED"], defines["FS_CL_FIN"], defines["FS_CL_RESET"]) == (1, 2, 4)
    assert (abi.CLOSE_ACK_OWED, abi.CLOSE_FIN, abi.CLOSE_RESET) == (ref.ACK_OWED, ref.FIN_TAKEN, ref.RESET) == (1, 2, 4)
    assert defines["FS_CLOSE_MAX_CLOSERS"] == abi.CLOSE_MAX_CLOSERS == 65536
    # the receive call's codes 1, 4 and 5 keep their numbers
    assert (abi.CLOSE_TAKEN, abi.CLOSE_REJECTED, abi.CLOSE_KEEPALIVE) == (abi.RECV_TAKEN, abi.RECV_REJECTED, abi.RECV_KEEPALIVE)


def test_null_context_needs_no_device():
    lib = framesum.load_library()
    none = ctypes.c_void_p()
    some = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    tail = (some, 8, some, some, some, none, some, none, none)
    listen = (some, 1, some, 1, 0, some, some, none, some, none, none)
    closing = (some, 1, some, some, none)
    assert lib.fs_close_flows_batch(None, some, some, some, 1, 0, 0, some, 1, some, 64, some, none, some, some, none, *listen,
                                    *closing, *tail, none) == -1
    assert lib.fs_close_flows_batch_host(None, some, 64, some, some, 1, 0, 0, some, 1, some, 64, some, none, some, some, none,
                                         *listen, *closing, *tail) == -1


# ---- the binding: what the methods hand to the C ABI ---------------------------------------------------------

@pytest.fixture
def eng(monkeypatch, tmp_path):
    product = tmp_path / "libframesum.so"
    product.write_bytes(b"")
    monkeypatch.setattr(ctypes, "CDLL", RecvStandIn)
    monkeypatch.setattr(abi, "_LIB_PATH", str(product))
    monkeypatch.setattr(abi, "_lib", None)
    monkeypatch.setattr(abi, "_libs", {})
    e = framesum.Engine(0)
    for name, (restype, argtypes) in abi.CLOSE_PROTOTYPES.items():  # the loader set the sixth table too
        assert getattr(e.lib, name).restype is restype and getattr(e.lib, name).argtypes == argtypes
    e.lib.calls.clear()
    yield e
    e.close()


def test_close_flows_host_marshals(eng):
    lengths = np.array([60, 61, 1514], dtype=np.uint32)
    offsets = np.array([0, 60, 124], dtype=np.uint64)
    frames = np.arange(1640, dtype=np.uint32).astype(np.uint8)
    socks, snd = np.zeros(2, dtype=SOCK_DTYPE), recv_ref.snd_of((5, 100), (6, 200))
    rings = np.zeros(500, dtype=np.uint8)
    listeners = accept_ref.listeners_of((acases.local(80), acases.MAC, 0, 3))
    slots = acases.default_slots(3)
    closers = np.zeros(4, dtype=CLOSER_DTYPE)
    res = eng.close_flows_host(frames, offsets, lengths, socks, snd, rings, listeners, slots, closers, mtu=1500, flags=1,
                               synack_flags=2, payload=False)
    cout, sclose, ctl, conns, lout, of, synacks, syn_out, syn_st, snd_out, code, socks_out, delivered, payload = res[:14]
    (call,) = eng.lib.calls
    name, args = call
    want = [eng._ctx.value, frames, frames.nbytes, offsets, lengths, 3, 1500, 1, socks, 2, rings, 500, socks_out, delivered, snd,
            snd_out, code, listeners, 1, slots, 3, 2, conns, lout, of, synacks, syn_out, syn_st, closers, 4, cout, sclose, ctl,
            None, 0]
    assert name == "fs_close_flows_batch_host" and len(args) == 42 and payload is None
    for k, w in enumerate(want):
        assert plain(args[k]) == (w.ctypes.data if isinstance(w, np.ndarray) else w), f"argument {k}"
    assert cout.dtype == CLOSE_OUT_DTYPE and cout.shape == (4,) and sclose.dtype == CLOSE_OUT_DTYPE and sclose.shape == (2,)
    assert ctl.dtype == np.uint8 and ctl.shape == (3,)
    # ctl_code left out, and no closers: null pointers
    res = eng.close_flows_host(frames, offsets, lengths, socks, snd, rings, listeners, slots, np.zeros(0, dtype=CLOSER_DTYPE),
                               ctl_code=False, payload=False)
    args = eng.lib.calls[1][1]
    assert res[2] is None and [plain(args[k]) for k in (29, 30, 32)] == [0, None, None] and plain(args[31]) == res[1].ctypes.data
    # the accept call's own path is what it was
    eng.accept_flows_host(frames, offsets, lengths, socks, snd, rings, listeners, slots, payload=False)
    assert eng.lib.calls[2][0] == "fs_accept_flows_batch_host" and len(eng.lib.calls[2][1]) == 37


def test_closers_from_and_state_after_send():
    socks = np.zeros(4, dtype=SOCK_DTYPE)
    for i in range(4):
        socks["key"][i] = np.arange(13) + i
        socks["rcv_wnd"][i], socks["snd_nxt"][i], socks["rcv_nxt"][i] = 100 + i, 200 + i, 300 + i
    out = np.zeros(4, dtype=CLOSE_OUT_DTYPE)
    out["state"] = (4, 9, 0, 4)
    out["rcv_nxt"], out["snd_una"], out["snd_wnd"] = (1, 2, 0, 4), (5, 6, 0, 8), (9, 10, 0, 12)
    idx, closers = framesum.closers_from(socks, out)
    assert list(idx) == [1, 2] and closers.dtype == CLOSER_DTYPE
    assert bytes(closers["key"][0]) == bytes(socks["key"][1]) and int(closers["state"][0]) == 9
    assert (int(closers["rcv_nxt"][0]), int(closers["snd_una"][0]), int(closers["snd_wnd"][0])) == (2, 6, 10)
    assert (int(closers["rcv_wnd"][0]), int(closers["snd_nxt"][0])) == (101, 201) and int(closers["state"][1]) == 0
    # Send's transitions (control_user.go:118-137)
    FINF, ACKF = framesum.TX_FIN, framesum.TX_ACK
    table = {(4, FINF): 5, (9, FINF): 10, (7, ACKF): 8, (4, ACKF): 4, (9, ACKF): 9, (7, 0): 7, (5, FINF): 5, (6, ACKF): 6,
             (10, ACKF): 10, (8, ACKF): 8, (4, 0): 4, (9, FINF | ACKF): 10}
    for (state, sent), want in table.items():
        assert framesum.state_after_send(state, sent) == want, (state, sent)
