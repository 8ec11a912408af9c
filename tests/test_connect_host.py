"""The connect call (fs_connect_flows_batch / fs_connect_flows_batch_host) without a GPU: the agreement of
the two restatements of tests/connect_ref.py over a grid of one-frame cases, replies included, except on the
differences the header states, each of which the grid is shown to reach; rule 7 against the client model of
tests/handshake.py; the arithmetic of seqs_amd/csrc/framesum_connect.h under ASan + UBSan (a stand-alone
program run as a child process, which also goes through every rejection of the opener list); the seventh
header against the binding's table, record layouts and constants; the entry points' null-context path; what
the Python methods hand to the C ABI; socks_from_connect."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 (before the stand-in replaces ctypes.CDLL: torch loads its own libraries through it)

from seqs_amd import abi, framesum
from seqs_amd.framesum import CLOSER_DTYPE, CONNECT_OUT_DTYPE, OPENER_DTYPE, SOCK_DTYPE

import accept_cases as acases
import accept_ref
import connect_ref as ref
import conversation as conv
import handshake
import recv_cases as rcases
import recv_ref
from test_deliver_host import SAN, plain
from test_recv_host import RecvStandIn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tests", "csrc")
HEADER = open(os.path.join(ROOT, "include", "framesum_connect.h")).read()
BODY = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
CLOSE_BODY = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "framesum_close.h")).read(), flags=re.S)
TEXT = " ".join(HEADER.replace("*", " ").split())
M32 = ref.M32
FIN, SYN, RST, ACK, PSH = ref.FIN, ref.SYN, ref.RST, ref.ACK, recv_ref.PSH


# ---- the two restatements agree --------------------------------------------------------------------------

FLAGS = [s | a | r | f | p for s in (0, SYN) for a in (0, ACK) for r in (0, RST) for f in (0, FIN) for p in (0, PSH)]
ISSES = (1000, M32 - 1, (1 << 31) - 1)
WNDS = (0, 1, 1000, M32 - 1)
REFUSALS = ("errZeroWindow", "errSeqNotInWindow", "errLastNotInWindow", "errRequireSequential")
NAMED = {"rst": "(a) an RST", "syn": "(b) a SYN that carries data, or flag bits beside SYN and ACK",
         "after rule 5": "(c) the state after rule 5"}


def opener_of(iss, rcv_wnd, flags=0):
    key = bytes([6, 10, 0, 0, 9, 10, 0, 0, 1, 0x1F, 0x90, 0xC0, 0x01])
    return ref.openers_of((key, flags, b"\x02\x00\x00\x00\x00\x01", b"\x02\x00\x00\x00\x00\x02", iss, rcv_wnd, 0x4321))[0]


def go_state(tcb):
    return (tcb.state, tcb.rcv_IRS, tcb.rcv_NXT, tcb.snd_UNA, tcb.snd_NXT, tcb.snd_WND)


def go_reply(tcb, op):
    """The frame the block owes after Recv: PendingSegment, Send, CalculateHeaders."""
    seg, ok = tcb.PendingSegment(0)
    assert ok and tcb.Send(seg) is None
    return ref.go_headers(seg, op, int(op["ip_id"]))


@pytest.mark.parametrize("iss", ISSES)
def test_the_two_restatements_agree_on_one_frame(iss):
    seen = dict(agree=0, rst=0, syn=0)
    reached, codes = set(), set()
    total = 0
    for rcv_wnd in WNDS:
        op = opener_of(iss, rcv_wnd)
        sendable = rcv_wnd <= 0xFFFF  # (Send refuses a larger window, control.go:364; the contract clamps the field)
        seqs = sorted({0, 1, M32 - 1, (rcv_wnd - 1) % M32, rcv_wnd})
        acks = sorted({(iss + d) % M32 for d in (-1, 0, 1, 2, 1 + (1 << 31), 1 - (1 << 31), 1 << 31)})
        lens = sorted({0, 1, min(rcv_wnd, 65535), min(rcv_wnd + 1, 65535)})  # (what a frame can carry)
        for flags9, seq, ack, length in itertools.product(FLAGS, seqs, acks, lens):
            total += 1
            seg = (seq, ack, 4321, flags9, length)
            tcb = ref.go_dial(iss, rcv_wnd)
            before = go_state(tcb)
            err = ref.go_recv(tcb, recv_ref.Segment(*seg))
            r = ref.Rec(iss)
            got = ref.walk(r, rcv_wnd, [seg], 40, [7], lambda k: 0)
            code = got[0] if got else ref.code_of(iss, rcv_wnd, seg)
            codes.add(code)
            if code == ref.ENDS_RST:
                # difference (a): the reference makes a listener of the block, or owes a challenge ACK
                assert flags9 & RST and r.stop == 40 and r.flags == ref.STOP_RST and r.reply == 0 and r.state == 3
                assert err == "errDropSegment" and (tcb.became_listener != tcb.challengeAck)
                reached.add("rst:listener" if tcb.became_listener else "rst:challenge")
                seen["rst"] += 1
                continue
            if code == ref.ENDS_SYN:
                # difference (b): no ring exists yet
                assert flags9 & SYN and not flags9 & RST and (length > 0 or flags9 & (FIN | PSH))
                assert r.stop == 40 and r.flags == ref.STOP_SYN and r.reply == 0 and r.state == 3
                reached.add("syn:taken" if err is None else "syn:refused")
                seen["syn"] += 1
                continue
            assert r.stop == 41 and r.flags == 0
            mine = (r.state, r.irs, r.rcv_nxt, r.snd_una, r.snd_nxt, r.snd_wnd)
            if code == ref.KEEPALIVE:
                assert err == "keepalive" and (r.n_keepalive, r.n_rejected) == (1, 0)
            elif code == ref.REJECTED:
                assert err in REFUSALS and not flags9 & SYN and (r.n_keepalive, r.n_rejected) == (0, 1)
                reached.add(err)
            elif code == ref.EXPECTED:
                assert err == "errExpectedSYN" and (r.n_keepalive, r.n_rejected) == (0, 1)
            if code in (ref.KEEPALIVE, ref.REJECTED, ref.EXPECTED):
                assert go_state(tcb) == before == mine and tcb.pending == [0, 0] and r.reply == 0 and r.frame == ref.NONE
            elif code == ref.BAD_ACK:
                assert err == "errDropSegment" and tcb.pending[0] == RST and tcb.rstPtr == ack == r.rst_seq
                assert go_state(tcb) == mine == (3, 0, 0, iss, iss, 4321) and r.reply == ref.REPLY_RST and r.frame == 7
                if sendable:
                    assert go_reply(tcb, op) == ref.reply_header(op, r)
                reached.add("bad ack: old" if not recv_ref.go_less_than(iss, ack) else "bad ack: unsent")
            else:
                assert code == ref.TAKEN and err is None and go_state(tcb) == mine and r.frame == 7
                assert r.state == (4 if flags9 & ACK else 2) and r.irs == seq and r.rcv_nxt == (seq + 1) % M32
                assert r.reply == (ref.REPLY_ACK if flags9 & ACK else ref.REPLY_SYNACK)
                if sendable:
                    assert go_reply(tcb, op) == ref.reply_header(op, r)
                    assert tcb.snd_NXT == (iss + 1) % M32 and tcb.pending == [0, 0]
                reached.add(("taken", r.state))
            seen["agree"] += 1
    assert sum(seen.values()) == total
    assert codes == {1, 4, 5, 10, 11, ref.ENDS_RST, ref.ENDS_SYN}
    assert {"rst:listener", "rst:challenge", "syn:taken", "syn:refused", "bad ack: old", "bad ack: unsent", ("taken", 4),
            ("taken", 2)} <= reached
    assert {"errZeroWindow", "errSeqNotInWindow", "errLastNotInWindow", "errRequireSequential"} <= reached


def test_difference_c_is_reached_and_the_first_syn_is_synsentSegments():
    """After rule 5 the reference's block has snd.NXT = iss, so it refuses the right SYN-ACK too; the
    contract's opener, listed again with the same iss, takes it."""
    iss, op = 5000, opener_of(5000, 4096, ref.SEND_SYN)
    tcb = ref.go_dial(iss, 4096)
    assert ref.go_recv(tcb, recv_ref.Segment(0, iss + 2, 100, ACK, 0)) == "errDropSegment" and tcb.snd_NXT == iss
    good = (77, iss + 1, 900, SYN | ACK, 0)
    assert ref.go_recv(tcb, recv_ref.Segment(*good)) == "errDropSegment" and tcb.state == 3  # acksUnsentData
    r = ref.Rec(iss)
    assert ref.walk(r, 4096, [good], 0, [0], lambda k: 1460) == [1] and r.state == 4 and r.peer_mss == 1460
    # the SYN of a flagged opener without a reply is handleInitSyn's frame
    fresh = ref.go_dial(iss, 4096)
    r = ref.Rec(iss)
    r.reply = ref.REPLY_SYN
    assert ref.go_headers(fresh.synsentSegment(), op, int(op["ip_id"])) == ref.reply_header(op, r)


def test_the_header_names_the_differences_the_grid_leaves_out():
    for words in NAMED.values():
        assert words in TEXT, words
    for words in ("So a frame passes iff Seq == 0 and (len == 0, or rcv_wnd > 0 and len + FIN - 1 < rcv_wnd)",
                  "only iss + 1 passes", "The accept stage does not know the openers", "With n_openers == 0 no launch is added",
                  "no byte of an opener with reply 0 is written", "the ctl_code entries of frames in an opener's flow are 0"):
        assert words in TEXT, words


def test_rule2_literal_cases_are_the_one_line_form():
    hits = set()
    for rcv_wnd in (0, 1, 2, 1000, 65535, 65536, 1 << 31, M32 - 1):
        for seq in sorted({0, 1, 2, 999, 1000, M32 - 1, (rcv_wnd - 1) % M32, rcv_wnd}):
            for length in (0, 1, 2, 999, 1000, 1001, 65535):
                for fin in (0, FIN):
                    tcb = ref.go_dial(9, rcv_wnd)
                    err = tcb.validateIncomingSegment(recv_ref.Segment(seq, 0, 0, fin, length))
                    assert (err is None) == ref.seq_passes(seq, fin, length, rcv_wnd), (rcv_wnd, seq, length, fin, err)
                    hits.add(err)
    assert hits == {None, *REFUSALS}


def test_rule5_only_iss_plus_1_passes():
    for iss in (0, 1, 1000, (1 << 31) - 1, 1 << 31, M32 - 2, M32 - 1):
        for d in (0, 1, 2, 3, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 31) + 2, M32 - 2, M32 - 1):
            ack = (iss + d) % M32
            old = not recv_ref.go_less_than(iss, ack)
            unsent = not recv_ref.go_less_than_eq(ack, (iss + 1) % M32)
            assert (old or unsent) == (d != 1) and old == (d == 0 or d > 1 << 31) and unsent == (2 <= d <= 1 << 31)
            assert (ref.code_of(iss, 100, (0, ack, 0, SYN | ACK, 0)) == ref.BAD_ACK) == (d != 1)


def test_rule7_is_the_handshake_clients_take_synack():
    rng = np.random.default_rng(41)
    for k in range(6):
        c = handshake.Client(rng, k, b"")
        seq, window = (M32 - 1, 0) if k == 1 else (int(rng.integers(0, M32)), int(rng.integers(0, 65536)))
        fr = rcases.frame(conv.mirrored(bytes(c.hdr)), seq, (c.iss + 1) % M32, SYN | ACK, window, options=b"\x02\x04\x05\xb4")
        r = ref.Rec(c.iss)
        assert ref.walk(r, c.rcv_wnd, [recv_ref.fields(fr)], 0, [0], lambda _: accept_ref.peer_mss(fr[54:58])) == [1]
        c.take_synack(fr)
        assert c.state == "Established" and r.state == 4 and r.peer_mss == 1460
        assert (c.rcv_nxt, c.snd_una, c.snd_nxt, c.snd_wnd) == (r.rcv_nxt, r.snd_una, r.snd_nxt, r.snd_wnd)


# ---- the stand-alone sanitizer build -----------------------------------------------------------------------

def test_connect_arithmetic_under_asan_ubsan():
    out = os.path.join(CSRC, "build", "test_connect")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *SAN, "-o", out, os.path.join(CSRC, "test_connect.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "connect checks OK" in r.stdout


# ---- the seventh header and the binding's tables -----------------------------------------------------------

def params_of(body, name):
    p = body[body.index(name + "(") + len(name) + 1 :]
    return [" ".join(x.split()) for x in p[: p.index(")")].split(",")]


NEW_PARAMS = ["const fs_cn_sock* openers", "uint32_t n_openers", "uint32_t reply_flags", "fs_cn_out* openers_out",
              "uint8_t* replies", "fs_digest* reply_out", "uint8_t* reply_status"]


def test_connect_prototypes_are_the_headers():
    names = ["fs_connect_flows_batch", "fs_connect_flows_batch_host"]
    assert re.findall(r"^fs_status\s+(fs_\w+)\s*\(", BODY, flags=re.M) == list(abi.CONNECT_PROTOTYPES) == names
    others = (set(abi.PROTOTYPES) | set(abi.DELIVER_PROTOTYPES) | set(abi.SEND_RINGS_PROTOTYPES) | set(abi.RECV_PROTOTYPES) |
              set(abi.ACCEPT_PROTOTYPES) | set(abi.CLOSE_PROTOTYPES))
    assert not set(abi.CONNECT_PROTOTYPES) & others and '#include "framesum_close.h"' in HEADER
    for name, (restype, argtypes) in abi.CONNECT_PROTOTYPES.items():
        params = params_of(BODY, name)
        assert restype is ctypes.c_int32 and len(params) == len(argtypes) == 49, name
        for p, t in zip(params, argtypes):
            want = ctypes.c_void_p if "*" in p else {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}[p.split()[0]]
            assert t is want, (name, p)
        # every parameter of the close call up to and including `ctl_code`, the seven new ones, the rest
        theirs = params_of(CLOSE_BODY, name.replace("connect", "close"))
        at = theirs.index("uint8_t* ctl_code") + 1
        assert params == theirs[:at] + NEW_PARAMS + theirs[at:]
    lib = framesum.load_library()
    for name, (restype, argtypes) in abi.CONNECT_PROTOTYPES.items():
        assert getattr(lib, name).restype is restype and getattr(lib, name).argtypes == argtypes


C_TYPES = {"uint8_t": ("u1", 1), "uint16_t": ("<u2", 2), "uint32_t": ("<u4", 4)}


def test_connect_dtypes_and_constants_are_the_headers():
    for name, dtype, size in (("fs_cn_sock", OPENER_DTYPE, 40), ("fs_cn_out", CONNECT_OUT_DTYPE, 48)):
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
    assert CONNECT_OUT_DTYPE.fields["reply"][1] == 42 and OPENER_DTYPE.fields["iss"][1] == 28
    defines = {k: int(v) for k, v in re.findall(r"#define (FS_\w+) (\d+)u", HEADER)}
    for k, v in dict(LISTEN=1, SYN_RCVD=2, SYN_SENT=3).items():
        assert defines["FS_ST_" + k] == getattr(abi, "ST_" + k) == getattr(ref, k) == v
    assert defines["FS_CN_BAD_ACK"] == abi.CN_BAD_ACK == ref.BAD_ACK == 11 and defines["FS_CN_SEND_SYN"] == abi.CN_SEND_SYN == 1
    for k, v in dict(NONE=0, ACK=1, SYNACK=2, RST=3, SYN=4).items():
        assert defines["FS_CN_REPLY_" + k] == getattr(abi, "CN_REPLY_" + k) == getattr(ref, "REPLY_" + k) == v
    assert (defines["FS_CN_STOP_RST"], defines["FS_CN_STOP_SYN"]) == (abi.CN_STOP_RST, abi.CN_STOP_SYN) == (1, 2)
    assert defines["FS_CONNECT_MAX_OPENERS"] == abi.CONNECT_MAX_OPENERS == 65536
    # codes 1, 4, 5 and 10 keep their close-call names and numbers
    assert (ref.TAKEN, ref.REJECTED, ref.KEEPALIVE, ref.EXPECTED) == (abi.CLOSE_TAKEN, abi.CLOSE_REJECTED, abi.CLOSE_KEEPALIVE,
                                                                     abi.CLOSE_EXPECTED)


def test_null_context_needs_no_device():
    lib = framesum.load_library()
    none = ctypes.c_void_p()
    some = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    tail = (some, 8, some, some, some, none, some, none, none)
    listen = (some, 1, some, 1, 0, some, some, none, some, none, none)
    closing = (some, 1, some, some, none)
    opening = (some, 1, 0, some, some, none, none)
    assert lib.fs_connect_flows_batch(None, some, some, some, 1, 0, 0, some, 1, some, 64, some, none, some, some, none, *listen,
                                      *closing, *opening, *tail, none) == -1
    assert lib.fs_connect_flows_batch_host(None, some, 64, some, some, 1, 0, 0, some, 1, some, 64, some, none, some, some, none,
                                           *listen, *closing, *opening, *tail) == -1


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
    for name, (restype, argtypes) in abi.CONNECT_PROTOTYPES.items():  # the loader set the seventh table too
        assert getattr(e.lib, name).restype is restype and getattr(e.lib, name).argtypes == argtypes
    e.lib.calls.clear()
    yield e
    e.close()


def test_connect_flows_host_marshals(eng):
    lengths = np.array([60, 61, 1514], dtype=np.uint32)
    offsets = np.array([0, 60, 124], dtype=np.uint64)
    frames = np.arange(1640, dtype=np.uint32).astype(np.uint8)
    socks, snd = np.zeros(2, dtype=SOCK_DTYPE), recv_ref.snd_of((5, 100), (6, 200))
    rings = np.zeros(500, dtype=np.uint8)
    listeners = accept_ref.listeners_of((acases.local(80), acases.MAC, 0, 3))
    slots = acases.default_slots(3)
    closers = np.zeros(4, dtype=CLOSER_DTYPE)
    openers = np.zeros(5, dtype=OPENER_DTYPE)
    res = eng.connect_flows_host(frames, offsets, lengths, socks, snd, rings, listeners, slots, closers, openers, reply_flags=2,
                                 mtu=1500, flags=1, synack_flags=2, payload=False)
    oout, replies, rout, rst = res[:4]
    cout, sclose, ctl, conns, lout, of, synacks, syn_out, syn_st, snd_out, code, socks_out, delivered, payload = res[4:18]
    (call,) = eng.lib.calls
    name, args = call
    want = [eng._ctx.value, frames, frames.nbytes, offsets, lengths, 3, 1500, 1, socks, 2, rings, 500, socks_out, delivered, snd,
            snd_out, code, listeners, 1, slots, 3, 2, conns, lout, of, synacks, syn_out, syn_st, closers, 4, cout, sclose, ctl,
            openers, 5, 2, oout, replies, rout, rst, None, 0]
    assert name == "fs_connect_flows_batch_host" and len(args) == 49 and payload is None
    for k, w in enumerate(want):
        assert plain(args[k]) == (w.ctypes.data if isinstance(w, np.ndarray) else w), f"argument {k}"
    assert oout.dtype == CONNECT_OUT_DTYPE and oout.shape == (5,) and replies.shape == (5 * 64,) and rst.shape == (5,)
    # the reply results left out, and no openers: null pointers
    res = eng.connect_flows_host(frames, offsets, lengths, socks, snd, rings, listeners, slots, closers,
                                 np.zeros(0, dtype=OPENER_DTYPE), reply_results=False, payload=False)
    args = eng.lib.calls[1][1]
    assert res[2] is None and res[3] is None and [plain(args[k]) for k in (34, 36, 37, 38, 39)] == [0, None, None, None, None]
    # the close call's own path is what it was
    eng.close_flows_host(frames, offsets, lengths, socks, snd, rings, listeners, slots, closers, payload=False)
    assert eng.lib.calls[2][0] == "fs_close_flows_batch_host" and len(eng.lib.calls[2][1]) == 42


def test_socks_from_connect():
    rows = [opener_of(1000 + k, 500 + k) for k in range(4)]
    openers = np.array(rows, dtype=OPENER_DTYPE)
    openers["key"][:, 10] = np.arange(4)
    out = np.zeros(4, dtype=CONNECT_OUT_DTYPE)
    out["state"] = (3, 4, 2, 3)
    out["rcv_nxt"], out["snd_una"], out["snd_wnd"], out["peer_mss"] = (0, 71, 81, 0), (1000, 1002, 1002, 1003), (1, 300, 400, 9), (0, 0, 536, 0)
    idx, socks, snd, tx = framesum.socks_from_connect(openers, out, ring_off=np.arange(4) * 64, ring_size=64)
    assert list(idx) == [1, 2] and socks.dtype == SOCK_DTYPE
    assert bytes(socks["key"][0]) == bytes(openers["key"][1]) and [int(x) for x in socks["snd_nxt"]] == [1002, 1003]
    assert [int(x) for x in socks["rcv_nxt"]] == [71, 81] and [int(x) for x in socks["rcv_wnd"]] == [501, 502]
    assert [int(x) for x in socks["ring_off"]] == [64, 128] and (socks["ring_free"] == 64).all()
    assert [int(x) for x in snd["snd_una"]] == [1002, 1002] and [int(x) for x in snd["snd_wnd"]] == [300, 400]
    assert [int(x) for x in tx["mss"]] == [1460, 536] and [int(x) for x in tx["snd_nxt"]] == [1002, 1003]
    h = bytes(tx["hdr"][0])
    key = bytes(openers["key"][1])
    assert h[0:6] == bytes(openers["remote_mac"][1]) and h[6:12] == bytes(openers["local_mac"][1])
    assert h[26:30] == key[5:9] and h[30:34] == key[1:5] and h[34:36] == key[11:13] and h[36:38] == key[9:11]
    nid = accept_ref.prand16(accept_ref.prand16(0x4321))
    assert h[18:20] == nid.to_bytes(2, "big")
