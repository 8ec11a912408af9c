"""The accept call (fs_accept_flows_batch / fs_accept_flows_batch_host) without a GPU: the arithmetic of
seqs_amd/csrc/framesum_accept.h under ASan + UBSan (a stand-alone program run as a child process, which
also goes through every rejection of the listener and slot lists), the fifth header against the binding's
table, record layouts and constants, the entry points' null-context path, what the Python methods hand to
the C ABI, socks_from_accept, and the agreement of the two restatements of tests/accept_ref.py over a grid
of first frames, except on the stated differences, each of which is shown to be reached."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 (before the stand-in replaces ctypes.CDLL: torch loads its own libraries through it)

from seqs_amd import abi, framesum
from seqs_amd.framesum import (ACCEPT_CONN_DTYPE, ACCEPT_SLOT_DTYPE, DIGEST_DTYPE, LISTENER_DTYPE, LISTENER_OUT_DTYPE,
                               SND_DTYPE, SOCK_DTYPE, TX_SOCK_DTYPE)

import accept_cases as cases
import accept_ref as ref
import deliver_ref as dref
import flows_ref as fref
import recv_ref
from test_deliver_host import SAN, plain
from test_recv_host import RecvStandIn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tests", "csrc")
HEADER = open(os.path.join(ROOT, "include", "framesum_accept.h")).read()
BODY = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
RECV_BODY = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "framesum_recv.h")).read(), flags=re.S)
M32 = ref.M32
SYN = ref.SYN


def test_accept_arithmetic_under_asan_ubsan():
    out = os.path.join(CSRC, "build", "test_accept")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *SAN, "-o", out, os.path.join(CSRC, "test_accept.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "accept checks OK" in r.stdout


# ---- the fifth header and the binding's tables -------------------------------------------------------

def params_of(body, name):
    p = body[body.index(name + "(") + len(name) + 1 :]
    return [" ".join(x.split()) for x in p[: p.index(")")].split(",")]


NEW_PARAMS = ["const fs_listener* listeners", "uint32_t n_listeners", "const fs_accept_slot* slots", "uint32_t n_slots",
              "uint32_t synack_flags", "fs_accept_conn* conns", "fs_listener_out* listeners_out", "uint32_t* accept_of",
              "uint8_t* synacks", "fs_digest* synack_out", "uint8_t* synack_status"]


def test_accept_prototypes_are_the_headers():
    names = ["fs_accept_flows_batch", "fs_accept_flows_batch_host"]
    assert re.findall(r"^fs_status\s+(fs_\w+)\s*\(", BODY, flags=re.M) == list(abi.ACCEPT_PROTOTYPES) == names
    others = set(abi.PROTOTYPES) | set(abi.DELIVER_PROTOTYPES) | set(abi.SEND_RINGS_PROTOTYPES) | set(abi.RECV_PROTOTYPES)
    assert not set(abi.ACCEPT_PROTOTYPES) & others and '#include "framesum_recv.h"' in HEADER
    for name, (restype, argtypes) in abi.ACCEPT_PROTOTYPES.items():
        params = params_of(BODY, name)
        assert restype is ctypes.c_int32 and len(params) == len(argtypes) == 37, name
        for p, t in zip(params, argtypes):
            want = ctypes.c_void_p if "*" in p else {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}[p.split()[0]]
            assert t is want, (name, p)
        # every parameter of the receive call up to and including `code`, the eleven new ones, the rest
        theirs = params_of(RECV_BODY, name.replace("accept", "recv"))
        at = theirs.index("uint8_t* code") + 1
        assert params == theirs[:at] + NEW_PARAMS + theirs[at:]
    lib = framesum.load_library()
    for name, (restype, argtypes) in abi.ACCEPT_PROTOTYPES.items():
        assert getattr(lib, name).restype is restype and getattr(lib, name).argtypes == argtypes


C_TYPES = {"uint8_t": ("u1", 1), "uint16_t": ("<u2", 2), "uint32_t": ("<u4", 4)}


def test_accept_dtypes_and_constants_are_the_headers():
    for name, dtype, size in (("fs_listener", LISTENER_DTYPE, 24), ("fs_accept_slot", ACCEPT_SLOT_DTYPE, 12),
                              ("fs_accept_conn", ACCEPT_CONN_DTYPE, 48), ("fs_listener_out", LISTENER_OUT_DTYPE, 16)):
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
    defines = dict(re.findall(r"#define (FS_ACCEPT_\w+) (\w+)u", HEADER))
    assert int(defines["FS_ACCEPT_STRIDE"]) == abi.ACCEPT_STRIDE == ref.STRIDE == 64
    assert int(defines["FS_ACCEPT_NONE"], 16) == abi.ACCEPT_NONE == ref.NONE == 0xFFFFFFFF
    assert int(defines["FS_ACCEPT_FULL"], 16) == abi.ACCEPT_FULL == ref.FULL == 0xFFFFFFFE
    assert int(defines["FS_ACCEPT_MAX_LISTENERS"]) == abi.ACCEPT_MAX_LISTENERS == 65536
    assert int(defines["FS_ACCEPT_MAX_SLOTS"]) == abi.ACCEPT_MAX_SLOTS == 65536
    # the header states the three differences, the half-open listing and how the host form returns synacks
    text = " ".join(HEADER.replace("*", " ").split())
    for words in ("A SYN that carries data is not a candidate", "never spends two slots on a retransmitted SYN",
                  "there is no wildcard address", "snd[s] = {iss, conn.snd_wnd}", "come back WHOLE"):
        assert words in text, words


def test_null_context_needs_no_device():
    lib = framesum.load_library()
    none = ctypes.c_void_p()
    some = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    tail = (some, 8, some, some, some, none, some, none, none)
    listen = (some, 1, some, 1, 0, some, some, none, some, none, none)
    assert lib.fs_accept_flows_batch(None, some, some, some, 1, 0, 0, some, 1, some, 64, some, none, some, some, none, *listen,
                                     *tail, none) == -1
    assert lib.fs_accept_flows_batch_host(None, some, 64, some, some, 1, 0, 0, some, 1, some, 64, some, none, some, some, none,
                                          *listen, *tail) == -1


# ---- the binding: what the methods hand to the C ABI ---------------------------------------------------

@pytest.fixture
def eng(monkeypatch, tmp_path):
    product = tmp_path / "libframesum.so"
    product.write_bytes(b"")
    monkeypatch.setattr(ctypes, "CDLL", RecvStandIn)
    monkeypatch.setattr(abi, "_LIB_PATH", str(product))
    monkeypatch.setattr(abi, "_lib", None)
    monkeypatch.setattr(abi, "_libs", {})
    e = framesum.Engine(0)
    for name, (restype, argtypes) in abi.ACCEPT_PROTOTYPES.items():  # the loader set the fifth table too
        assert getattr(e.lib, name).restype is restype and getattr(e.lib, name).argtypes == argtypes
    e.lib.calls.clear()
    yield e
    e.close()


def test_accept_flows_host_marshals(eng):
    lengths = np.array([60, 61, 1514], dtype=np.uint32)
    offsets = np.array([0, 60, 124], dtype=np.uint64)
    frames = np.arange(1640, dtype=np.uint32).astype(np.uint8)
    socks, snd = np.zeros(2, dtype=SOCK_DTYPE), recv_ref.snd_of((5, 100), (6, 200))
    rings = np.zeros(500, dtype=np.uint8)
    listeners = ref.listeners_of((cases.local(80), cases.MAC, 0, 3))
    slots = cases.default_slots(3)
    res = eng.accept_flows_host(frames, offsets, lengths, socks, snd, rings, listeners, slots, 1500, 1, 2, payload=False)
    conns, lout, of, synacks, syn_out, syn_st, snd_out, code, socks_out, delivered, payload = res[:11]
    (call,) = eng.lib.calls
    name, args = call
    want = [eng._ctx.value, frames, frames.nbytes, offsets, lengths, 3, 1500, 1, socks, 2, rings, 500, socks_out, delivered, snd,
            snd_out, code, listeners, 1, slots, 3, 2, conns, lout, of, synacks, syn_out, syn_st, None, 0]
    assert name == "fs_accept_flows_batch_host" and len(args) == 37 and payload is None
    for k, w in enumerate(want):
        assert plain(args[k]) == (w.ctypes.data if isinstance(w, np.ndarray) else w), f"argument {k}"
    assert conns.dtype == ACCEPT_CONN_DTYPE and conns.shape == (3,) and lout.dtype == LISTENER_OUT_DTYPE and lout.shape == (1,)
    assert of.dtype == np.uint32 and (of == abi.ACCEPT_NONE).all() and synacks.shape == (192,) and syn_out.dtype == DIGEST_DTYPE
    # the nullable arrays left out: null pointers
    res = eng.accept_flows_host(frames, offsets, lengths, socks, snd, rings, listeners, slots, accept_of=False,
                                synack_results=False, payload=False)
    args = eng.lib.calls[1][1]
    assert res[2] is None and res[4] is None and res[5] is None and [plain(args[k]) for k in (24, 26, 27)] == [None] * 3
    # no slots: conns and synacks are null pointers too
    eng.accept_flows_host(frames, offsets, lengths, socks, snd, rings, ref.listeners_of((cases.local(80), cases.MAC, 0, 0)),
                          ref.slots_of(), payload=False)
    args = eng.lib.calls[2][1]
    assert [plain(args[k]) for k in (20, 22, 25)] == [0, None, None]


def test_socks_from_accept():
    case = cases.three_listeners()
    buf, off, ln = fref.pack(case.frames)
    synacks = np.zeros(len(case.slots) * 64, dtype=np.uint8)
    e = ref.expected(buf, off, ln, 0, 0, np.zeros(8, np.uint8), 0, 0, case.socks, case.snd, np.zeros(64, np.uint8),
                     case.listeners, case.slots, 0, synacks)
    idx, socks, snd, tx = framesum.socks_from_accept(e["conns"], case.slots, case.listeners, np.arange(16) * 100, 100, mss=536)
    assert list(idx) == [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14] and socks.dtype == SOCK_DTYPE and snd.dtype == SND_DTYPE
    assert tx.dtype == TX_SOCK_DTYPE and len(socks) == len(snd) == len(tx) == 13
    for k, slot in enumerate(idx):
        c, sl = e["conns"][slot], case.slots[slot]
        fr = case.frames[int(c["frame"])]
        assert bytes(socks["key"][k]) == fref.flow_key(fr) and int(socks["rcv_nxt"][k]) == int(c["irs"]) + 1
        assert int(socks["snd_nxt"][k]) == int(sl["iss"]) + 1 and int(socks["rcv_wnd"][k]) == int(sl["rcv_wnd"])
        assert (int(socks["ring_off"][k]), int(socks["ring_size"][k]), int(socks["ring_free"][k])) == (100 * slot, 100, 100)
        assert (int(snd["snd_una"][k]), int(snd["snd_wnd"][k])) == (int(sl["iss"]), int(c["snd_wnd"]))
        # the template is the SYN-ACK's header with the next ID: same addresses, ports and MACs
        sa = bytes(e["synacks"][slot * 64 : slot * 64 + 54])
        hdr = bytes(tx["hdr"][k])
        assert hdr[:16] == sa[:16] and hdr[22:24] == sa[22:24] and hdr[26:38] == sa[26:38] and hdr[46] == 0x50
        assert int.from_bytes(hdr[18:20], "big") == ref.prand16(int.from_bytes(sa[18:20], "big"))
        assert int(tx["mss"][k]) == 536 and int(tx["snd_una"][k]) == int(tx["snd_nxt"][k]) == int(sl["iss"]) + 1
    # the listed half-open connection takes the handshake's third ACK as code 1, a wrong Ack as 2 or 3
    iss, irs = int(case.slots["iss"][0]), int(e["conns"]["irs"][0])
    for ack, code in ((iss + 1, recv_ref.TAKEN), (iss, recv_ref.DUPLICATE), (iss + 2, recv_ref.UNSENT)):
        codes, una, _, _ = recv_ref.contract([(irs + 1, ack % M32, 500, recv_ref.ACK, 0)], [False], int(snd["snd_una"][0]),
                                             int(snd["snd_wnd"][0]), int(socks["rcv_nxt"][0]), int(socks["snd_nxt"][0]), 8192)
        assert codes == [code] and (una == iss + 1) == (code == recv_ref.TAKEN)


# ---- the two restatements agree ------------------------------------------------------------------------

OTHER = cases.OTHER_FLAGS
GRID = list(itertools.product((0,) + OTHER, (0, 1), (0, 1), (0, 1, 65535), (7, M32 - 1)))  # flag, Ack, payload, window, Seq


def one_batch(frames, listeners, slots, socks=None):
    buf, off, ln = fref.pack(frames)
    synacks = np.zeros(len(slots) * 64, dtype=np.uint8)
    socks = dref.socks_of() if socks is None else socks
    snd = recv_ref.snd_of(*[(0, 0)] * len(socks))
    return ref.expected(buf, off, ln, 0, 0, np.zeros(8, np.uint8), 0, 0, socks, snd, np.zeros(64, np.uint8), listeners, slots, 0,
                        synacks)


@pytest.mark.parametrize("rcv_wnd", [0, 65535, 65536, M32 - 1])
def test_the_two_restatements_agree_on_first_frames(rcv_wnd):
    rng = np.random.default_rng(8100)
    frames = fref.finish([cases.syn(cases.header(rng, 0x100 + k), seq=seq, window=window, flags9=SYN | bit, ack=ack,
                                    payload=b"p" * pay) for k, (bit, ack, pay, window, seq) in enumerate(GRID)])
    slots = ref.slots_of(*[(M32 - 2 + k, rcv_wnd, (0xFFF0 + k) & 0xFFFF) for k in range(len(GRID))])
    e = one_batch(frames, ref.listeners_of((cases.local(80), cases.MAC, 0, len(GRID))), slots)
    assert e["n_flows"] == len(GRID)
    seen = dict(agree_open=0, agree_drop=0, data=0, window=0)
    for f, (fr, (bit, ack, pay, window, seq)) in enumerate(zip(frames, GRID)):
        slot = int(e["accept_of"][f])
        sl = slots[slot if slot != ref.NONE else 0]
        lst = ref.GoListener(cases.LOCAL_IP, 80, cases.MAC, [ref.GoConn(int(sl["iss"]), rcv_wnd, int(sl["ip_id"]))])
        err, idx = lst.recv(fr)
        tcb = lst.conns[0].scb
        if bit == 0 and ack == 0 and pay == 1:
            # difference 1: the reference opens on a SYN with data and advances rcv.NXT over it
            assert slot == ref.NONE and (err, idx) == (None, 0) and tcb.state == ref.STATE_SYN_RCVD
            assert tcb.rcv_NXT == (seq + 2) % M32 and lst.conns[0].rx == b"p"
            seen["data"] += 1
            continue
        if slot == ref.NONE:
            assert (err, idx) == ("ErrDroppedPacket", None) and tcb.state == ref.STATE_LISTEN and (bit or ack)
            seen["agree_drop"] += 1
            continue
        c = e["conns"][slot]
        assert (err, idx) == (None, 0) and tcb.state == ref.STATE_SYN_RCVD and (bit, ack, pay) == (0, 0, 0)
        assert (tcb.rcv_IRS, tcb.rcv_NXT, tcb.snd_UNA, tcb.snd_WND) == (int(c["irs"]), int(c["rcv_nxt"]), int(sl["iss"]), int(c["snd_wnd"]))
        assert lst.conns[0].remoteMAC == bytes(c["remote_mac"]) and lst.conns[0].remote == (bytes(c["key"][1:5]), int.from_bytes(bytes(c["key"][9:11]), "big"))
        sent = lst.send(0)
        mine = bytes(e["synacks"][slot * 64 : slot * 64 + 54])
        if rcv_wnd > 65535:
            # the stated window difference: the frame here carries min(rcv_wnd, 65535); the reference's Send
            # refuses a window above 16 bits (errWindowTooLarge) before CalculateHeaders would truncate it
            assert sent == "errWindowTooLarge" and mine[48:50] == b"\xff\xff"
            seen["window"] += 1
            continue
        assert sent == mine and tcb.snd_NXT == int(c["snd_nxt"]) and tcb.pending == [0, 0]  # zero window included
        assert recv_ref.fields(mine)[:4] == (int(sl["iss"]), (seq + 1) % M32, rcv_wnd, ref.SYNACK)
        seen["agree_open"] += 1
    assert seen["data"] == 6 and seen["agree_drop"] == len(GRID) - 12
    assert (seen["window"], seen["agree_open"]) == ((6, 0) if rcv_wnd > 65535 else (0, 6))


def test_the_other_two_differences_are_reached():
    rng = np.random.default_rng(8200)
    h1, h2 = cases.header(rng, 0x111), cases.header(rng, 0x222)
    s1, s2 = fref.finish([cases.syn(h1, seq=10), cases.syn(h2, seq=20)])
    # difference 2: a known remote's retransmitted SYN. Both remotes open; the first connection is freed
    # for reuse; the second remote's SYN comes again
    lst = ref.GoListener(cases.LOCAL_IP, 80, cases.MAC, [ref.GoConn(1000, 100, 1), ref.GoConn(2000, 100, 2)])
    assert lst.recv(s1) == (None, 0) and lst.recv(s2) == (None, 1)
    lst.conns[0] = ref.GoConn(3000, 100, 3)
    assert lst.recv(s2) == (None, 0) and lst.conns[0].remote == lst.conns[1].remote  # two connections, one remote
    # here the host lists the half-open connection: its SYN is no candidate, a stranger's is
    listeners, slots = ref.listeners_of((cases.local(80), cases.MAC, 0, 2)), ref.slots_of((3000, 100, 3), (4000, 100, 4))
    socks = dref.socks_of(dref.sock(fref.flow_key(s2), 21, 0, 8, snd_nxt=2001))
    e = one_batch([s2, s1], listeners, slots, socks)
    assert [int(x) for x in e["accept_of"][:2]] == [ref.NONE, 0] and int(e["listeners_out"]["n_syn"][0]) == 1
    # without the listing it is one: the listing is what saves the slot
    assert [int(x) for x in one_batch([s2, s1], listeners, slots)["accept_of"][:2]] == [0, 1]
    # difference 3: a SYN to the listener's port at another address. TCPListener.recv never looks at the
    # destination address; here no listener's `local` equals it
    (s3,) = fref.finish([cases.syn(cases.header(rng, 0x333, ip=bytes([10, 0, 0, 9])), seq=30)])
    lst = ref.GoListener(cases.LOCAL_IP, 80, cases.MAC, [ref.GoConn(1000, 100, 1)])
    assert lst.recv(s3) == (None, 0)
    assert int(one_batch([s3], listeners, slots)["accept_of"][0]) == ref.NONE
