"""The ARP call off the GPU: the two statements of tests/arp_ref.py agree over a grid of one-frame cases and
differ only in the stated differences (a) to (d), each of which is reached; seqs_amd/csrc/framesum_arp.h alone
under ASan + UBSan (tests/csrc/test_arp.cpp, a stand-alone program); the ninth header against the binding's
tables, record layouts and the library's exported symbols; the host-side helpers."""
import ctypes
import itertools
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from seqs_amd import abi, framesum
from seqs_amd.framesum import ARP_HOST_DTYPE, ARP_HOST_OUT_DTYPE, ARP_QUERY_DTYPE, ARP_QUERY_OUT_DTYPE

import arp_ref as ref
from test_deliver_host import SAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tests", "csrc")
HEADER = open(os.path.join(ROOT, "include", "framesum_arp.h")).read()
BODY = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
UDP_BODY = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "framesum_udp.h")).read(), flags=re.S)
TEXT = " ".join(HEADER.replace("*", " ").split())

US, US_MAC = "10.0.0.1", "02:00:00:00:00:01"
PEER, PEER_MAC = "10.0.0.2", "02:00:00:00:00:02"


def flip(b: bytes, bit: int) -> bytes:
    b = bytearray(b)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


def prefill(slots):
    rng = np.random.default_rng(5)
    return (rng.integers(1, 256, slots * ref.STRIDE, dtype=np.uint8), rng.integers(1, 256, slots * 8, dtype=np.uint8).view(ref.DIGEST_DTYPE),
            rng.integers(1, 256, slots, dtype=np.uint8))


def both(frames, hosts, queries, n_reply_slots, arp_flags=0, mtu=0, fcs=False):
    pre = prefill(n_reply_slots + len(queries))
    a = ref.expected(frames, ref.verdicts(frames, mtu, fcs), hosts, queries, n_reply_slots, arp_flags, *pre, mtu=mtu, fcs=fcs)
    b = ref.recv_eth_model(frames, hosts, queries, n_reply_slots, arp_flags, *pre, mtu=mtu, fcs=fcs)
    return a, b


# ---- the two statements agree ------------------------------------------------------------------------------

QUERY_STATES = ("wait", "flagged", "done", "none")


def one_frame_cases():
    """(name, frame) over the grid: every Operation 0..3, each support field off by one, the destination MAC
    ours, broadcast and one bit away, ProtoTarget and ProtoSender ours and one bit away."""
    us, peer = ref.ip4(US), ref.ip4(PEER)
    for op, dst, tpa, spa in itertools.product(range(4), ("ours", "broadcast", "bit"), ("ours", "bit"), ("theirs", "bit")):
        d = {"ours": ref.mac6(US_MAC), "broadcast": ref.BROADCAST, "bit": flip(ref.mac6(US_MAC), 47)}[dst]
        yield (f"op{op}-{dst}-{tpa}-{spa}",
               ref.arp_frame(op, PEER_MAC, peer if spa == "theirs" else flip(peer, 0), US_MAC if op == 2 else b"\0" * 6,
                             us if tpa == "ours" else flip(us, 31), dst=d))
    for field, good in (("htype", 1), ("ptype", 0x0800), ("hlen", 6), ("plen", 4)):
        for d, dst in itertools.product((-1, 1), (ref.BROADCAST, flip(ref.mac6(US_MAC), 0))):
            yield f"{field}{d:+d}", ref.who_has(PEER_MAC, peer, us, dst=dst, **{field: good + d})


@pytest.mark.parametrize("state", QUERY_STATES)
@pytest.mark.parametrize("free", [0, 1])
def test_the_two_statements_agree_over_the_grid(state, free):
    hosts, n_reply = ref.hosts_of([ref.host_row(US, US_MAC, free=free)])
    queries = ref.queries_of([] if state == "none" else [ref.query_row(0, PEER, send=state == "flagged")])
    codes = set()
    for name, frame in one_frame_cases():
        # "done": an earlier reply in the same batch has resolved the query
        first = [ref.is_at(PEER_MAC, PEER, US_MAC, US)] if state == "done" else []
        a, b = both(first + [frame], hosts, queries, n_reply)
        assert ref.same(a, b) == [], (name, ref.same(a, b), a[5], b[5])
        padded, _ = both(first + [frame + b"\0" * 18], hosts, queries, n_reply)
        assert ref.same(a, padded) == [], name  # trailing padding is ignored
        codes.add(int(a[5][-1]))
        if name.startswith("op") and int(a[5][-1]) == ref.UNSUPPORTED:
            assert name[2] in "03"
    want = {ref.UNSUPPORTED, ref.IGNORED, ref.ANSWERED if free else ref.FULL}
    want |= {"wait": {ref.RESOLVED}, "done": {ref.STALE}}.get(state, set())
    assert codes == want, (codes, want)


@pytest.mark.parametrize("arp_flags", range(4))
def test_built_frames_mtu_and_fcs_reach_both_statements_alike(arp_flags):
    hosts, n_reply = ref.hosts_of([ref.host_row(US, US_MAC, free=2), ref.host_row("10.0.0.9", "02:00:00:00:00:09", free=1)])
    queries = ref.queries_of([ref.query_row(0, PEER), ref.query_row(1, "10.0.0.77", send=True)])
    frames = [ref.who_has(PEER_MAC, PEER, US), ref.is_at(PEER_MAC, PEER, US_MAC, US), ref.who_has(PEER_MAC, PEER, "10.0.0.9"),
              ref.who_has(PEER_MAC, PEER, US)[:41], ref.who_has(PEER_MAC, PEER, US, etype=0x0800), ref.who_has(PEER_MAC, PEER, US)[:33]]
    for mtu in (0, 59, 60):
        a, b = both(frames, hosts, queries, n_reply, arp_flags, mtu=mtu)
        assert ref.same(a, b) == []
        size = (60 if arp_flags & ref.PAD else 42) + (4 if arp_flags & ref.FCS_APPEND else 0)
        assert list(a[5]) == [ref.ANSWERED, ref.RESOLVED, ref.ANSWERED, 0, 0, 0] and list(a[6][:3]) == [0, 0, 2]
        refused = mtu == 59 and arp_flags & ref.PAD
        assert list(a[4][[0, 2, 4]]) == [2 if refused else 4] * 3  # FS_ERR_EXCEEDS_MTU or FS_ARP
        reply = bytes(a[2][:size])
        assert reply[:42] == ref.arp_frame(2, US_MAC, US, PEER_MAC, PEER, dst=PEER_MAC, src=US_MAC)
        assert bytes(a[2][4 * 64 : 4 * 64 + 42]) == ref.who_has("02:00:00:00:00:09", "10.0.0.9", "10.0.0.77")
        # slot 1 (free, unused) and slot 3 (an unflagged query's) keep every byte; so does the rest of each 64
        fill = np.random.default_rng(5).integers(1, 256, 5 * 64, dtype=np.uint8)  # (both()'s prefill of the frames)
        assert np.array_equal(a[2][64:128], fill[64:128]) and np.array_equal(a[2][192:256], fill[192:256])
        assert np.array_equal(a[2][size:64], fill[size:64])
    wire = [f + zlib.crc32(f).to_bytes(4, "little") for f in frames[:3]]
    wire[1] = wire[1][:-1] + bytes([wire[1][-1] ^ 0x80])
    a, b = both(wire, hosts, queries, n_reply, arp_flags, fcs=True)
    assert ref.same(a, b) == [] and list(a[5]) == [ref.ANSWERED, 0, ref.ANSWERED] and a[1][0]["state"] == ref.Q_WAIT


# ---- the stated differences, each reached ------------------------------------------------------------------

def faithful(frames, hosts, queries, n_reply_slots):
    return ref.recv_eth_model(frames, hosts, queries, n_reply_slots, 0, *prefill(n_reply_slots + len(queries)), faithful=True)


def test_difference_a_one_pending_response_becomes_free_slots():
    frames = [ref.who_has(PEER_MAC, f"10.0.1.{k}", US) for k in range(3)]
    one, n1 = ref.hosts_of([ref.host_row(US, US_MAC, free=1)])
    a, b = both(frames, one, ref.queries_of([]), n1)
    (f, _) = faithful(frames, one, ref.queries_of([]), n1)
    assert ref.same(a, b) == [] and ref.same(a, f) == [] and list(a[5]) == [ref.ANSWERED, ref.FULL, ref.FULL]  # free = 1 is the reference
    three, n3 = ref.hosts_of([ref.host_row(US, US_MAC, free=3)])
    a, b = both(frames, three, ref.queries_of([]), n3)
    (f, _) = faithful(frames, three, ref.queries_of([]), n3)
    assert ref.same(a, b) == [] and list(a[5]) == [ref.ANSWERED] * 3 and list(a[6]) == [0, 1, 2]
    assert list(f[5]) == [ref.ANSWERED, ref.FULL, ref.FULL] and set(ref.same(a, f)) >= {"arp_code", "hosts_out", "arp_frames"}
    assert "One pendingResponse becomes `free` slots" in TEXT


def test_difference_b_a_malformed_frame_with_a_foreign_mac():
    hosts, n = ref.hosts_of([ref.host_row(US, US_MAC)])
    foreign = flip(ref.mac6(US_MAC), 3)
    frames = [ref.who_has(PEER_MAC, PEER, US, dst=foreign, hlen=5), ref.who_has(PEER_MAC, PEER, US, dst=foreign),
              ref.who_has(PEER_MAC, PEER, US, hlen=5)]
    a, b = both(frames, hosts, ref.queries_of([]), n)
    (f, _) = faithful(frames, hosts, ref.queries_of([]), n)
    assert ref.same(a, b) == [] and list(a[5]) == [ref.UNSUPPORTED, ref.IGNORED, ref.UNSUPPORTED]
    assert list(f[5]) == [ref.IGNORED, ref.IGNORED, ref.UNSUPPORTED] and ref.same(a, f) == ["arp_code"]  # both drop it
    assert "here a malformed one is FS_ARP_UNSUPPORTED whatever its MAC" in TEXT


def test_difference_c_the_result_keeps_the_whole_header():
    hosts, n = ref.hosts_of([ref.host_row(US, US_MAC)])
    queries = ref.queries_of([ref.query_row(0, PEER)])
    frames = [ref.who_has(PEER_MAC, PEER, "10.0.0.200"), ref.is_at(PEER_MAC, PEER, "02:aa:aa:aa:aa:aa", US, dst=US_MAC)]
    a, b = both(frames, hosts, queries, n)
    (f, clients) = faithful(frames, hosts, queries, n)
    assert ref.same(a, b) == [] and ref.same(a, f) == []
    r = clients[0].results[0]  # `c.result = *ahdr`: every field of the reply, the odd HardwareTarget too
    assert r.put() == frames[1][14:42] and r.HardwareTarget == ref.mac6("02:aa:aa:aa:aa:aa")
    assert bytes(a[1][0]["mac"]) == r.HardwareSender == ref.mac6(PEER_MAC) and a[1][0]["frame"] == 1 and a[1][0]["n_replies"] == 1
    assert a[1].dtype.names == ("state", "reserved", "mac", "frame", "n_replies")  # the MAC and the frame index come back


def test_difference_d_several_hosts_and_several_queries():
    hosts, n = ref.hosts_of([ref.host_row(US, US_MAC), ref.host_row("10.0.0.3", US_MAC)])  # two hosts sharing a MAC
    queries = ref.queries_of([ref.query_row(0, PEER), ref.query_row(0, "10.0.0.5"), ref.query_row(1, PEER)])
    frames = [ref.is_at(PEER_MAC, PEER, US_MAC, US), ref.is_at("02:00:00:00:00:05", "10.0.0.5", US_MAC, US),
              ref.is_at(PEER_MAC, PEER, US_MAC, "10.0.0.3"), ref.who_has(PEER_MAC, PEER, "10.0.0.3"), ref.who_has(PEER_MAC, PEER, US)]
    a, b = both(frames, hosts, queries, n)
    (f, _) = faithful(frames, hosts, queries, n)
    assert ref.same(a, b) == [] and list(a[5]) == [ref.RESOLVED, ref.RESOLVED, ref.RESOLVED, ref.ANSWERED, ref.ANSWERED]
    assert list(a[6]) == [0, 1, 2, 1, 0] and list(a[1]["state"]) == [ref.Q_DONE] * 3
    # the reference's client has one result: the second BeginResolve of host 0 replaced the first
    assert list(f[5]) == [ref.IGNORED, ref.RESOLVED, ref.RESOLVED, ref.ANSWERED, ref.ANSWERED] and list(f[1]["state"]) == [ref.Q_WAIT, ref.Q_DONE, ref.Q_DONE]
    assert "Several hosts and several queries per call" in TEXT


def test_a_flagged_query_stays_unanswered_and_zero_is_an_address():
    hosts, n = ref.hosts_of([ref.host_row("0.0.0.0", US_MAC, free=1), ref.host_row(US, US_MAC, free=1)])
    queries = ref.queries_of([ref.query_row(1, PEER, send=True)])
    frames = [ref.is_at(PEER_MAC, PEER, US_MAC, US), ref.who_has(PEER_MAC, PEER, "0.0.0.0"), ref.who_has(PEER_MAC, PEER, "10.0.0.77")]
    a, b = both(frames, hosts, queries, n)
    assert ref.same(a, b) == [] and list(a[5]) == [ref.IGNORED, ref.ANSWERED, ref.IGNORED] and a[1][0]["state"] == ref.Q_SENT
    assert a[1][0]["n_replies"] == 0 and a[1][0]["frame"] == ref.NONE
    a, b = both([], hosts, queries, n)  # n == 0: the flagged request is still built
    assert ref.same(a, b) == [] and bytes(a[2][2 * 64 : 2 * 64 + 42]) == ref.who_has(US_MAC, US, PEER) and a[4][2] == 4
    a, b = both(frames, hosts[:0], queries[:0], 0)  # no host: the codes alone
    assert ref.same(a, b) == [] and list(a[5]) == [ref.IGNORED] * 3 and (a[6] == ref.NONE).all()


# ---- the header-only arithmetic under the sanitizers -------------------------------------------------------

def test_arp_arithmetic_under_asan_ubsan():
    out = os.path.join(CSRC, "build", "test_arp")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *SAN, "-o", out, os.path.join(CSRC, "test_arp.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "arp checks OK" in r.stdout


# ---- the ninth header and the binding's tables -------------------------------------------------------------

def params_of(body, name):
    p = body[body.index(name + "(") + len(name) + 1 :]
    return [" ".join(x.split()) for x in p[: p.index(")")].split(",")]


NEW_PARAMS = ["const fs_arp_host* hosts", "uint32_t n_hosts", "const fs_arp_query* queries", "uint32_t n_queries",
              "uint32_t n_reply_slots", "uint32_t arp_flags", "fs_arp_host_out* hosts_out", "fs_arp_query_out* queries_out",
              "uint8_t* arp_frames", "fs_digest* arp_out", "uint8_t* arp_status", "uint8_t* arp_code", "uint32_t* arp_of"]


def test_arp_prototypes_are_the_headers():
    names = ["fs_arp_flows_batch", "fs_arp_flows_batch_host"]
    assert re.findall(r"^fs_status\s+(fs_\w+)\s*\(", BODY, flags=re.M) == list(abi.ARP_PROTOTYPES) == names
    others = (set(abi.PROTOTYPES) | set(abi.DELIVER_PROTOTYPES) | set(abi.SEND_RINGS_PROTOTYPES) | set(abi.RECV_PROTOTYPES) |
              set(abi.ACCEPT_PROTOTYPES) | set(abi.CLOSE_PROTOTYPES) | set(abi.CONNECT_PROTOTYPES) | set(abi.UDP_PROTOTYPES))
    assert not set(abi.ARP_PROTOTYPES) & others and '#include "framesum_udp.h"' in HEADER
    for name, (restype, argtypes) in abi.ARP_PROTOTYPES.items():
        params = params_of(BODY, name)
        assert restype is ctypes.c_int32 and len(params) == len(argtypes) == 69, name
        for p, t in zip(params, argtypes):
            want = ctypes.c_void_p if "*" in p else {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}[p.split()[0]]
            assert t is want, (name, p)
        # every parameter of the UDP call up to and including `cell_of`, the thirteen new ones, the rest
        theirs = params_of(UDP_BODY, name.replace("arp", "udp"))
        at = theirs.index("uint32_t* cell_of") + 1
        assert params == theirs[:at] + NEW_PARAMS + theirs[at:]
    lib = framesum.load_library()  # (a library that lacks one of the two symbols raises here)
    for name, (restype, argtypes) in abi.ARP_PROTOTYPES.items():
        assert getattr(lib, name).restype is restype and getattr(lib, name).argtypes == argtypes


C_TYPES = {"uint8_t": 1, "uint16_t": 2, "uint32_t": 4, "uint64_t": 8}


def test_arp_dtypes_and_constants_are_the_headers():
    for name, dtype, mine, size in (("fs_arp_host", ARP_HOST_DTYPE, ref.HOST_DTYPE, 20), ("fs_arp_query", ARP_QUERY_DTYPE, ref.QUERY_DTYPE, 12),
                                    ("fs_arp_host_out", ARP_HOST_OUT_DTYPE, ref.HOST_OUT_DTYPE, 16),
                                    ("fs_arp_query_out", ARP_QUERY_OUT_DTYPE, ref.QUERY_OUT_DTYPE, 16)):
        body = BODY[BODY.index("typedef struct " + name + " {") : BODY.index("} " + name + ";")]
        at, fields = 0, []
        for ctype, decl in re.findall(r"(uint8_t|uint16_t|uint32_t|uint64_t)\s+([^;]+);", body):
            for item in decl.split(","):
                m = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", item)
                count = int(m.group(2) or 1)
                fields.append((m.group(1), at, C_TYPES[ctype] * count))
                assert at % C_TYPES[ctype] == 0, (name, m.group(1))  # no padding: every field naturally aligned
                at += C_TYPES[ctype] * count
        assert at == size == dtype.itemsize, name
        assert [(f, dtype.fields[f][1], dtype.fields[f][0].itemsize) for f in dtype.names] == fields, name
        assert dtype == mine, name
        assert f"{size} bytes" in HEADER[HEADER.index("typedef struct " + name + " {") :].split("\n")[0]
    defines = dict(re.findall(r"#define (FS_\w+) (\w+)u", HEADER))
    assert int(defines["FS_ARP_NONE"], 16) == abi.ARP_NONE == ref.NONE
    assert int(defines["FS_ARP_MAX_HOSTS"]) == abi.ARP_MAX_HOSTS == 65536 == int(defines["FS_ARP_MAX_QUERIES"]) == abi.ARP_MAX_QUERIES
    assert int(defines["FS_ARP_MAX_REPLY_SLOTS"]) == abi.ARP_MAX_REPLY_SLOTS == 65536
    assert int(defines["FS_ARP_FRAME"]) == abi.ARP_FRAME == 42 and int(defines["FS_ARP_FRAME_PADDED"]) == abi.ARP_FRAME_PADDED == 60
    assert int(defines["FS_ARP_PAD"]) == abi.ARP_PAD == ref.PAD == 1 and abi.FCS_APPEND == ref.FCS_APPEND == 2
    assert int(defines["FS_ARP_SEND_REQUEST"]) == abi.ARP_SEND_REQUEST == ref.SEND_REQUEST
    enums = dict((k, int(v)) for k, v in re.findall(r"(FS_ARP_\w+) = (\d+)", BODY))
    for name, mine, theirs in (("NOT_ARP", abi.ARP_NOT_ARP, ref.NOT_ARP), ("UNSUPPORTED", abi.ARP_UNSUPPORTED, ref.UNSUPPORTED),
                               ("IGNORED", abi.ARP_IGNORED, ref.IGNORED), ("ANSWERED", abi.ARP_ANSWERED, ref.ANSWERED),
                               ("FULL", abi.ARP_FULL, ref.FULL), ("RESOLVED", abi.ARP_RESOLVED, ref.RESOLVED),
                               ("STALE", abi.ARP_STALE, ref.STALE), ("Q_WAIT", abi.ARP_Q_WAIT, ref.Q_WAIT),
                               ("Q_DONE", abi.ARP_Q_DONE, ref.Q_DONE), ("Q_SENT", abi.ARP_Q_SENT, ref.Q_SENT)):
        assert enums["FS_ARP_" + name] == mine == theirs, name
    assert ref.FS_ARP == 4 and ref.STRIDE == abi.ACCEPT_STRIDE


def test_null_context_needs_no_device():
    lib = framesum.load_library()
    none = ctypes.c_void_p()
    some = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    tail = (some, 8, some, some, some, none, some, none, none)
    listen = (some, 1, some, 1, 0, some, some, none, some, none, none)
    closing = (some, 1, some, some, none)
    opening = (some, 1, 0, some, some, none, none)
    udp = (some, 1, some, 64, some, none, none)
    arp = (some, 1, some, 1, 1, 0, some, some, some, none, none, none, none)
    assert lib.fs_arp_flows_batch(None, some, some, some, 1, 0, 0, some, 1, some, 64, some, none, some, some, none, *listen,
                                  *closing, *opening, *udp, *arp, *tail, none) == -1
    assert lib.fs_arp_flows_batch_host(None, some, 64, some, some, 1, 0, 0, some, 1, some, 64, some, none, some, some, none,
                                       *listen, *closing, *opening, *udp, *arp, *tail) == -1


# ---- the host-side helpers ---------------------------------------------------------------------------------

def test_arp_host_arp_query_split_arp_and_hosts_after():
    from seqs_amd import arp_host, arp_query, arp_reply_slots, hosts_after, split_arp

    rows = [arp_host(US, US_MAC, free=2), arp_host("10.0.0.9", bytes([2, 0, 0, 0, 0, 9]), slot0=2, free=1)]
    assert rows[0].tobytes() == ref.host_row(US, US_MAC, free=2).tobytes() and rows[1].tobytes() == ref.host_row("10.0.0.9", "02:00:00:00:00:09", 2, 1).tobytes()
    hosts = np.concatenate(rows)
    queries = np.concatenate([arp_query(0, PEER), arp_query(1, "10.0.0.77", send=True)])
    assert queries.tobytes() == ref.queries_of([ref.query_row(0, PEER), ref.query_row(1, "10.0.0.77", send=True)]).tobytes()
    assert arp_reply_slots(hosts) == 3 and arp_reply_slots(hosts[:0]) == 0
    frames = [ref.who_has(PEER_MAC, PEER, US), ref.is_at(PEER_MAC, PEER, US_MAC, US), ref.who_has(PEER_MAC, PEER, "10.0.0.9")]
    out = ref.expected(frames, ref.verdicts(frames), hosts, queries, 3, ref.FCS_APPEND)
    replies, requests, resolutions = split_arp(hosts, queries, out[0], out[1], out[2], arp_flags=ref.FCS_APPEND)
    assert [len(r) for r in replies] == [1, 1] and len(replies[0][0]) == 46
    assert replies[0][0][:42] == ref.arp_frame(2, US_MAC, US, PEER_MAC, PEER, dst=PEER_MAC, src=US_MAC)
    assert list(requests) == [1] and requests[1][:42] == ref.who_has("02:00:00:00:00:09", "10.0.0.9", "10.0.0.77")
    assert resolutions == {0: (ref.mac6(PEER_MAC), 1)}
    nxt = hosts_after(hosts, out[0])
    assert nxt.tobytes() == hosts.tobytes() and list(hosts_after(hosts, out[0], free=[1, 0])["free"]) == [1, 0]
    with pytest.raises(AssertionError):
        hosts_after(hosts[::-1], out[0])
