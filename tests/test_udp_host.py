"""The UDP call off the GPU: the two statements of tests/udp_ref.py agree over a grid and differ only in the
stated difference, which is reached; seqs_amd/csrc/framesum_udp.h alone under ASan + UBSan
(tests/csrc/test_udp.cpp, a stand-alone program); the eighth header against the binding's tables, record
layouts and the library's exported symbols; the host-side helpers."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from seqs_amd import abi, framesum
from seqs_amd.framesum import UDP_CELL_DTYPE, UDP_PORT_DTYPE, UDP_PORT_OUT_DTYPE

import udp_ref as ref
from test_deliver_host import SAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tests", "csrc")
HEADER = open(os.path.join(ROOT, "include", "framesum_udp.h")).read()
BODY = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
CONNECT_BODY = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "framesum_connect.h")).read(), flags=re.S)
TEXT = " ".join(HEADER.replace("*", " ").split())

US, OTHER, BCAST = "10.0.0.1", "10.0.0.2", "255.255.255.255"


def both(frames, ports, cells_bytes, mtu=0, fcs=False):
    cells0 = np.random.default_rng(5).integers(1, 256, cells_bytes, dtype=np.uint8)
    a = ref.expected(frames, ref.verdicts(frames, mtu, fcs), ports, cells0, fcs)
    b = ref.recv_eth_model(frames, ports, cells0, mtu, fcs)
    return a, b


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


# ---- the two statements agree ------------------------------------------------------------------------------

@pytest.mark.parametrize("listed", ["exact", "wildcard", "both"])
@pytest.mark.parametrize("free", [0, 1, 2, 5, 6])
def test_the_two_statements_agree_over_the_grid(listed, free):
    rows = []
    if listed in ("exact", "both"):
        rows.append(ref.port_row(US, 67, 3, 48, wcell=2, free=min(free, 3)))
    if listed in ("wildcard", "both"):
        rows.append(ref.port_row("0.0.0.0", 67, 6, 40, wcell=5, free=free))
    rows.append(ref.port_row(US, 123, 2, 64, free=min(free, 2)))
    ports, cells_bytes = ref.lay_out(rows, lead=16, gap=8)
    frames = []
    for k, (dst, dport, proto) in enumerate(itertools.product((US, OTHER, BCAST), (67, 68, 123), (17, 6))):
        frames.append(ref.udp_frame(f"192.168.{k}.9", dst, 1000 + k, dport, bytes(range(k % 19)), proto=proto))
    # each rejected verdict of the UDP branch: bad checksum, zero port, UDP Length below 8, too short, TotalLength past the frame
    good = ref.udp_frame("192.168.1.1", US, 5000, 67, b"abcdefgh")
    frames += [ref.udp_frame("192.168.1.1", US, 5000, 67, b"abcdefgh", bad_csum=True),
               good[:34] + b"\0\0" + good[36:], good[:38] + b"\0\7" + good[40:], good[:40], good[:30],
               good[:16] + (24).to_bytes(2, "big") + good[18:38],
               good[:16] + (500).to_bytes(2, "big") + good[18:], good[:12] + b"\x08\x06" + good[14:], good]
    # truncation by -1 / 0 / +1 against each cell size, IP options, a UDP Length that disagrees, padding
    for room in (8, 16, 32):
        for d in (-1, 0, 1):
            frames.append(ref.udp_frame("192.168.2.2", US if room != 8 else OTHER, 6000, 67 if room != 32 else 123, bytes(room + d)))
    frames.append(ref.udp_frame("192.168.3.3", US, 7000, 67, b"opts", ip_options=b"\x01" * 8))
    frames.append(ref.udp_frame("192.168.3.3", US, 7000, 123, b"long", udp_length=99, pad=b"\0" * 7))
    a, b = both(frames, ports, cells_bytes)
    assert same(a, b), (a[0], b[0])
    assert a[0]["n_matched"].sum() > 0 and (free == 0 or a[0]["n_admitted"].sum() > 0)
    v = ref.verdicts(frames)
    assert {1, 7, 9, 10, 11, 13} <= set(int(x) for x in v) and (a[1][v != 0] == ref.NONE).all()
    if listed == "both":  # an exact address wins over the wildcard; other destinations go to the wildcard
        assert a[1][0] == 0 and set(a[1][[k for k, f in enumerate(frames) if f[30:34] == ref.ip4(OTHER) and a[1][k] != ref.NONE]]) == {1}


def test_mtu_and_fcs_reach_both_statements_alike():
    ports, cells_bytes = ref.lay_out([ref.port_row("0.0.0.0", 67, 4, 64)])
    frames = [ref.udp_frame(US, OTHER, 68, 67, bytes(k)) for k in (0, 20, 30, 40)]
    a, b = both(frames, ports, cells_bytes, mtu=14 + 28 + 25)
    assert same(a, b) and list(a[1]) == [0, 0, ref.NONE, ref.NONE]
    from oracle import pyref
    wire = [pyref.fill_frame(f, 0, pyref.FCS_APPEND)[0] for f in frames]
    wire[1] = wire[1][:-1] + bytes([wire[1][-1] ^ 0x80])
    a, b = both(wire, ports, cells_bytes, fcs=True)
    assert same(a, b) and list(a[1]) == [0, ref.NONE, 0, 0] and list(a[2]) == [0, ref.NONE, 1, 2]


def test_the_stated_difference_is_reached_and_n_cells_1_is_the_reference():
    """The reference's handler holds one packet and drops while it is pending: a one-cell queue. A longer
    queue admits what the reference would drop: that, and nothing else, is the difference."""
    frames = [ref.udp_frame(f"192.168.0.{k + 1}", US, 68, 67, bytes([k]) * 5) for k in range(3)]
    one, cells_bytes = ref.lay_out([ref.port_row(US, 67, 1, 40)])
    a, b = both(frames, one, cells_bytes)
    assert same(a, b) and list(a[2]) == [0, ref.FULL, ref.FULL] and a[0]["n_admitted"][0] == 1
    three, cells_bytes = ref.lay_out([ref.port_row(US, 67, 3, 40)])
    a, _ = both(frames, three, cells_bytes)
    assert list(a[2]) == [0, 1, 2]
    for phrase in ("Difference from the reference", "has no queue", "drops a packet while one is", "FS_UDP_FULL are this call's batch form"):
        assert phrase in TEXT, phrase


def test_wrap_and_truncation_numbers():
    ports, cells_bytes = ref.lay_out([ref.port_row(US, 67, 3, 40, wcell=2, free=3)])
    frames = [ref.udp_frame(OTHER, US, 9, 67, bytes([65 + k]) * (7 + k)) for k in range(3)]
    (out, port_of, cell_of, cells), b = both(frames, ports, cells_bytes)
    assert same((out, port_of, cell_of, cells), b)
    assert list(cell_of) == [2, 0, 1] and out[0]["wcell"] == 2 and out[0]["free"] == 0
    assert out[0]["n_truncated"] == 1 and out[0]["bytes"] == 7 + 8 + 8 and out[0]["first"] == 0
    h = cells[40:72].view(UDP_CELL_DTYPE)[0]  # cell 1: the third frame
    assert (h["frame"], h["len"], h["stored"], h["udp_length"], h["src_port"]) == (2, 9, 8, 17, 9)
    assert bytes(h["src_ip"]) == ref.ip4(OTHER) and bytes(h["dst_mac"]) == frames[2][:6]


# ---- the header-only arithmetic under the sanitizers -------------------------------------------------------

def test_udp_arithmetic_under_asan_ubsan():
    out = os.path.join(CSRC, "build", "test_udp")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *SAN, "-o", out, os.path.join(CSRC, "test_udp.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "udp checks OK" in r.stdout


# ---- the eighth header and the binding's tables ------------------------------------------------------------

def params_of(body, name):
    p = body[body.index(name + "(") + len(name) + 1 :]
    return [" ".join(x.split()) for x in p[: p.index(")")].split(",")]


NEW_PARAMS = ["const fs_udp_port* ports", "uint32_t n_ports", "uint8_t* cells", "uint64_t cells_bytes",
              "fs_udp_port_out* ports_out", "uint32_t* port_of", "uint32_t* cell_of"]


def test_udp_prototypes_are_the_headers():
    names = ["fs_udp_flows_batch", "fs_udp_flows_batch_host"]
    assert re.findall(r"^fs_status\s+(fs_\w+)\s*\(", BODY, flags=re.M) == list(abi.UDP_PROTOTYPES) == names
    others = (set(abi.PROTOTYPES) | set(abi.DELIVER_PROTOTYPES) | set(abi.SEND_RINGS_PROTOTYPES) | set(abi.RECV_PROTOTYPES) |
              set(abi.ACCEPT_PROTOTYPES) | set(abi.CLOSE_PROTOTYPES) | set(abi.CONNECT_PROTOTYPES))
    assert not set(abi.UDP_PROTOTYPES) & others and '#include "framesum_connect.h"' in HEADER
    assert len(abi.PROTOTYPES) == 30
    for name, (restype, argtypes) in abi.UDP_PROTOTYPES.items():
        params = params_of(BODY, name)
        assert restype is ctypes.c_int32 and len(params) == len(argtypes) == 56, name
        for p, t in zip(params, argtypes):
            want = ctypes.c_void_p if "*" in p else {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}[p.split()[0]]
            assert t is want, (name, p)
        # every parameter of the connect call up to and including `reply_status`, the seven new ones, the rest
        theirs = params_of(CONNECT_BODY, name.replace("udp", "connect"))
        at = theirs.index("uint8_t* reply_status") + 1
        assert params == theirs[:at] + NEW_PARAMS + theirs[at:]
    lib = framesum.load_library()  # (a library that lacks one of the two symbols raises here)
    for name, (restype, argtypes) in abi.UDP_PROTOTYPES.items():
        assert getattr(lib, name).restype is restype and getattr(lib, name).argtypes == argtypes


C_TYPES = {"uint8_t": 1, "uint16_t": 2, "uint32_t": 4, "uint64_t": 8}


def test_udp_dtypes_and_constants_are_the_headers():
    for name, dtype, mine, size in (("fs_udp_port", UDP_PORT_DTYPE, ref.PORT_DTYPE, 32), ("fs_udp_cell", UDP_CELL_DTYPE, ref.CELL_DTYPE, 32),
                                    ("fs_udp_port_out", UDP_PORT_OUT_DTYPE, ref.PORT_OUT_DTYPE, 32)):
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
    assert int(defines["FS_UDP_NONE"], 16) == abi.UDP_NONE == ref.NONE and int(defines["FS_UDP_FULL"], 16) == abi.UDP_FULL == ref.FULL
    assert int(defines["FS_UDP_MAX_PORTS"]) == abi.UDP_MAX_PORTS == 65536
    assert int(defines["FS_UDP_CELL_HEADER"]) == abi.UDP_CELL_HEADER == ref.HEADER == UDP_CELL_DTYPE.itemsize


def test_null_context_needs_no_device():
    lib = framesum.load_library()
    none = ctypes.c_void_p()
    some = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    tail = (some, 8, some, some, some, none, some, none, none)
    listen = (some, 1, some, 1, 0, some, some, none, some, none, none)
    closing = (some, 1, some, some, none)
    opening = (some, 1, 0, some, some, none, none)
    udp = (some, 1, some, 64, some, none, none)
    assert lib.fs_udp_flows_batch(None, some, some, some, 1, 0, 0, some, 1, some, 64, some, none, some, some, none, *listen,
                                  *closing, *opening, *udp, *tail, none) == -1
    assert lib.fs_udp_flows_batch_host(None, some, 64, some, some, 1, 0, 0, some, 1, some, 64, some, none, some, some, none,
                                       *listen, *closing, *opening, *udp, *tail) == -1


# ---- the host-side helpers ---------------------------------------------------------------------------------

def test_udp_port_split_dgrams_and_ports_after():
    from seqs_amd import ports_after, split_dgrams, udp_port

    rows = [udp_port(US, 67, 3, 40, wcell=2), udp_port("0.0.0.0", 67, 2, 48, free=1)]
    assert rows[0].tobytes() == ref.port_row(US, 67, 3, 40, wcell=2).tobytes()
    ports, cells_bytes = ref.lay_out(rows, lead=8)
    frames = [ref.udp_frame(OTHER, US, 9, 67, bytes([65 + k]) * (7 + k)) for k in range(3)] + \
             [ref.udp_frame(US, OTHER, 10 + k, 67, b"w" * k) for k in range(2)]
    out, port_of, cell_of, cells = ref.expected(frames, ref.verdicts(frames), ports, np.zeros(cells_bytes, dtype=np.uint8))
    got = split_dgrams(cells, ports, out)
    assert [[(int(h["frame"]), p) for h, p in q] for q in got] == [[(0, b"A" * 7), (1, b"B" * 8), (2, b"C" * 8)], [(3, b"")]]
    assert got[1][0][0]["src_port"] == 10 and bytes(got[0][2][0]["src_ip"]) == ref.ip4(OTHER) and got[0][2][0]["len"] == 9
    nxt = ports_after(ports, out)
    assert list(nxt["wcell"]) == [2, 1] and list(nxt["free"]) == [3, 1] and nxt["cells_off"].tobytes() == ports["cells_off"].tobytes()
    nxt = ports_after(ports, out, consumed=[1, 0])
    assert list(nxt["free"]) == [1, 0]
    with pytest.raises(AssertionError):
        ports_after(ports, out, consumed=[4, 0])
