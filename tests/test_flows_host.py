"""The flow-aware RX coalesce (fs_coalesce_flows_batch / fs_coalesce_flows_batch_host) without a GPU:
the arithmetic of seqs_amd/csrc/framesum_flows.h under ASan + UBSan (a stand-alone program run as a
child process), the ABI's argument checks through ctypes, the record layouts of the Python and the Go
binding against the header, and the sequential restatement of tests/flows_ref.py pinned on a
hand-computed case and on its equivalence with tests/coalesce_ref.py."""
import ctypes
import os
import re
import subprocess

import numpy as np

from seqs_amd import framesum

import coalesce_ref as cref
import flows_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tests", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
HEADER = open(os.path.join(ROOT, "include", "framesum.h")).read()


def test_flows_arithmetic_under_asan_ubsan():
    out = os.path.join(CSRC, "build", "test_flows")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *SAN, "-o", out, os.path.join(CSRC, "test_flows.cpp")],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "flows checks OK" in r.stdout


def test_argument_checks_need_no_device():
    lib = framesum.load_library()
    none = ctypes.c_void_p()
    some = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    # a null context is FS_E_INVALID before anything else is looked at, with good or bad arguments
    assert lib.fs_coalesce_flows_batch(None, some, some, some, 1, 0, 0, some, 8, some, some, some, none, some, none, none,
                                       none) == -1
    assert lib.fs_coalesce_flows_batch(None, none, none, none, 0, 0, 7, none, 0, none, none, none, none, none, none, none,
                                       none) == -1
    assert lib.fs_coalesce_flows_batch_host(None, some, 64, some, some, 1, 0, 0, some, 8, some, some, some, none, some,
                                            none, none) == -1
    assert lib.fs_coalesce_flows_batch_host(None, none, 0, none, none, 0, 0, 7, none, 0, none, none, none, none, none,
                                            none, none) == -1


def struct_fields(name):
    body = HEADER[HEADER.index("typedef struct " + name) : HEADER.index("} " + name + ";")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for ctype, names in re.findall(r"(uint\d+_t)\s+([a-z_, ]+);", body):
        out += [(ctype, nm.strip()) for nm in names.split(",")]
    return out


def test_flow_dtypes_are_the_c_structs():
    for name, dtype, size in (("fs_rx_flow", framesum.FLOW_DTYPE, 32), ("fs_rx_flow_totals", framesum.FLOW_TOTALS_DTYPE, 24)):
        fields = struct_fields(name)
        assert [f[1] for f in fields] == list(dtype.names), name
        at = 0
        for ctype, nm in fields:  # natural alignment leaves no padding: the offsets are the running sum
            width = int(ctype[4:-2]) // 8
            assert dtype.fields[nm][1] == at and at % width == 0 and dtype.fields[nm][0].itemsize == width, nm
            at += width
        assert at == dtype.itemsize == size
    assert list(framesum.FLOW_DTYPE.names) == ["payload_off", "payload_len", "first_run", "n_runs", "first_frame", "n_frames"]
    assert list(framesum.FLOW_TOTALS_DTYPE.names) == ["payload_bytes", "n_runs", "n_flows", "n_accepted", "reserved"]
    for sym in ("fs_coalesce_flows_batch", "fs_coalesce_flows_batch_host"):
        assert sym in framesum.EXPORTED_SYMBOLS


def call_args(text, name):
    """How many arguments the first call (or declaration) of `name(` in `text` has."""
    call = text[text.index(name + "(") :]
    depth, end = 0, 0
    for end, ch in enumerate(call):
        depth += ch == "("
        depth -= ch == ")"
        if depth == 0 and ch == ")":
            break
    args, depth, count = call[len(name) + 1 : end], 0, 1
    for ch in args:
        depth += ch == "("
        depth -= ch == ")"
        count += ch == "," and depth == 0
    return count


def test_go_file_declares_coalesce_flows_batch():
    eth = open(os.path.join(ROOT, "go", "eth", "digest_gpu.go")).read()
    for sym in ("func (g *GPU) CoalesceFlowsBatch(", "type Flow struct", "C.fs_coalesce_flows_batch_host(", "C.fs_rx_flow",
                "C.fs_rx_flow_totals"):
        assert sym in eth, sym
    assert eth.index("func (g *GPU) CoalesceBatch(") < eth.index("type Flow struct") < \
        eth.index("func (g *GPU) CoalesceFlowsBatch(")
    # the fields of fs_rx_flow and fs_rx_flow_totals it reads are the header's
    used = set(re.findall(r"cf\[i\]\.([a-z_]+)", eth))
    assert used and used <= {f[1] for f in struct_fields("fs_rx_flow")}, used
    used = set(re.findall(r"\bft\.([a-z_]+)", eth))
    assert used and used <= {f[1] for f in struct_fields("fs_rx_flow_totals")}, used
    # the call passes as many arguments as the header declares
    assert call_args(eth, "C.fs_coalesce_flows_batch_host") == call_args(HEADER, "fs_status fs_coalesce_flows_batch_host") == 17
    assert call_args(HEADER, "fs_status fs_coalesce_flows_batch") == 17


def hand_case():
    """A0 B0 A1 bad B1 U A2: two TCP flows interleaved, a damaged frame of flow A that carries none
    of its in-order bytes, and a UDP frame."""
    rng = np.random.default_rng(11)
    ha, hb = ref.flow_header(rng, 0x1111), ref.flow_header(rng, 0x2222)
    a = ref.segments(rng, ha, 1000, [100, 37, 20])
    b = ref.segments(rng, hb, 5, [10, 20])
    bad = ref.segments(rng, ha, 900000, [33])
    u = ref.udp_frame(rng, b"abcdefg", pad=11)
    frames = ref.finish([a[0], b[0], a[1], bad[0], b[1], u, a[2]])
    damaged = bytearray(frames[3])
    damaged[60] ^= 1
    frames[3] = bytes(damaged)
    return frames


def records(arr):
    return [tuple(int(r[k]) for k in arr.dtype.names if k != "reserved") for r in arr]


def test_restatement_on_the_hand_computed_case(oracle_lib):
    frames = hand_case()
    for lead, fcs in ((0, False), (3, True)):
        fr = [f + zlib_crc(f) for f in frames] if fcs else frames
        buf, off, ln = ref.pack(fr, lead)
        noise = np.random.default_rng(2).integers(0, 256, 400, dtype=np.uint8)
        e = ref.expected(buf, off, ln, 0, ref.RX_FCS if fcs else 0, noise, 5, 250)
        assert list(e["st"]) == [0, 0, 0, 13, 0, 0, 0]
        assert list(e["order"]) == [0, 2, 6, 1, 4, 5]
        # runs: (payload_off, payload_len, first_frame = index into order, n_frames, tcp_flags)
        assert records(e["runs"]) == [(0, 157, 0, 3, ref.ACK), (157, 30, 3, 2, ref.ACK), (187, 7, 5, 1, 0)]
        # flows: (payload_off, payload_len, first_run, n_runs, first_frame, n_frames)
        assert records(e["flows"]) == [(0, 157, 0, 1, 0, 3), (157, 30, 1, 1, 3, 2), (187, 7, 2, 1, 5, 1)]
        assert list(e["run_of"]) == [0, 1, 0, ref.NO_RUN, 1, 2, 0]
        assert (e["payload_bytes"], e["n_runs"], e["n_flows"], e["n_accepted"]) == (194, 3, 3, 6)
        want = (frames[0][54:154] + frames[2][54:91] + frames[6][54:74] + frames[1][54:64] + frames[4][54:74] + b"abcdefg")
        assert e["payload"][5:199].tobytes() == want
        assert np.array_equal(e["payload"][:5], noise[:5]) and np.array_equal(e["payload"][199:], noise[199:])
        # a cap inside A2's payload: it stays out, and so does every frame behind it that does not fit
        c = ref.expected(buf, off, ln, 0, ref.RX_FCS if fcs else 0, noise, 5, 150)
        assert c["payload"][5:142].tobytes() == want[:137] and np.array_equal(c["payload"][142:], noise[142:])
        assert c["runs"].tobytes() == e["runs"].tobytes() and c["flows"].tobytes() == e["flows"].tobytes()
        assert c["payload_bytes"] == 194
    # the same frames through the frame-before-it rule: every frame a run of its own
    buf, off, ln = ref.pack(frames, 0)
    assert cref.expected(buf, off, ln, 0, 0, np.zeros(400, dtype=np.uint8))["n_runs"] == 6


def zlib_crc(f: bytes) -> bytes:
    import zlib

    return zlib.crc32(f).to_bytes(4, "little")


def contiguous_batch(seed, damage=False):
    """Flows one after the other: runs of several segments, UDP, a pure ACK, TCP with options, a run
    cut by PSH. `damage`: one frame between two flows is damaged."""
    rng = np.random.default_rng(seed)
    frames = ref.segments(rng, ref.flow_header(rng, 0x100), (1 << 32) - 50, [100, 37, 1])
    frames.append(ref.udp_frame(rng, b"0123456789", pad=3))
    frames += ref.segments(rng, ref.flow_header(rng, 0x101), 7, [0])
    if damage:
        frames += ref.segments(rng, ref.flow_header(rng, 0x102), 70, [25])
    hdr = ref.flow_header(rng, 0x103)
    frames += ref.segments(rng, hdr, 500, [64, 64], last_flags=ref.ACK | ref.PSH)
    frames += ref.segments(rng, hdr, 628, [9])
    frames.append(ref.tcp_frame(ref.flow_header(rng, 0x104), 1, b"with options", options=b"\x01\x01\x01\x01"))
    frames = ref.finish(frames)
    if damage:
        d = bytearray(frames[5])
        d[56] ^= 4
        frames[5] = bytes(d)
    return frames


def test_restatement_equals_the_frame_before_rule_on_contiguous_flows(oracle_lib):
    for seed in range(4):
        frames = contiguous_batch(seed)
        buf, off, ln = ref.pack(frames, seed)
        noise = np.random.default_rng(seed).integers(0, 256, 600, dtype=np.uint8)
        for cap in (None, 140):
            e = ref.expected(buf, off, ln, 0, 0, noise, 3, cap)
            c = cref.expected(buf, off, ln, 0, 0, noise, 3, cap)
            assert np.array_equal(e["payload"], c["payload"]) and e["runs"].tobytes() == c["runs"].tobytes()
            assert np.array_equal(e["run_of"], c["run_of"]) and e["n_runs"] == c["n_runs"] == 6
            assert list(e["order"]) == list(range(len(frames))) and e["n_flows"] == 5
        # with a rejected frame between two flows a run's first_frame counts the accepted frames only
        frames = contiguous_batch(seed, damage=True)
        buf, off, ln = ref.pack(frames, seed)
        e = ref.expected(buf, off, ln, 0, 0, noise, 3)
        c = cref.expected(buf, off, ln, 0, 0, noise, 3)
        assert e["st"][5] == 13 and list(e["order"]) == [0, 1, 2, 3, 4, 6, 7, 8, 9]
        assert np.array_equal(e["payload"], c["payload"]) and np.array_equal(e["run_of"], c["run_of"])
        mapped = e["runs"].copy()
        mapped["first_frame"] = e["order"][e["runs"]["first_frame"]]
        assert mapped.tobytes() == c["runs"].tobytes()
