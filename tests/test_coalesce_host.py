"""The RX coalesce (fs_coalesce_batch / fs_coalesce_batch_host) without a GPU: the arithmetic of
seqs_amd/csrc/framesum_coalesce.h under ASan + UBSan (a stand-alone program run as a child process),
the ABI's first argument check through ctypes, the record layouts of the Python and the Go binding
against the header, and the sequential restatement of tests/coalesce_ref.py pinned on small cases."""
import ctypes
import os
import re
import subprocess

import numpy as np

from seqs_amd import framesum

import coalesce_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tests", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
HEADER = open(os.path.join(ROOT, "include", "framesum.h")).read()


def test_coalesce_arithmetic_under_asan_ubsan():
    out = os.path.join(CSRC, "build", "test_coalesce")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *SAN, "-o", out,
                    os.path.join(CSRC, "test_coalesce.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "coalesce checks OK" in r.stdout


def test_argument_checks_need_no_device():
    lib = framesum.load_library()
    none = ctypes.c_void_p()
    some = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    # a null context is FS_E_INVALID before anything else is looked at, with good or bad arguments
    assert lib.fs_coalesce_batch(None, some, some, some, 1, 0, 0, some, 8, some, none, some, none, none, none) == -1
    assert lib.fs_coalesce_batch(None, none, none, none, 0, 0, 7, none, 0, none, none, none, none, none, none) == -1
    assert lib.fs_coalesce_batch_host(None, some, 64, some, some, 1, 0, 0, some, 8, some, none, some, none, none) == -1
    assert lib.fs_coalesce_batch_host(None, none, 0, none, none, 0, 0, 7, none, 0, none, none, none, none, none) == -1


def struct_fields(name):
    body = HEADER[HEADER.index("typedef struct " + name) : HEADER.index("} " + name + ";")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(uint\d+_t)\s+([a-z_]+)(?:\[(\d+)\])?;", body)


def test_run_dtype_is_the_c_struct():
    d = framesum.RUN_DTYPE
    assert d.itemsize == 24
    fields = struct_fields("fs_rx_run")
    assert [f[1] for f in fields] == list(d.names) == ["payload_off", "payload_len", "first_frame", "n_frames",
                                                       "tcp_flags", "reserved"]
    at = 0
    for ctype, name, count in fields:  # natural alignment leaves no padding: the offsets are the running sum
        size = int(ctype[4:-2]) // 8
        assert d.fields[name][1] == at and at % size == 0, name
        at += size * int(count or 1)
    assert at == 24
    t = framesum.TOTALS_DTYPE
    assert t.itemsize == 16 and [f[1] for f in struct_fields("fs_rx_totals")] == list(t.names)
    assert [t.fields[k][1] for k in t.names] == [0, 8, 12]
    assert re.search(r"#define FS_RX_FCS (\d+)u", HEADER).group(1) == str(framesum.RX_FCS)
    assert framesum.NO_RUN == ref.NO_RUN == 0xFFFFFFFF and ref.RX_FCS == framesum.RX_FCS


def test_go_file_declares_coalesce_batch():
    eth = open(os.path.join(ROOT, "go", "eth", "digest_gpu.go")).read()
    for sym in ("func (g *GPU) CoalesceBatch(", "C.fs_coalesce_batch_host(", "type Run struct", "C.FS_RX_FCS",
                "C.fs_rx_run", "C.fs_rx_totals"):
        assert sym in eth, sym
    # CoalesceBatch stands beside SegmentBatch, in the same build-tagged file
    assert eth.startswith("//go:build framesum")
    assert eth.index("func (g *GPU) SegmentBatch(") < eth.index("func (g *GPU) CoalesceBatch(")
    # the fields of fs_rx_run and fs_rx_totals it reads are the header's
    run_fields = {f[1] for f in struct_fields("fs_rx_run")}
    used = set(re.findall(r"cr\[i\]\.([a-z_]+)", eth))
    assert used and used <= run_fields, used
    assert set(re.findall(r"totals\.([a-z_]+)", eth)) <= {f[1] for f in struct_fields("fs_rx_totals")}
    # the call passes as many arguments as the header declares
    decl = HEADER[HEADER.index("fs_status fs_coalesce_batch_host(") :]
    decl = decl[: decl.index(");")]
    call = eth[eth.index("C.fs_coalesce_batch_host(") :]
    depth, end = 0, 0
    for end, ch in enumerate(call):
        depth += ch == "("
        depth -= ch == ")"
        if depth == 0 and ch == ")":
            break
    args, depth, count = call[len("C.fs_coalesce_batch_host(") : end], 0, 1
    for ch in args:
        depth += ch == "("
        depth -= ch == ")"
        count += ch == "," and depth == 0
    assert count == decl.count(",") + 1 == 15


def test_scan_block_is_exported():
    B = ref.scan_block()
    assert B >= 64 and B % 64 == 0


def test_restatement_on_small_cases(oracle_lib):
    rng = np.random.default_rng(1)
    hdr = ref.flow_header(rng)
    frames = ref.segments(rng, hdr, (1 << 32) - 50, [100, 37, 1], last_flags=ref.ACK | ref.PSH)
    frames.append(ref.udp_frame(rng, b"abcdefg", pad=11))
    frames += ref.segments(rng, hdr, 88, [0])  # a pure ACK
    frames += ref.segments(rng, ref.flow_header(rng, 0x99), 5, [10, 20], pad_to=60)
    frames = ref.finish(frames)
    bad = bytearray(frames[5])
    bad[54] ^= 1
    frames[5] = bytes(bad)
    for lead, fcs in ((0, False), (3, True)):
        fr = [f + framesum_crc(f) for f in frames] if fcs else frames
        buf, off, ln = ref.pack(fr, lead)
        noise = np.random.default_rng(2).integers(0, 256, 400, dtype=np.uint8)
        e = ref.expected(buf, off, ln, 0, ref.RX_FCS if fcs else 0, noise, 5, 200)
        assert list(e["st"]) == [0, 0, 0, 0, 0, 13, 0]
        assert [(int(r["first_frame"]), int(r["n_frames"]), int(r["payload_off"]), int(r["payload_len"]),
                 int(r["tcp_flags"])) for r in e["runs"]] == \
            [(0, 3, 0, 138, ref.ACK | ref.PSH), (3, 1, 138, 7, 0), (4, 1, 145, 0, ref.ACK), (6, 1, 145, 20, ref.ACK)]
        assert list(e["run_of"]) == [0, 0, 0, 1, 2, ref.NO_RUN, 3] and (e["payload_bytes"], e["n_runs"]) == (165, 4)
        want = b"".join(f[54:54 + n] for f, n in zip(frames[:3], (100, 37, 1))) + b"abcdefg" + frames[6][54:74]
        assert e["payload"][5:170].tobytes() == want
        assert np.array_equal(e["payload"][:5], noise[:5]) and np.array_equal(e["payload"][170:], noise[170:])
        # a cap inside the second frame's payload: it and the later frames stay out, the rest is the same
        c = ref.expected(buf, off, ln, 0, ref.RX_FCS if fcs else 0, noise, 5, 120)
        assert c["payload"][5:105].tobytes() == want[:100] and np.array_equal(c["payload"][105:], noise[105:])
        assert c["runs"].tobytes() == e["runs"].tobytes() and c["payload_bytes"] == 165


def framesum_crc(f: bytes) -> bytes:
    import zlib

    return zlib.crc32(f).to_bytes(4, "little")


def test_known_answer_frames_are_runs_of_their_own(oracle_lib):
    frames = ref.kat_frames()
    buf, off, ln = ref.pack(frames, 2)
    e = ref.expected(buf, off, ln, 0, 0, np.zeros(int(ln.sum()), dtype=np.uint8))
    ok = [i for i in range(len(frames)) if e["st"][i] == 0]
    assert len(ok) >= 2 and e["n_runs"] >= 2
    at = 0
    for r in e["runs"]:
        f = frames[int(r["first_frame"])]
        s, end = ref.payload_range(f)
        assert int(r["payload_off"]) == at
        if int(r["n_frames"]) == 1:
            assert e["payload"][at : at + end - s].tobytes() == f[s:end]
        at += int(r["payload_len"])
    assert at == e["payload_bytes"]
