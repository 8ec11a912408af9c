"""The TX frame build (fs_segment_layout / fs_segment_batch) without a GPU: the host arithmetic of
seqs_amd/csrc/framesum_segment.h under ASan + UBSan (a stand-alone program run as a child process),
fs_segment_layout against the Python restatement, the ABI's argument checks (they run before any
device call), and the restatement itself pinned on the reference's known-answer frames."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from seqs_amd import framesum

import segment_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tests", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def test_segment_arithmetic_under_asan_ubsan():
    out = os.path.join(CSRC, "build", "test_segment")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *SAN, "-o", out,
                    os.path.join(CSRC, "test_segment.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "segment checks OK" in r.stdout


def random_specs(rng, n):
    specs, at = [], 0
    for _ in range(n):
        if rng.integers(0, 4) == 0:
            hdr, mss, ln = ref.udp_header(rng), 0, int(rng.integers(0, 1473))
        else:
            hdr, mss = ref.tcp_header(rng), int(rng.choice([0, 1, 2, 63, 64, 65, 536, 1446, 1460]))
            ln = int(rng.integers(0, 40 if mss in (1, 2) else 6000))
        specs.append((hdr, at, ln, mss))
        at += ln
    return specs, at


def test_layout_agrees_with_restatement():
    rng = np.random.default_rng(11)
    for _ in range(200):
        specs, _ = random_specs(rng, int(rng.integers(1, 12)))
        flags, align = int(rng.choice([0, 2])), int(rng.choice([1, 2, 4, 64, 4096]))
        lens = [len(h) + (min(mss, ln - k * mss) if mss else ln)
                for h, _, ln, mss in specs for k in range(ref.n_frames(mss, ln))]
        _, total = ref.layout(lens, flags, align)
        assert framesum.segment_layout(ref.make_sends(specs), flags, align) == (len(lens), total)
    assert framesum.segment_layout(np.zeros(0, dtype=framesum.SEND_DTYPE), 0, 4) == (0, 0)


def test_layout_beyond_4_gib():
    # the layout tests/test_gpu_large_offsets.py builds on the device: its slots pass 2^32
    from test_gpu_large_offsets import big_layout

    for flags in (0, 2):
        sends, lens, offs, total, first, _ = big_layout(flags)
        assert total > 1 << 32 and int(offs.max()) >= 1 << 32
        assert framesum.segment_layout(sends, flags, 4096) == (lens.size, total)
        # the per-send bases are exact: the layout of the first k sends ends where send k begins
        for k in (1, int(np.searchsorted(offs[first[:-1]], 1 << 32)), sends.size - 1):
            assert framesum.segment_layout(sends[:k], flags, 4096) == (int(first[k]), int(offs[first[k]]))
            assert int(offs[first[k]]) == int(first[k]) * 4096
        k = int(np.searchsorted(offs[first[:-1]], 1 << 32))
        assert int(offs[first[k - 1]]) < 1 << 32 <= int(offs[first[k]])
    # with align 1 the same sends stay far below 2^32: the slots, not the bytes, carry the layout up
    assert framesum.segment_layout(sends, 0, 1)[1] == int(lens.sum()) < 1 << 28


def test_send_dtype_is_the_c_struct():
    d = framesum.SEND_DTYPE
    assert d.itemsize == 72
    assert [d.fields[k][1] for k in ("hdr", "mss", "payload_off", "payload_len", "reserved")] == [0, 54, 56, 64, 68]


def test_argument_checks_need_no_device():
    lib = framesum.load_library()
    rng = np.random.default_rng(3)
    sends = ref.make_sends([(ref.tcp_header(rng), 0, 1000, 100)])
    p, none = sends.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p()
    n, b = ctypes.c_uint64(), ctypes.c_uint64()
    # a null context fails before anything else is looked at
    assert lib.fs_segment_batch(None, p, 1, none, 1000, 0, 0, 4, none, 0, none, none, none, none, none) == -1
    assert lib.fs_segment_batch_host(None, p, 1, none, 1000, 0, 0, 4, none, 0, none, none, none, none) == -1
    assert lib.fs_segment_layout(p, 1, 0, 4, ctypes.byref(n), ctypes.byref(b)) == 0 and (n.value, b.value) == (10, 1560)
    assert lib.fs_segment_layout(None, 1, 0, 4, ctypes.byref(n), ctypes.byref(b)) == -1
    for flags, align in ((1, 4), (4, 4), (0, 0), (0, 3), (0, 8192)):
        assert lib.fs_segment_layout(p, 1, flags, align, ctypes.byref(n), ctypes.byref(b)) == -1, (flags, align)
        assert lib.fs_segment_layout(p, 0, flags, align, ctypes.byref(n), ctypes.byref(b)) == -1, (flags, align)

    def bad(edit):
        s = sends.copy()
        edit(s)
        with pytest.raises(framesum.FramesumError):
            framesum.segment_layout(s)

    bad(lambda s: s["reserved"].__setitem__(0, 1))
    bad(lambda s: s["hdr"].__setitem__((0, 13), 6))     # EtherType
    bad(lambda s: s["hdr"].__setitem__((0, 14), 0x46))  # IHL
    bad(lambda s: s["hdr"].__setitem__((0, 23), 1))     # protocol
    bad(lambda s: s["hdr"].__setitem__((0, 46), 0x60))  # data offset
    bad(lambda s: (s["hdr"].__setitem__((0, 23), 17), s["mss"].__setitem__(0, 8)))  # UDP with mss
    bad(lambda s: (s["mss"].__setitem__(0, 0), s["payload_len"].__setitem__(0, 65496)))
    bad(lambda s: (s["mss"].__setitem__(0, 1), s["payload_len"].__setitem__(0, 4097)))


def test_prand16_pinned():
    assert ref.prand16(1) == 0x8181
    x, seen = 1, set()
    for _ in range(4096):
        seen.add(x)
        x = ref.prand16(x)
    assert len(seen) == 4096 and 0 not in seen  # no short cycle on the way to the longest send


def test_restatement_gives_the_known_answer_frames_back(oracle_lib):
    frames, specs, payload = ref.kat_sends()
    assert len(frames) >= 2 and {f[23] for f in frames} == {6, 17}
    for flags in (0, 2):
        for align in (1, 64):
            noise = np.random.default_rng(5).integers(0, 256, 4096, dtype=np.uint8)
            buf, off, ln, dig, st = ref.expected(specs, payload, 0, flags, align, noise)
            for f, o, n in zip(frames, off, ln):
                assert buf[int(o) : int(o) + int(n)].tobytes() == f
            assert (st == 0).all()
            # nothing outside the frames (and their FCS) moved
            mask = np.ones(noise.size, dtype=bool)
            for o, n in zip(off, ln):
                mask[int(o) : int(o) + int(n) + (4 if flags else 0)] = False
            assert np.array_equal(buf[mask], noise[mask])
