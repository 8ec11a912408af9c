"""The builders of tests/test_gpu_coalesce_edges.py and tests/test_gpu_segment_sweep.py, run through the
references alone (no GPU): the conditions without which those GPU tests would pass vacuously (the
frames are accepted, the options are there, every verdict occurs, the loops take the turns they are
meant to), and the new helpers of tests/coalesce_ref.py on small cases."""
import numpy as np

import coalesce_ref as ref
import segment_ref as sref
import test_gpu_coalesce_edges as ce
import test_gpu_segment_sweep as ss
from oracle import coracle


def reference(frames, mtu=0, flags=0, lead=0):
    buf, off, ln = ref.pack(frames, lead)
    return ref.expected(buf, off, ln, mtu, flags, np.zeros(int(ln.sum()) + 8, dtype=np.uint8))


def runs_of(e):
    return [(int(r["first_frame"]), int(r["n_frames"])) for r in e["runs"]]


# ---- the helpers ---------------------------------------------------------------------------------

def test_tcp_frame_with_ip_options(oracle_lib):
    rng = np.random.default_rng(1)
    hdr = ref.flow_header(rng)
    plain = ref.tcp_frame(hdr, 5, b"abc", ref.ACK, 9, ce.NOP4)
    f = ref.tcp_frame(hdr, 5, b"abc", ref.ACK, 9, ce.NOP4, ip_options=2 * ce.NOP4)
    assert f[14] == 0x47 and int.from_bytes(f[16:18], "big") == 20 + 8 + 24 + 3 == len(f) - 14
    assert f[:14] == plain[:14] and f[18:34] == plain[18:34] and f[34:42] == 2 * ce.NOP4 and f[42:] == plain[34:]
    assert ref.payload_range(f) == (14 + 28 + 24, len(f)) and f[66:] == b"abc"
    e = reference(ref.finish([f, plain]))
    assert list(e["st"]) == [0, 0] and list(e["runs"]["tcp_flags"]) == [ref.ACK, ref.ACK]
    assert ref.tcp_frame(hdr, 5, b"abc", ref.ACK, 9, ce.NOP4, ip_options=b"") == plain


def test_pack_at():
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (5, 0, 9, 1)]
    buf, off, ln = ref.pack_at(frames, [2, 0, 3, 1], [3, 0, 7, 2], seed=1, tail=6)
    assert list(off) == [12, 27, 3, 24] and list(ln) == [5, 0, 9, 1] and buf.size == 15 + 12 + 6
    assert off.dtype == np.uint64 and ln.dtype == np.uint32
    for f, o in zip(frames, off):
        assert buf[int(o) : int(o) + len(f)].tobytes() == f
    noise = ref.pack_at([b""] * 4, range(4), [0] * 4, seed=1, tail=33)[0]  # (the same generator, no frames)
    free = np.ones(buf.size, dtype=bool)
    for f, o in zip(frames, off):
        free[int(o) : int(o) + len(f)] = False
    assert np.array_equal(buf[free], noise[free]) and len(set(buf[free].tolist())) > 8


def test_with_fcs(oracle_lib):
    frames = ce.verdict_batch(1)[:40]
    out = ref.with_fcs(frames, [3, 17])
    import zlib

    for i, (f, g) in enumerate(zip(frames, out)):
        assert g[: len(f)] == f and len(g) == len(f) + 4  # (checksum fields as they were: nothing refilled)
        diff = int.from_bytes(g[len(f) :], "little") ^ zlib.crc32(f)
        assert (bin(diff).count("1") == 1) if i in (3, 17) else diff == 0
    e = reference(out, flags=ref.RX_FCS)
    plain = reference(frames)
    assert e["st"][3] == e["st"][17] == ce.FS_ERR_FCS
    rest = [i for i in range(40) if i not in (3, 17)]
    assert np.array_equal(e["st"][rest], plain["st"][rest])


# ---- the coalesce builders -----------------------------------------------------------------------

def test_grid_is_accepted_whole(oracle_lib):
    frames, what = ce.grid_frames()
    assert len(frames) == 396 and len(set(what)) == 396
    e = reference(frames)
    assert (e["st"] == 0).all() and e["n_runs"] == 396 and e["payload_bytes"] == 132 * 38
    starts = [ref.payload_range(f)[0] for f in frames]
    assert max(starts) == 134 and min(starts) == 42
    assert {(f[14] & 15, f[14 + 4 * (f[14] & 15) + 12] >> 4) for f, w in zip(frames, what) if w[0] == 6} == \
        {(i, t) for i in range(5, 16) for t in range(5, 16)}
    # over the rotations every frame sits at a wave's first lane and at its last
    for j in range(396):
        at = {(j - r) % 396 % 64 for r in range(ce.GRID_ROTATIONS)}
        assert {0, 63} <= at, j
    assert ce.rotated([0, 1, 2, 3], 1) == [1, 2, 3, 0]


def test_verdict_batches_hold_what_they_are_for(oracle_lib):
    for seed in ce.VERDICT_SEEDS:
        frames = ce.verdict_batch(seed)
        e = reference(frames, lead=seed)
        ok = [f for f, v in zip(frames, e["st"]) if v == 0]
        assert sum(f[23] == 6 and f[14] & 15 > 5 for f in ok) >= 25
        assert sum(f[23] == 17 and f[14] & 15 > 5 for f in ok) >= 25
        assert set(e["st"].tolist()) == {0, 1} | set(range(3, 14))
        assert set(ce.spliced_runs()) <= set(runs_of(e)) and e["st"][ce.SPLICE_AT[1] + 2] == 5
        capped = reference(frames, mtu=1514)
        assert 2 in capped["st"] and set(ce.spliced_runs()) <= set(runs_of(capped))
        assert max(len(f) for f in frames) >= 9000 and min(len(f) for f in frames) == 0


def test_fcs_batch_has_good_and_damaged_frames(oracle_lib):
    frames, damaged = ce.fcs_batch()
    e = reference(frames, flags=ref.RX_FCS)
    plain = reference(ce.verdict_batch(1))
    assert (e["st"][damaged] == ce.FS_ERR_FCS).all() and (plain["st"][damaged] == 0).sum() >= 10
    assert (e["st"] == 0).sum() >= 100 and ce.FS_ERR_FCS not in np.delete(e["st"], damaged)
    assert e["payload_bytes"] < plain["payload_bytes"] and max(n for _, n in runs_of(e)) > 1


def test_order_cases_keep_the_batch(oracle_lib):
    frames = ce.six_run()
    for name, buf, off, ln in ce.order_cases(frames, 2):
        got = [buf[int(o) : int(o) + int(n)].tobytes() for o, n in zip(off, ln)]
        assert got == (frames[:3] + frames[2:] if name == "twice" else frames), name
        e = ref.expected(buf, off, ln, 0, 0, np.zeros(1000, dtype=np.uint8))
        assert runs_of(e) == ([(0, 3), (3, 4)] if name == "twice" else [(0, 6)])
        if name == "reverse":
            assert (np.diff(off.astype(np.int64)) < 0).all()
        if name == "random":
            assert (np.diff(off.astype(np.int64)) < 0).any() and (np.diff(off.astype(np.int64)) > 0).any()


def test_boundary_cases_split_where_they_should(oracle_lib):
    b = 64
    for case in ce.SPLITS:
        e = reference(ce.boundary_case(b, case))
        assert e["run_of"][b] != e["run_of"][b - 1], case
        assert e["run_of"][b] != ref.NO_RUN and e["run_of"][b + 1] != ref.NO_RUN, case
        # ... and nowhere else before: one run up to the altered frame
        assert runs_of(e)[0] == (0, b if case in ("seq", "byte0", "byte53", "ece", "psh", "syn") else b - 1), case
        assert e["n_runs"] == (2 if case in ("psh", "damaged") else 3), case
    assert runs_of(reference(ce.boundary_case(b, "control"))) == [(0, b + 2)]
    st = reference(ce.boundary_case(b, "damaged"))["st"]
    assert st[b - 1] == 13 and (np.delete(st, b - 1) == 0).all()
    assert len(ce.boundary_case(b, "udp42")[b - 1]) == 42
    f = ce.boundary_case(b, "ihl6")[b - 1]
    assert f[14] == 0x46 and f[50] >> 4 == 5
    assert ce.boundary_case(b, "doff6")[b - 1][46] >> 4 == 6 and len(ce.boundary_case(b, "ack")[b - 1]) == 54


def test_scan_carry_cases_need_a_second_turn(oracle_lib):
    B = ref.scan_block()
    frames = ce.carry_frames()
    n = len(frames)
    assert n == B * B + B + 1 and -(-n // B) == B + 2 > B
    assert 60 <= min(map(len, frames)) and max(map(len, frames)) <= 80
    e = reference(frames)
    assert runs_of(e) == [(0, n)]
    d = reference(ce.damaged_first_turn(frames))
    assert runs_of(d) == [(B * B, B + 1)] and (d["st"][: B * B] == 13).all()  # nothing accepted in the first B blocks


def test_body_frames(oracle_lib):
    frames = ce.body_frames()
    e = reference(frames)
    m = len(ce.BODY_LENGTHS)
    assert m == 46 and list(e["st"]) == [0] * m + [7, 7, 0, 0]
    assert [int(x) for x in e["runs"]["payload_len"]] == ce.BODY_LENGTHS + [65481, 65493]
    assert [int.from_bytes(f[16:18], "big") for f in frames[m:]] == [65535, 65535, 65521, 65521]
    # one more byte of TotalLength and RecvEth's uint16 `end` wraps: these are the longest payloads
    f = bytearray(frames[-1]) + b"\0"
    f[16:18] = (65522).to_bytes(2, "big")
    assert coracle.recv_eth(bytes(f))[0] == 7
    for pieces in (32, 33, 48, 49, 64, 65):  # a body of that many 16-byte pieces at some destination alignment
        assert any(ref_body(n, a) == pieces for n in ce.BODY_LENGTHS for a in range(16))


def ref_body(n, align):
    head = min(n, -align % 16)
    return (n - head) // 16


def test_cap_frames(oracle_lib):
    frames = ce.cap_frames()
    e = reference(frames)
    assert (e["st"] == 0).all() and [int(x) for x in e["runs"]["payload_len"]] == ce.CAP_SIZES
    assert [f[23] for f in frames] == [6, 6, 17, 6, 6, 6]


# ---- the segment builders ------------------------------------------------------------------------

def test_sweep_takes_every_turn_count_and_lane(oracle_lib):
    specs, payload = ss.sweep_specs()
    assert len(specs) == 3153 and [s[2] for s in specs] == list(range(3153))
    assert {ss.turns(s[2]) for s in specs} == {0, 1, 2, 3, 4}
    assert (ss.turns(1), ss.turns(1024), ss.turns(1025), ss.turns(2048), ss.turns(2049), ss.turns(3073)) == (1, 1, 2, 2, 3, 4)
    # with three turns and more: every length of the short first piece in every lane
    assert {(C % 16, (-(-C // 16) - 1) % 64) for _, _, C, _ in specs if ss.turns(C) >= 3 and C % 16} >= \
        {(m, lane) for m in range(1, 16) for lane in range(64)}
    assert {s[0][23] for s in specs[0::2]} == {6} and {s[0][23] for s in specs[1::2]} == {17}
    assert all(at == C % 61 and at + C <= payload.size for _, at, C, _ in specs)
    noise = np.zeros(6 << 20, dtype=np.uint8)
    _, _, lens, _, st = sref.expected(specs, payload, 0, sref.FCS_APPEND, 1, noise)
    assert (st == 0).all() and lens.size == 3153


def test_large_mss_and_search_specs(oracle_lib):
    specs, payload = ss.large_mss_specs()
    assert len(specs) == 20 and all(sref.n_frames(mss, L) == 3 for _, _, L, mss in specs)
    assert all(at + L <= payload.size for _, at, L, _ in specs)
    assert {L - 2 * mss for _, _, L, mss in specs if L < 3 * mss - 1} == {1, 15}
    _, _, lens, _, st = sref.expected(specs, payload, 0, 0, 64, np.zeros(1 << 20, dtype=np.uint8))
    assert (st == 0).all() and lens.max() == 54 + 8946
    for n in ss.SEARCH_SENDS:
        for long_first in (False, True):
            specs, payload = ss.search_specs(n, long_first)
            assert len(specs) == n and all(at + L <= payload.size for _, at, L, _ in specs)
            assert sum(sref.n_frames(mss, L) for _, _, L, mss in specs) == n + (69 if long_first else 0)
