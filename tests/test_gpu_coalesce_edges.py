"""The RX coalesce on the GPU at the shapes tests/test_gpu_coalesce.py leaves out: IP options (the
classify step's read of the TCP bytes beyond the 54-byte header) and payload starts up to 134, every
verdict between runs, frames whose memory order is not the batch order, the join rule where the frame
before is re-classified by a wave's first lane, more scan blocks than one turn of the partials scan
takes, copy bodies at the boundaries of the four pieces in flight, the longest payloads, payload_cap
at every value, and the context's scratch reused without a sync. Same method as there: the WHOLE
payload buffer byte for byte, runs, run_of, totals, digests and verdicts against
tests/coalesce_ref.py + the C oracle. The builders (no GPU needed) are also run by
tests/test_edge_case_builders.py, which asserts that they reach the cases they are meant to."""
import functools
import random

import numpy as np
import pytest

import coalesce_ref as ref
import engines
import framegen
from test_gpu_coalesce import TAIL, alternating_runs, base_specs, compare, long_run, run_list

pytestmark = pytest.mark.gpu

ACK, FIN, SYN, PSH, ECE = ref.ACK, ref.FIN, ref.SYN, ref.PSH, 0x40
NOP4 = b"\x01\x01\x01\x01"
FS_ERR_FCS = 14


@pytest.fixture(scope="module")
def eng():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()  # (torch's runtime first, as in the other GPU suites)
    e = Engine(0)
    yield e
    e.close()


def stage(buf, off, ln, mtu=0, flags=0, plead=0, cap=None, seed=0):
    """What one fs_coalesce_batch of the host batch (buf, off, ln) into payload + plead of a noise-filled
    device buffer needs, on the device: (the expected dict, the whole payload tensor, the call's arguments)."""
    import torch

    room = int(ln.sum()) if cap is None else cap
    noise = np.random.default_rng(77 + seed).integers(0, 256, plead + room + TAIL, dtype=np.uint8)
    e = ref.expected(buf, off, ln, mtu, flags, noise, plead, room)
    e["noise"] = noise
    dev = torch.device("cuda:0")
    pt = torch.from_numpy(noise).to(dev)
    args = (torch.from_numpy(buf).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
            torch.from_numpy(ln.astype(np.int32)).to(dev), mtu, flags, pt[plead : plead + room])
    return e, pt, args


def check(eng, buf, off, ln, mtu=0, flags=0, plead=0, cap=None, seed=0):
    """One staged call, waited for and compared in full. Returns the expected dict, with the device's
    own run records under "dev_runs"."""
    import torch

    from seqs_amd import split_runs

    e, pt, args = stage(buf, off, ln, mtu, flags, plead, cap, seed)
    res = eng.coalesce_device(*args)
    torch.cuda.synchronize()
    compare(e, pt.cpu().numpy(), *res[1:])
    e["dev_runs"] = split_runs(res[1], res[3])[0]
    return e


def build(specs):
    return [s["raw"] if "raw" in s else
            ref.tcp_frame(s["hdr"], s["seq"], s["payload"], s["flags"], s["ident"], s["options"],
                          ip_options=s.get("ip_options", b"")) for s in specs]


# ---- 1. IHL x data offset ------------------------------------------------------------------------

GRID_PAYLOADS = (0, 1, 37)
GRID_ROTATIONS = 76  # 0..63 as a wave has lanes, and 12 more: 396 frames are 6 waves and 12 frames


@functools.lru_cache(maxsize=None)
def grid_frames():
    """(frames, (proto, ip_opts, tcp_opts, payload) per frame): TCP with 0..10 dwords of IP options x
    0..10 dwords of TCP options, UDP with 0..10 dwords of IP options, payloads of 0, 1 and 37 bytes."""
    rnd = random.Random(4)
    what = [(6, i, t, p) for i in range(11) for t in range(11) for p in GRID_PAYLOADS]
    what += [(17, i, 0, p) for i in range(11) for p in GRID_PAYLOADS]
    return [framegen.valid_frame(rnd, proto, payload=p, ip_opts=i, tcp_opts=t) for proto, i, t, p in what], what


def rotated(seq, r):
    return list(seq[r:]) + list(seq[:r])


def test_ihl_and_data_offset_grid(eng):
    frames, what = grid_frames()
    n = len(frames)
    for r in range(GRID_ROTATIONS):
        fr, wh = rotated(frames, r), rotated(what, r)
        buf, off, ln = ref.pack(fr, lead=r % 4, seed=r)
        e = check(eng, buf, off, ln, plead=r % 16, seed=r)
        assert (e["st"] == 0).all() and run_list(e) == [(k, 1) for k in range(n)], r
        assert e["payload_bytes"] == sum(w[3] for w in wh)
        # the flags byte of a TCP frame with 40 bytes of IP options lies at 14 + 4 * 15 + 13
        for k, (proto, ihl_opts, _, _) in enumerate(wh):
            if proto == 6 and ihl_opts == 10:
                assert int(e["dev_runs"]["tcp_flags"][k]) == fr[k][14 + 4 * 15 + 13], (r, k)


# ---- 2. options inside a flow --------------------------------------------------------------------

def test_ip_options_inside_a_flow(eng):
    rng = np.random.default_rng(41)
    s = base_specs(rng)
    s[2]["ip_options"] = NOP4  # IHL 6 on segment 2 alone: it joins neither neighbour
    e = check(eng, *ref.pack(ref.finish(build(s)), lead=2), plead=3, seed=1)
    assert run_list(e) == [(0, 2), (2, 1), (3, 2)] and e["payload_bytes"] == 402
    s = base_specs(rng)
    for x in s:
        x["ip_options"] = NOP4  # the whole flow with IHL 6, Seq continuing: no frame with options joins
    e = check(eng, *ref.pack(ref.finish(build(s)), lead=1), plead=6, seed=2)
    assert run_list(e) == [(k, 1) for k in range(5)] and e["payload_bytes"] == 402
    s = base_specs(rng)
    s[1]["ip_options"] = NOP4
    s[1]["flags"] = ACK | FIN
    e = check(eng, *ref.pack(ref.finish(build(s)), lead=3), plead=9, seed=3)
    assert run_list(e) == [(0, 1), (1, 1), (2, 3)]
    assert [int(x) for x in e["dev_runs"]["tcp_flags"]] == [ACK, ACK | FIN, ACK]


# ---- 3. every verdict between runs ---------------------------------------------------------------

SPLICE_AT = (10, 100, 200)  # where the three flows start in the spliced batch; the second is split
VERDICT_SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def verdict_batch(seed):
    """framegen.edge_batch(seed) (every verdict, IP and TCP options, padding, corrupted checksums) with
    three flows of four continuing segments spliced in at SPLICE_AT; a frame of IP version 6 stands
    between the second and the third segment of the flow at SPLICE_AT[1]."""
    frames = list(framegen.edge_batch(seed))
    rng = np.random.default_rng(300 + seed)
    for k, at in enumerate(SPLICE_AT):
        flow = ref.finish(ref.segments(rng, ref.flow_header(rng, 0x6000 + k), int(rng.integers(0, 1 << 32)),
                                       [int(x) for x in rng.integers(1, 200, 4)]))
        if k == 1:
            bad = bytearray(flow[1])
            bad[14] = 0x65
            flow[2:2] = [bytes(bad)]
        frames[at:at] = flow
    return frames


def spliced_runs():
    a, b, c = SPLICE_AT
    return [(a, 4), (b, 2), (b + 3, 2), (c, 4)]


@pytest.mark.parametrize("seed", VERDICT_SEEDS)
def test_every_verdict_between_runs(eng, seed):
    frames = verdict_batch(seed)
    for mtu in (0, 1514):
        buf, off, ln = ref.pack(frames, lead=seed, seed=seed)
        e = check(eng, buf, off, ln, mtu, plead=seed + 4, seed=seed + mtu)
        assert set(spliced_runs()) <= set(run_list(e))
        assert e["st"][SPLICE_AT[1] + 2] == 5 and e["run_of"][SPLICE_AT[1] + 2] == ref.NO_RUN
        assert (mtu == 0) == (2 not in e["st"])


@pytest.mark.parametrize("variant", engines.VARIANTS, ids=engines.IDS)
def test_verdicts_under_every_digest_kernel(variant):
    e2 = engines.engine_for(variant)
    try:
        buf, off, ln = ref.pack(verdict_batch(1), lead=2, seed=variant)
        for mtu in (0, 1514):
            e = check(e2, buf, off, ln, mtu, plead=1, seed=variant)  # (out and status are compared too)
            assert set(spliced_runs()) <= set(run_list(e))
    finally:
        e2.close()


def fcs_batch():
    """verdict_batch(1) with every frame's FCS behind it, every eighth one's damaged."""
    frames = verdict_batch(1)
    damaged = list(range(0, len(frames), 8))
    return ref.with_fcs(frames, damaged), damaged


def test_verdicts_with_damaged_fcs(eng):
    frames, damaged = fcs_batch()
    buf, off, ln = ref.pack(frames, lead=3, seed=5)
    e = check(eng, buf, off, ln, flags=ref.RX_FCS, plead=2, seed=5)
    plain = ref.expected(*ref.pack(verdict_batch(1), lead=3, seed=5), 0, 0, np.zeros(int(ln.sum()), dtype=np.uint8))
    assert (e["st"][damaged] == FS_ERR_FCS).all() and (e["run_of"][damaged] == ref.NO_RUN).all()
    rest = np.setdiff1d(np.arange(len(frames)), damaged)
    assert np.array_equal(e["st"][rest], plain["st"][rest])
    # the damaged frames contribute no payload: the total is that of the accepted frames left
    kept = [ref.payload_range(f) for f, v in zip(frames, e["st"]) if v == 0]
    assert e["payload_bytes"] == sum(end - start for start, end in kept) < plain["payload_bytes"]


# ---- 4. memory order is not batch order ----------------------------------------------------------

def six_run():
    rng = np.random.default_rng(43)
    return ref.finish(ref.segments(rng, ref.flow_header(rng, 0x7000), 0xFFFFFF00, [90, 33, 100, 1, 64, 77]))


def order_cases(frames, dup):
    """(name, buf, offsets, lengths) of the batch laid out in reverse, in a seeded random order with
    gaps of 0..40 bytes, and in order with frame `dup` listed twice in a row."""
    n = len(frames)
    rng = np.random.default_rng(44)
    yield ("reverse",) + ref.pack_at(frames, range(n - 1, -1, -1), [3] + [0] * (n - 1), seed=1)
    yield ("random",) + ref.pack_at(frames, rng.permutation(n), rng.integers(0, 41, n), seed=2)
    buf, off, ln = ref.pack_at(frames, range(n), [1] + [0] * (n - 1), seed=3)
    yield "twice", buf, np.insert(off, dup + 1, off[dup]), np.insert(ln, dup + 1, ln[dup])


def test_memory_order_is_not_batch_order(eng):
    want = run_list(check(eng, *ref.pack(verdict_batch(2), lead=2)))
    for name, buf, off, ln in order_cases(verdict_batch(2), SPLICE_AT[1] + 1):
        e = check(eng, buf, off, ln, plead=5, seed=len(name))
        if name != "twice":
            assert run_list(e) == want, name
        else:  # the flow's second segment twice: the copy opens a run of its own
            assert {(SPLICE_AT[1], 2), (SPLICE_AT[1] + 2, 1)} <= set(run_list(e))
            assert e["n_runs"] == len(want) + 1
    for name, buf, off, ln in order_cases(six_run(), 2):
        e = check(eng, buf, off, ln, plead=7, seed=len(name))
        # a duplicate does not continue itself (its Seq is not the one expected), the next frame continues it
        assert run_list(e) == ([(0, 3), (3, 4)] if name == "twice" else [(0, 6)]), name
        assert e["payload_bytes"] == 365 + (100 if name == "twice" else 0)


# ---- 5. the join rule at wave and block boundaries -----------------------------------------------

BOUNDARIES = (64, 128, 256, 512)
SPLITS = ("seq", "byte0", "byte53", "ece", "psh", "syn", "damaged", "udp", "udp42", "ihl6", "doff6", "ack")


def boundary_case(b, case, seed=0):
    """A flow of b + 2 continuing segments with frame b or b - 1 altered as `case` names: the frames
    (checksums filled). Frame b is the first of a wave (and, from 256 on, of a scan block): its lane
    reads frame b - 1 itself."""
    rng = np.random.default_rng(1000 * b + seed)
    s = base_specs(rng, seq0=int(rng.integers(0, 1 << 32)), sizes=[int(x) for x in rng.integers(6, 27, b + 2)])
    corrupt = None
    if case == "seq":
        s[b]["seq"] += 1
    elif case in ("byte0", "byte53"):
        raw = bytearray(build([s[b]])[0])
        raw[0 if case == "byte0" else 53] ^= 0x40
        s[b] = dict(raw=bytes(raw))
    elif case == "ece":
        s[b]["flags"] = ACK | ECE
    elif case == "psh":
        s[b - 1]["flags"] = ACK | PSH
    elif case == "syn":
        s[b]["flags"] = ACK | SYN
    elif case == "damaged":
        corrupt = 54
    elif case == "udp":
        s[b - 1] = dict(raw=ref.udp_frame(rng, rng.integers(0, 256, 33, dtype=np.uint8).tobytes()))
    elif case == "udp42":
        s[b - 1] = dict(raw=ref.udp_frame(rng, b""))
    elif case == "ihl6":
        s[b - 1]["ip_options"] = NOP4
    elif case == "doff6":
        s[b - 1]["options"] = NOP4
    elif case == "ack":  # frame b - 1 without payload, the later ones' Seq continuing from it
        cut = len(s[b - 1]["payload"])
        s[b - 1]["payload"] = b""
        for x in s[b:]:
            x["seq"] -= cut
    else:
        assert case == "control"
    frames = ref.finish(build(s))
    if corrupt is not None:
        f = bytearray(frames[b - 1])
        f[corrupt] ^= 0x01
        frames[b - 1] = bytes(f)
    return frames


@pytest.mark.parametrize("b", BOUNDARIES)
def test_join_rule_at_wave_and_block_boundaries(eng, b):
    for k, case in enumerate(SPLITS + ("control",)):
        buf, off, ln = ref.pack(boundary_case(b, case), lead=1 + k % 7, seed=k)
        e = check(eng, buf, off, ln, plead=k % 5, seed=b + k)
        if case == "control":
            assert e["run_of"][b] == e["run_of"][b - 1] == 0 and run_list(e) == [(0, b + 2)]
        else:
            assert e["run_of"][b] != e["run_of"][b - 1], case
            assert e["run_of"][b] != ref.NO_RUN and e["run_of"][b + 1] != ref.NO_RUN, case
            # the run before the split ends with frame b - 1, or with b - 2 where b - 1 is the altered one
            assert run_list(e)[0] == (0, b if case in ("seq", "byte0", "byte53", "ece", "psh", "syn") else b - 1), case


# ---- 6. more scan blocks than one turn of the partials scan --------------------------------------

def carry_frames():
    """B * B + B + 1 continuing segments of one flow: B + 2 scan blocks of B frames, so the partials
    scan (B blocks a turn) takes a second turn for the last two."""
    B = ref.scan_block()
    return long_run(B * B + B + 1, 61)


def damaged_first_turn(frames):
    """The frames with a payload byte flipped in the first B * B of them: every block of the partials
    scan's first turn is empty."""
    B = ref.scan_block()
    out = list(frames)
    for i in range(B * B):
        f = bytearray(out[i])
        f[56] ^= 0x80
        out[i] = bytes(f)
    return out


@pytest.fixture(scope="module")
def carry():
    return carry_frames()


def test_scan_carry_one_run(eng, carry):
    n = len(carry)
    e = check(eng, *ref.pack(carry, lead=3, seed=6), plead=1, seed=6)
    assert run_list(e) == [(0, n)] and int(e["dev_runs"]["n_frames"][0]) == n == 65793


def test_scan_carry_alternating_runs(eng):
    B = ref.scan_block()
    frames, k = alternating_runs(B * B + B + 1, 62)
    e = check(eng, *ref.pack(frames, lead=2, seed=7), plead=7, seed=7)
    assert e["n_runs"] == k and [c for _, c in run_list(e)][:4] == [1, 2, 1, 2]


def test_scan_carry_nothing_accepted_in_the_first_turn(eng, carry):
    B = ref.scan_block()
    e = check(eng, *ref.pack(damaged_first_turn(carry), lead=1, seed=8), plead=5, seed=8)
    assert run_list(e) == [(B * B, B + 1)] and (e["st"][: B * B] == 13).all()
    assert (e["run_of"][: B * B] == ref.NO_RUN).all() and (e["run_of"][B * B :] == 0).all()


def test_scan_carry_under_a_capped_grid(carry):
    from seqs_amd import Engine

    e3 = Engine(0)
    try:
        e3.set_workgroups(3)
        e = check(e3, *ref.pack(carry, lead=3, seed=6), plead=1, seed=9)
        assert run_list(e) == [(0, len(carry))]
    finally:
        e3.close()


# ---- 7. copy bodies at the in-flight boundaries, and the longest payloads ------------------------

BODY_PIECES = (15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129)
BODY_LENGTHS = [16 * k + d for k in BODY_PIECES for d in (0, 1, 15)] + [8946]
# TotalLength 65,535: 14 + TotalLength wraps RecvEth's uint16 `end` (stacks/portstack.go:202), so
# these two are rejected whole; TotalLength 65,521 is the largest that passes: the longest payloads
# that are copied are 65,481 (TCP) and 65,493 (UDP) bytes
WRAPPED = (("tcp", 65495), ("udp", 65507))
LONGEST = (("tcp", 65481), ("udp", 65493))


@functools.lru_cache(maxsize=None)
def body_frames():
    rng = np.random.default_rng(45)
    kinds = [("tcp", n) for n in BODY_LENGTHS] + list(WRAPPED) + list(LONGEST)
    frames = []
    for k, (kind, n) in enumerate(kinds):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        frames.append(ref.udp_frame(rng, data) if kind == "udp" else
                      ref.tcp_frame(ref.flow_header(rng, 0x2000 + k), int(rng.integers(0, 1 << 32)), data))
    return ref.finish(frames)


@pytest.mark.parametrize("plead", range(16))
def test_copy_body_boundaries_and_longest_payloads(eng, plead):
    frames = body_frames()
    m = len(BODY_LENGTHS)
    for lead in (0, 5):
        e = check(eng, *ref.pack(frames, lead, seed=lead), plead=plead, seed=16 * plead + lead)
        assert list(e["st"]) == [0] * m + [7, 7, 0, 0]
        assert [int(x) for x in e["dev_runs"]["payload_len"]] == BODY_LENGTHS + [n for _, n in LONGEST]
        assert e["payload_bytes"] == sum(BODY_LENGTHS) + sum(n for _, n in LONGEST)


# ---- 8. payload_cap at every value ---------------------------------------------------------------

CAP_SIZES = [5, 0, 17, 1, 40, 0]


def cap_frames():
    rng = np.random.default_rng(46)
    frames = []
    for k, n in enumerate(CAP_SIZES):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        frames.append(ref.udp_frame(rng, data) if k == 2 else ref.tcp_frame(ref.flow_header(rng, 0x5100 + k), 7 * k, data))
    return ref.finish(frames)


def test_payload_cap_at_every_value(eng):
    total = sum(CAP_SIZES)
    buf, off, ln = ref.pack(cap_frames(), lead=6)
    ends = np.cumsum(CAP_SIZES)
    for cap in range(total + 2):
        e = check(eng, buf, off, ln, plead=cap % 16, cap=cap, seed=cap)
        assert e["payload_bytes"] == total and e["n_runs"] == len(CAP_SIZES)
        # a frame is copied if and only if it ends at or below the cap
        last = int(ends[ends <= cap].max()) if (ends <= cap).any() else 0
        p = cap % 16
        assert np.array_equal(e["payload"][p + last :], e["noise"][p + last :])
        # the host form into the caller's own buffer: the same bytes, the noise behind them kept
        noise = np.random.default_rng(500 + cap).integers(0, 256, cap + TAIL, dtype=np.uint8)
        h = ref.expected(buf, off, ln, 0, 0, noise, 0, cap)
        mine = noise.copy()
        _, runs, run_of, totals, dig, st = eng.coalesce_host(buf, off, ln, payload=mine[:cap])
        assert np.array_equal(mine, h["payload"]), cap
        assert runs.tobytes() == h["runs"].tobytes() and np.array_equal(run_of, h["run_of"])
        assert (int(totals["payload_bytes"]), int(totals["n_runs"])) == (total, len(CAP_SIZES))
        assert np.array_equal(dig, h["dig"]) and np.array_equal(st, h["st"])


# ---- 9. the context's scratch, reused by a smaller batch without a sync --------------------------

def test_scratch_reuse_without_a_sync():
    import torch

    from seqs_amd import Engine

    B = ref.scan_block()
    e1 = Engine(0)
    try:
        batches = [ref.pack(alternating_runs(2 * B + 1, 91)[0], lead=1, seed=1),
                   ref.pack(ref.finish(build(base_specs(np.random.default_rng(92)))), lead=2, seed=2),
                   ref.pack(long_run(B + 1, 93), lead=3, seed=3)]
        staged = [stage(*b, plead=k, seed=90 + k) for k, b in enumerate(batches)]
        torch.cuda.synchronize()
        results = [e1.coalesce_device(*args) for _, _, args in staged]  # one stream, nothing between the calls
        torch.cuda.synchronize()
        for (e, pt, _), res in zip(staged, results):
            compare(e, pt.cpu().numpy(), *res[1:])
        assert [e["n_runs"] for e, _, _ in staged][1:] == [1, 1]
    finally:
        e1.close()
