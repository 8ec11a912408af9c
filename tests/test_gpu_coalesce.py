"""The RX coalesce on the GPU (fs_coalesce_batch / fs_coalesce_batch_host) against the sequential
restatement + C oracle of tests/coalesce_ref.py. Every comparison is the WHOLE payload buffer byte for
byte (lead and tail noise included: a store outside a payload shows), plus runs[:n_runs], run_of, the
totals, digests and verdicts."""
import numpy as np
import pytest

import coalesce_ref as ref
import segment_ref as sref

pytestmark = pytest.mark.gpu

FCS_APPEND = 2
TAIL = 96  # noise past the payload's last possible byte
ACK, FIN, SYN, PSH = ref.ACK, ref.FIN, ref.SYN, ref.PSH


@pytest.fixture(scope="module")
def eng():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()  # (torch's runtime first, as in the other GPU suites)
    e = Engine(0)
    yield e
    e.close()


def compare(e, got_payload, runs, run_of, totals, out, st):
    """Device results against ref.expected()'s dict."""
    from seqs_amd import TOTALS_DTYPE, split_digests, split_runs

    t = np.ascontiguousarray(totals.cpu().numpy()).view(TOTALS_DTYPE)[0]
    assert (int(t["payload_bytes"]), int(t["n_runs"]), int(t["reserved"])) == (e["payload_bytes"], e["n_runs"], 0)
    r, _, _ = split_runs(runs, totals)
    assert r.tobytes() == e["runs"].tobytes(), (r, e["runs"])
    assert np.array_equal(run_of.cpu().numpy().view(np.uint32), e["run_of"])
    bad = np.flatnonzero(got_payload != e["payload"])
    assert bad.size == 0, f"{bad.size} payload bytes differ, first at {bad[:8]}"
    crc, ipc, l4c = split_digests(out.cpu().numpy())
    assert np.array_equal(crc, e["dig"]["crc32"]) and np.array_equal(ipc, e["dig"]["ip_csum"])
    assert np.array_equal(l4c, e["dig"]["l4_csum"])
    assert np.array_equal(st.cpu().numpy(), e["st"])


def check(eng, buf, off, ln, mtu=0, flags=0, plead=0, cap=None, seed=0):
    """One fs_coalesce_batch of the host batch (buf, off, ln) into payload + plead of a noise-filled
    device buffer; everything compared. Returns the expected dict."""
    import torch

    room = int(ln.sum()) if cap is None else cap
    noise = np.random.default_rng(77 + seed).integers(0, 256, plead + room + TAIL, dtype=np.uint8)
    e = ref.expected(buf, off, ln, mtu, flags, noise, plead, room)
    dev = torch.device("cuda:0")
    pt = torch.from_numpy(noise).to(dev)
    res = eng.coalesce_device(torch.from_numpy(buf).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
                              torch.from_numpy(ln.astype(np.int32)).to(dev), mtu, flags, payload=pt[plead : plead + room])
    torch.cuda.synchronize()
    compare(e, pt.cpu().numpy(), *res[1:])
    e["noise"] = noise
    return e


def run_list(e):
    return [(int(r["first_frame"]), int(r["n_frames"])) for r in e["runs"]]


# ---- 1. round trip through fs_segment_batch ------------------------------------------------------

def round_trip_sends():
    from test_gpu_segment import edge_specs

    specs, payload = edge_specs()
    flows = []
    for i, (hdr, at, ln, mss) in enumerate(specs):  # one flow per send
        h = bytearray(hdr)
        h[34:36] = (0x1000 + i).to_bytes(2, "big")
        flows.append((bytes(h), at, ln, mss))
    return flows, payload


def segmented(eng, specs, payload, flags, lead):
    """The sends built on the device behind `lead` bytes of noise: (frames tensor, offsets, lengths as
    the coalesce takes them)."""
    import torch

    from seqs_amd import segment_layout

    sends = sref.make_sends(specs)
    _, nbytes = segment_layout(sends, flags, 1)
    dev = torch.device("cuda:0")
    buf = torch.from_numpy(np.random.default_rng(3).integers(0, 256, lead + nbytes + 64, dtype=np.uint8)).to(dev)
    _, off, ln, _, st = eng.segment_device(sends, torch.from_numpy(payload).to(dev), 0, flags, 1, frames=buf[lead:])
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    return buf, off + lead, ln + (4 if flags else 0)


@pytest.mark.parametrize("fcs", [False, True])
def test_round_trip_gives_the_sends_back(eng, fcs):
    import torch

    from seqs_amd import split_runs

    specs, payload = round_trip_sends()
    buf, off, ln = segmented(eng, specs, payload, FCS_APPEND if fcs else 0, lead=5)
    hb, ho, hl = buf.cpu().numpy(), off.cpu().numpy().astype(np.uint64), ln.cpu().numpy().astype(np.uint32)
    e = check(eng, hb, ho, hl, 0, ref.RX_FCS if fcs else 0, plead=3)
    # ... and straight from the device tensors, against what was sent
    want = b"".join(payload[at : at + n].tobytes() for _, at, n, _ in specs)
    pay, runs, _, totals, _, _ = eng.coalesce_device(buf, off, ln, 0, ref.RX_FCS if fcs else 0)
    torch.cuda.synchronize()
    r, total, n_runs = split_runs(runs, totals)
    assert total == len(want) and pay[:total].cpu().numpy().tobytes() == want
    assert n_runs == len(specs) == e["n_runs"]  # one run per send: TCP with payload, UDP, empty
    at, first = 0, 0
    for (hdr, _, n, mss), run in zip(specs, r):
        frames = sref.n_frames(mss, n)
        assert (int(run["payload_off"]), int(run["payload_len"]), int(run["first_frame"]), int(run["n_frames"])) == \
            (at, n, first, frames)
        assert int(run["tcp_flags"]) == (0 if hdr[23] == 17 else hdr[47])
        at, first = at + n, first + frames


# ---- 2. copy edges -------------------------------------------------------------------------------

COPY_LENGTHS = [0, 1, 2, 3, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1446]


@pytest.fixture(scope="module")
def copy_frames():
    rng = np.random.default_rng(21)
    frames = [ref.tcp_frame(ref.flow_header(rng, 0x2000 + k), int(rng.integers(0, 1 << 32)),
                            rng.integers(0, 256, n, dtype=np.uint8).tobytes()) for k, n in enumerate(COPY_LENGTHS)]
    return ref.finish(frames)


@pytest.mark.parametrize("plead", range(16))
def test_copy_edges_at_every_alignment(eng, copy_frames, plead):
    # frames lie back to back behind `lead` bytes, so lead = 0..15 puts every payload at every source
    # alignment; its destination alignment is plead + the lengths before it
    for lead in range(16):
        buf, off, ln = ref.pack(copy_frames, lead, seed=lead)
        e = check(eng, buf, off, ln, plead=plead, seed=16 * plead + lead)
        assert run_list(e) == [(k, 1) for k in range(len(COPY_LENGTHS))]
        assert e["payload_bytes"] == sum(COPY_LENGTHS)


# ---- 3. the join rule ----------------------------------------------------------------------------

SIZES = [100, 37, 1, 64, 200]


def base_specs(rng, seq0=1000, sizes=SIZES):
    hdr, specs, seq = ref.flow_header(rng), [], seq0
    for k, n in enumerate(sizes):
        specs.append(dict(hdr=hdr, seq=seq, payload=rng.integers(0, 256, n, dtype=np.uint8).tobytes(), flags=ACK,
                          ident=0x4000 + 7 * k, options=b""))
        seq += n
    return specs


def build(specs):
    return [s["raw"] if "raw" in s else ref.tcp_frame(s["hdr"], s["seq"], s["payload"], s["flags"], s["ident"], s["options"])
            for s in specs]


def join_case(eng, specs, mtu=0, corrupt=None, seed=0):
    frames = ref.finish(build(specs))
    if corrupt is not None:
        i, at = corrupt
        f = bytearray(frames[i])
        f[at] ^= 0x01
        frames[i] = bytes(f)
    buf, off, ln = ref.pack(frames, lead=1 + seed % 7, seed=seed)
    return check(eng, buf, off, ln, mtu, plead=seed % 5, seed=seed), frames


def test_join_base_and_seq(eng):
    rng = np.random.default_rng(31)
    e, frames = join_case(eng, base_specs(rng))
    assert run_list(e) == [(0, 5)] and e["payload_bytes"] == sum(SIZES) and int(e["runs"]["tcp_flags"][0]) == ACK
    # the fields segmentation varies differ between these frames, and they still join
    a, b = frames[1], frames[2]
    assert a[16:18] != b[16:18] and a[18:20] != b[18:20] and a[24:26] != b[24:26] and a[50:52] != b[50:52]
    for gap in (1, -1):  # frame 2 alone is off by one: neither it nor frame 3 continues its neighbour
        s = base_specs(rng)
        s[2]["seq"] += gap
        assert run_list(join_case(eng, s, seed=gap + 2)[0]) == [(0, 2), (2, 1), (3, 2)]
    for gap in (1, -1):  # a gap that the later frames carry on: the run splits in two
        s = base_specs(rng)
        for k in (2, 3, 4):
            s[k]["seq"] += gap
        assert run_list(join_case(eng, s, seed=gap + 5)[0]) == [(0, 2), (2, 3)]
    e, _ = join_case(eng, base_specs(rng, seq0=(1 << 32) - 120))  # Seq wraps inside frame 1
    assert run_list(e) == [(0, 5)]
    e, _ = join_case(eng, base_specs(rng, seq0=(1 << 32) - 100))  # ... and exactly at a frame boundary
    assert run_list(e) == [(0, 5)]


def test_join_splits_on_every_compared_header_byte(eng):
    rng = np.random.default_rng(32)
    for i in ref.COMPARED:
        s = base_specs(rng)
        raw = bytearray(build(s)[2])
        raw[i] ^= 0x40  # (byte 47: ECE, a compared bit; the checksums are filled after the flip)
        s[2] = dict(raw=bytes(raw))
        e, _ = join_case(eng, s, seed=i)
        assert e["run_of"][2] != e["run_of"][1] and e["n_runs"] >= 2, i
        assert e["run_of"][0] == e["run_of"][1] == 0, i


def test_join_flags_options_and_strangers(eng):
    rng = np.random.default_rng(33)
    # a corrupted payload byte in frame 2: ErrChecksumTCPorUDP, two runs, none of its bytes
    e, _ = join_case(eng, base_specs(rng), corrupt=(2, 54), seed=1)
    assert e["st"][2] == 13 and run_list(e) == [(0, 2), (3, 2)] and e["payload_bytes"] == sum(SIZES) - SIZES[2]
    assert e["run_of"][2] == ref.NO_RUN
    s = base_specs(rng)
    s[2]["flags"] = ACK | PSH  # PSH ends the run there
    e, _ = join_case(eng, s, seed=2)
    assert run_list(e) == [(0, 3), (3, 2)] and list(e["runs"]["tcp_flags"]) == [ACK | PSH, ACK]
    s = base_specs(rng)
    s[4]["flags"] = ACK | FIN  # FIN on the last frame only: it shows in the run's flags
    e, _ = join_case(eng, s, seed=3)
    assert run_list(e) == [(0, 5)] and list(e["runs"]["tcp_flags"]) == [ACK | FIN]
    s = base_specs(rng)
    s[2]["flags"] = ACK | SYN
    assert run_list(join_case(eng, s, seed=4)[0]) == [(0, 2), (2, 1), (3, 2)]
    s = base_specs(rng)
    s[2]["options"] = b"\x01\x01\x01\x01"  # data offset 6
    e, _ = join_case(eng, s, seed=5)
    assert run_list(e) == [(0, 2), (2, 1), (3, 2)] and e["payload_bytes"] == sum(SIZES)
    s = base_specs(rng, sizes=[100, 37, 0, 64, 200])  # a pure ACK in the middle
    e, _ = join_case(eng, s, seed=6)
    assert run_list(e) == [(0, 2), (2, 1), (3, 2)] and int(e["runs"]["payload_len"][1]) == 0
    s = base_specs(rng)
    s.insert(2, dict(raw=ref.udp_frame(rng, rng.integers(0, 256, 33, dtype=np.uint8).tobytes())))
    e, _ = join_case(eng, s, seed=7)
    assert run_list(e) == [(0, 2), (2, 1), (3, 3)] and list(e["runs"]["tcp_flags"]) == [ACK, 0, ACK]
    s = base_specs(rng, sizes=[100, 37, 1400, 64, 200])  # frame 2 above the MTU
    e, _ = join_case(eng, s, mtu=1000, seed=8)
    assert e["st"][2] == 2 and run_list(e) == [(0, 2), (3, 2)]


# ---- 4. scan boundaries --------------------------------------------------------------------------

def scan_sizes():
    B = ref.scan_block()
    return [1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1]


def long_run(n, seed):
    """n segments of one flow, frames of 60..80 bytes (payloads of 6..26)."""
    rng = np.random.default_rng(seed)
    return ref.finish(ref.segments(rng, ref.flow_header(rng), int(rng.integers(0, 1 << 32)),
                                   [int(x) for x in rng.integers(6, 27, n)]))


def alternating_runs(n, seed):
    """Runs of 1 and 2 frames in turn, each of a flow of its own; every other single is padded to 60 bytes."""
    rng = np.random.default_rng(seed)
    frames, k = [], 0
    while len(frames) < n:
        want = min(1 + k % 2, n - len(frames))
        sizes = [int(x) for x in rng.integers(6, 27, want)]
        if k % 4 == 0:
            sizes, pad = [int(rng.integers(1, 6))], 60
        else:
            pad = 0
        frames += ref.segments(rng, ref.flow_header(rng, 0x3000 + k), int(rng.integers(0, 1 << 32)), sizes, pad_to=pad)
        k += 1
    return ref.finish(frames), k


@pytest.mark.parametrize("n", scan_sizes())
def test_scan_boundaries(eng, n):
    buf, off, ln = ref.pack(long_run(n, n), lead=3, seed=n)
    e = check(eng, buf, off, ln, plead=1, seed=n)
    assert run_list(e) == [(0, n)]
    frames, k = alternating_runs(n, n + 1)
    buf, off, ln = ref.pack(frames, lead=2, seed=n)
    e = check(eng, buf, off, ln, plead=7, seed=n)
    assert e["n_runs"] == k and [c for _, c in run_list(e)][: 4] == [1, 2, 1, 2][: k]


def test_no_frame_accepted(eng):
    n = ref.scan_block() + 1
    frames = [bytearray(f) for f in long_run(n, 5)]
    for f in frames:
        f[56] ^= 0x80  # every payload corrupted
    buf, off, ln = ref.pack([bytes(f) for f in frames], lead=1)
    e = check(eng, buf, off, ln, plead=5)
    assert e["n_runs"] == 0 and e["payload_bytes"] == 0 and (e["st"] == 13).all() and (e["run_of"] == ref.NO_RUN).all()


# ---- 5. payload_cap ------------------------------------------------------------------------------

def test_payload_cap_in_the_middle_of_a_frame(eng):
    rng = np.random.default_rng(51)
    frames = ref.segments(rng, ref.flow_header(rng, 0x5000), 77, [300, 500, 700])
    frames.append(ref.udp_frame(rng, rng.integers(0, 256, 90, dtype=np.uint8).tobytes()))
    frames += ref.segments(rng, ref.flow_header(rng, 0x5001), 99, [0])
    frames += ref.segments(rng, ref.flow_header(rng, 0x5002), 5, [40, 50])
    buf, off, ln = ref.pack(ref.finish(frames), lead=6)
    full = check(eng, buf, off, ln, plead=2)
    cap = 300 + 500 + 333  # inside frame 2's payload
    e = check(eng, buf, off, ln, plead=2, cap=cap)
    assert e["payload_bytes"] == full["payload_bytes"] == 1680 > cap
    assert e["runs"].tobytes() == full["runs"].tobytes() and run_list(e) == [(0, 3), (3, 1), (4, 1), (5, 2)]
    # (compare() has checked the whole buffer: frames 0 and 1 copied, the noise from byte 800 on intact)
    assert np.array_equal(e["payload"][2 + 800 :], e["noise"][2 + 800 :])
    e = check(eng, buf, off, ln, plead=2, cap=0)  # nothing fits: payload may then be empty
    assert e["payload_bytes"] == 1680


# ---- 6. the host entry point and coalesce_batch --------------------------------------------------

def test_host_form_and_lists(eng):
    specs, payload = round_trip_sends()
    buf, off, ln = segmented(eng, specs, payload, 0, lead=0)
    hb, ho, hl = buf.cpu().numpy(), off.cpu().numpy(), ln.cpu().numpy()
    frames = [hb[int(o) : int(o) + int(n)].tobytes() for o, n in zip(ho, hl)] + ref.kat_frames()
    buf, off, ln = ref.pack(frames, lead=9)
    for cap in (None, 4000):
        room = int(ln.sum()) if cap is None else cap
        noise = np.random.default_rng(61).integers(0, 256, room + TAIL, dtype=np.uint8)
        e = ref.expected(buf, off, ln, 0, 0, noise, 0, room)
        mine = noise.copy()
        pay, runs, run_of, totals, dig, st = eng.coalesce_host(buf, off, ln, payload=mine[:room])
        assert np.array_equal(mine, e["payload"]) and runs.tobytes() == e["runs"].tobytes()
        assert np.array_equal(run_of, e["run_of"]) and np.array_equal(dig, e["dig"]) and np.array_equal(st, e["st"])
        assert (int(totals["payload_bytes"]), int(totals["n_runs"])) == (e["payload_bytes"], e["n_runs"])
    assert e["n_runs"] > len(specs)  # (the KAT frames add runs of their own)
    got = eng.coalesce_batch(frames)
    full = ref.expected(buf, off, ln, 0, 0, np.zeros(int(ln.sum()), dtype=np.uint8))
    want = [(int(r["first_frame"]), int(r["n_frames"]), int(r["tcp_flags"]),
             full["payload"][int(r["payload_off"]) : int(r["payload_off"]) + int(r["payload_len"])].tobytes())
            for r in full["runs"]]
    assert got == want
    assert eng.coalesce_batch([]) == []


# ---- 7. a capped grid ----------------------------------------------------------------------------

def test_grid_cap(eng):
    from seqs_amd import Engine

    n = scan_sizes()[-1]
    e3 = Engine(0)
    try:
        e3.set_workgroups(3)  # three workgroups loop over the scan blocks and the copy tiles
        buf, off, ln = ref.pack(long_run(n, 71), lead=3)
        assert run_list(check(e3, buf, off, ln, plead=1)) == [(0, n)]
        frames, k = alternating_runs(n, 72)
        buf, off, ln = ref.pack(frames, lead=2)
        assert check(e3, buf, off, ln, plead=7)["n_runs"] == k
    finally:
        e3.close()


# ---- the call's own checks -----------------------------------------------------------------------

def test_rejected_calls_and_empty_batch(eng):
    import torch

    from seqs_amd import FramesumError, split_runs

    buf, off, ln = ref.pack(long_run(4, 81), lead=4)
    dev = torch.device("cuda:0")
    tb, to, tl = (torch.from_numpy(buf).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
                  torch.from_numpy(ln.astype(np.int32)).to(dev))
    with pytest.raises(FramesumError):
        eng.coalesce_device(tb, to, tl, flags=2)  # unknown flag bit
    with pytest.raises(FramesumError):
        eng.coalesce_device(tb[1:], to, tl)  # frames not 4-byte aligned
    _, runs, run_of, totals, _, _ = eng.coalesce_device(tb, to[:0], tl[:0])
    torch.cuda.synchronize()
    assert split_runs(runs, totals)[1:] == (0, 0) and run_of.numel() == 0
