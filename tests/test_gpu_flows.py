"""The flow-aware RX coalesce on the GPU (fs_coalesce_flows_batch / fs_coalesce_flows_batch_host)
against the sequential restatement + C oracle of tests/flows_ref.py. Every comparison is the WHOLE
payload buffer byte for byte (lead and tail noise included: a store outside a payload shows), plus
runs[:n_runs], flows[:n_flows], order[:n_accepted], run_of, the totals, digests and verdicts."""
import ctypes

import numpy as np
import pytest

import coalesce_ref as cref
import flows_ref as ref
import segment_ref as sref

pytestmark = pytest.mark.gpu

FCS_APPEND = 2
TAIL = 96  # noise past the payload's last possible byte
ACK, FIN, PSH = ref.ACK, ref.FIN, ref.PSH


@pytest.fixture(scope="module")
def eng():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()  # (torch's runtime first, as in the other GPU suites)
    e = Engine(0)
    yield e
    e.close()


def to_device(buf, off, ln):
    import torch

    dev = torch.device("cuda:0")
    return (torch.from_numpy(buf).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
            torch.from_numpy(ln.astype(np.int32)).to(dev))


def compare(e, got_payload, runs, flows, order, run_of, totals, out, st):
    """Device results against ref.expected()'s dict."""
    from seqs_amd import split_digests, split_flows

    r, f, o, t = split_flows(runs, flows, order, totals)
    assert (int(t["payload_bytes"]), int(t["n_runs"]), int(t["n_flows"]), int(t["n_accepted"]), int(t["reserved"])) == \
        (e["payload_bytes"], e["n_runs"], e["n_flows"], e["n_accepted"], 0)
    assert np.array_equal(o, e["order"]), (o[:16], e["order"][:16])
    assert r.tobytes() == e["runs"].tobytes(), (r[:8], e["runs"][:8])
    assert f.tobytes() == e["flows"].tobytes(), (f[:8], e["flows"][:8])
    assert np.array_equal(run_of.cpu().numpy().view(np.uint32), e["run_of"])
    bad = np.flatnonzero(got_payload != e["payload"])
    assert bad.size == 0, f"{bad.size} payload bytes differ, first at {bad[:8]}"
    crc, ipc, l4c = split_digests(out.cpu().numpy())
    assert np.array_equal(crc, e["dig"]["crc32"]) and np.array_equal(ipc, e["dig"]["ip_csum"])
    assert np.array_equal(l4c, e["dig"]["l4_csum"])
    assert np.array_equal(st.cpu().numpy(), e["st"])


def check(eng, buf, off, ln, mtu=0, flags=0, plead=0, cap=None, seed=0, e=None):
    """One fs_coalesce_flows_batch of the host batch (buf, off, ln) into payload + plead of a
    noise-filled device buffer; everything compared. `e`: the expected dict of an earlier check of the
    same batch, buffer and cap, not computed again. Returns the expected dict."""
    import torch

    room = int(ln.sum()) if cap is None else cap
    noise = np.random.default_rng(77 + seed).integers(0, 256, plead + room + TAIL, dtype=np.uint8)
    if e is None:
        e = ref.expected(buf, off, ln, mtu, flags, noise, plead, room)
    pt = torch.from_numpy(noise).to(torch.device("cuda:0"))
    res = eng.coalesce_flows_device(*to_device(buf, off, ln), mtu, flags, payload=pt[plead : plead + room])
    torch.cuda.synchronize()
    compare(e, pt.cpu().numpy(), *res[1:])
    e["noise"] = noise
    return e


def run_list(e):
    return [(int(r["first_frame"]), int(r["n_frames"])) for r in e["runs"]]


def flow_list(e):
    return [(int(f["first_frame"]), int(f["n_frames"]), int(f["n_runs"])) for f in e["flows"]]


# ---- 1. two interleaved flows --------------------------------------------------------------------

def two_flows():
    rng = np.random.default_rng(101)
    a = ref.segments(rng, ref.flow_header(rng, 0x1111), 1000, [100, 37, 64])
    b = ref.segments(rng, ref.flow_header(rng, 0x2222), (1 << 32) - 40, [33, 200, 5])
    return ref.finish([a[0], b[0], a[1], b[1], a[2], b[2]])


def test_two_interleaved_flows(eng):
    import torch

    from seqs_amd import split_runs

    frames = two_flows()
    buf, off, ln = ref.pack(frames, lead=3)
    e = check(eng, buf, off, ln, plead=5)
    assert run_list(e) == [(0, 3), (3, 3)] and flow_list(e) == [(0, 3, 1), (3, 3, 1)]
    assert list(e["order"]) == [0, 2, 4, 1, 3, 5] and list(e["run_of"]) == [0, 1, 0, 1, 0, 1]
    want = b"".join(frames[i][54:] for i in (0, 2, 4, 1, 3, 5))
    assert e["payload"][5 : 5 + len(want)].tobytes() == want and e["payload_bytes"] == len(want) == 439
    assert [int(x) for x in e["flows"]["payload_len"]] == [201, 238]
    # the frame-before-it rule on the same batch: every frame a run of its own
    _, runs, _, totals, _, _ = eng.coalesce_device(*to_device(buf, off, ln))
    torch.cuda.synchronize()
    assert split_runs(runs, totals)[2] == 6


# ---- 2. round trip through fs_segment_batch, the sends interleaved -------------------------------

@pytest.mark.parametrize("fcs", [False, True])
def test_interleaved_sends_come_back_contiguous(eng, fcs):
    import torch

    from seqs_amd import split_flows
    from test_gpu_coalesce import round_trip_sends, segmented

    specs, payload = round_trip_sends()
    buf, off, ln = segmented(eng, specs, payload, FCS_APPEND if fcs else 0, lead=5)
    counts = [sref.n_frames(mss, n) for _, _, n, mss in specs]
    first = np.concatenate([[0], np.cumsum(counts)])
    perm = np.array([first[g] + k for g, k in ref.interleave([range(c) for c in counts])], dtype=np.int64)
    assert sorted(perm) == list(range(int(first[-1]))) and perm[1] == first[1]
    # only offsets and lengths move: the frames stay where fs_segment_batch built them
    poff, pln = off[torch.from_numpy(perm).to(off.device)], ln[torch.from_numpy(perm).to(ln.device)]
    hb, ho, hl = buf.cpu().numpy(), poff.cpu().numpy().astype(np.uint64), pln.cpu().numpy().astype(np.uint32)
    flags = ref.RX_FCS if fcs else 0
    e = check(eng, hb, ho, hl, 0, flags, plead=3)
    # ... and straight from the device tensors, against what was sent
    want = b"".join(payload[at : at + n].tobytes() for _, at, n, _ in specs)
    pay, runs, flows, order, _, totals, _, _ = eng.coalesce_flows_device(buf, poff.contiguous(), pln.contiguous(), 0, flags)
    torch.cuda.synchronize()
    r, f, o, t = split_flows(runs, flows, order, totals)
    assert int(t["payload_bytes"]) == len(want) and pay[: len(want)].cpu().numpy().tobytes() == want
    assert int(t["n_runs"]) == int(t["n_flows"]) == len(specs) == e["n_runs"]  # one flow and one run per send
    assert np.array_equal(perm[o], np.arange(perm.size))  # delivery order is the order the frames were built in
    at = 0
    for k, ((hdr, _, n, _), run, fl) in enumerate(zip(specs, r, f)):
        assert (int(run["payload_off"]), int(run["payload_len"]), int(run["first_frame"]), int(run["n_frames"])) == \
            (at, n, first[k], counts[k])
        assert (int(fl["payload_off"]), int(fl["payload_len"]), int(fl["first_run"]), int(fl["n_runs"]),
                int(fl["first_frame"]), int(fl["n_frames"])) == (at, n, k, 1, first[k], counts[k])
        assert int(run["tcp_flags"]) == (0 if hdr[23] == 17 else hdr[47])
        at += n


# ---- 3. contiguous flows: fs_coalesce_batch's result ---------------------------------------------

def test_contiguous_flows_equal_coalesce_batch(eng):
    import torch

    from seqs_amd import split_flows, split_runs
    from test_flows_host import contiguous_batch

    for seed in range(3):
        frames = contiguous_batch(seed)
        buf, off, ln = ref.pack(frames, lead=seed)
        e = check(eng, buf, off, ln, plead=seed, seed=seed)
        assert list(e["order"]) == list(range(len(frames)))
        tb, to, tl = to_device(buf, off, ln)
        room = int(ln.sum())
        noise = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, room + TAIL, dtype=np.uint8)).to(tb.device)
        p1, p2 = noise.clone(), noise.clone()
        _, runs1, run_of1, totals1, out1, st1 = eng.coalesce_device(tb, to, tl, payload=p1[:room])
        _, runs2, flows2, order2, run_of2, totals2, out2, st2 = eng.coalesce_flows_device(tb, to, tl, payload=p2[:room])
        torch.cuda.synchronize()
        r1, total1, n1 = split_runs(runs1, totals1)
        r2, _, _, t2 = split_flows(runs2, flows2, order2, totals2)
        assert torch.equal(p1, p2) and r1.tobytes() == r2.tobytes() and torch.equal(run_of1, run_of2)
        assert (total1, n1) == (int(t2["payload_bytes"]), int(t2["n_runs"]))
        assert torch.equal(out1, out2) and torch.equal(st1, st2)


# ---- 4. key edges --------------------------------------------------------------------------------

KEY_AT = [23, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37]


def test_every_key_byte_opens_a_flow(eng):
    rng = np.random.default_rng(41)
    base = bytearray(ref.flow_header(rng, 0x4141))
    frames = [ref.tcp_frame(bytes(base), 100, b"base")]
    for at in KEY_AT[1:]:
        h = bytearray(base)
        h[at] ^= 0x10
        frames.append(ref.tcp_frame(bytes(h), 100, b"other"))
    # byte 23 (the protocol): a UDP frame with the base's addresses and ports
    u = bytearray(ref.udp_frame(rng, b"udp payload"))
    u[26:38] = base[26:38]
    frames.append(bytes(u))
    # ... and once more the base flow, continuing its first frame behind all the others
    frames.append(ref.tcp_frame(bytes(base), 104, b"again"))
    buf, off, ln = ref.pack(ref.finish(frames), lead=1)
    e = check(eng, buf, off, ln, plead=2)
    assert e["n_flows"] == 14 and e["n_accepted"] == 15 and e["n_runs"] == 14
    assert list(e["order"]) == [0, 14] + list(range(1, 14)) and flow_list(e)[0] == (0, 2, 1)


def test_macs_ip_options_and_protocols(eng):
    rng = np.random.default_rng(42)
    hdr = bytearray(ref.flow_header(rng, 0x4242))
    other_mac = bytearray(hdr)
    other_mac[6:12] = bytes(x ^ 0x5A for x in hdr[6:12])
    stranger = ref.flow_header(rng, 0x4243)
    frames = [
        ref.tcp_frame(bytes(hdr), 10, b"0123456789"),
        ref.tcp_frame(stranger, 1, b"stranger"),
        # equal key, another source MAC: the same flow, but the join rule compares the MACs
        ref.tcp_frame(bytes(other_mac), 20, b"from another MAC"),
        # the same ports behind 8 bytes of IP options: the same flow (and never joined)
        ref.tcp_frame(bytes(hdr), 36, b"behind options", ip_options=b"\x01" * 8),
    ]
    # UDP with the TCP flow's addresses and ports: a flow of its own
    u = bytearray(ref.udp_frame(rng, b"udp"))
    u[26:38] = hdr[26:38]
    frames.append(bytes(u))
    # inside one flow: a pure ACK and a segment with TCP options are runs of one
    frames.append(ref.tcp_frame(bytes(hdr), 50, b""))
    frames.append(ref.tcp_frame(bytes(hdr), 50, b"with tcp options", options=b"\x01\x01\x01\x01"))
    frames.append(ref.tcp_frame(bytes(hdr), 66, b"plain again"))
    frames.append(ref.tcp_frame(bytes(hdr), 77, b"and joined"))
    buf, off, ln = ref.pack(ref.finish(frames), lead=2)
    e = check(eng, buf, off, ln, plead=1)
    assert list(e["st"]) == [0] * 9
    assert list(e["order"]) == [0, 2, 3, 5, 6, 7, 8, 1, 4]
    assert flow_list(e) == [(0, 7, 6), (7, 1, 1), (8, 1, 1)]
    assert run_list(e) == [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (5, 2), (7, 1), (8, 1)]


# ---- 5. rejected frames --------------------------------------------------------------------------

def damaged(frame, at=56):
    f = bytearray(frame)
    f[at] ^= 0x80
    return bytes(f)


def test_rejected_frames(eng):
    rng = np.random.default_rng(51)
    a = ref.finish(ref.segments(rng, ref.flow_header(rng, 0x5151), 700, [40, 50, 60, 70]))
    b = ref.finish(ref.segments(rng, ref.flow_header(rng, 0x5252), 9, [11, 12]))
    # a damaged frame of flow B between A1 and A2 does not split A
    frames = [a[0], a[1], damaged(b[0]), a[2], a[3], b[1]]
    buf, off, ln = ref.pack(frames, lead=1)
    e = check(eng, buf, off, ln, plead=3)
    assert list(e["st"]) == [0, 0, 13, 0, 0, 0] and run_list(e) == [(0, 4), (4, 1)] and list(e["order"]) == [0, 1, 3, 4, 5]
    assert e["run_of"][2] == ref.NO_RUN
    # a damaged A1 splits A at the Seq gap
    frames = [a[0], damaged(a[1]), b[0], a[2], a[3], b[1]]
    buf, off, ln = ref.pack(frames, lead=2)
    e = check(eng, buf, off, ln, plead=1)
    assert list(e["st"]) == [0, 13, 0, 0, 0, 0] and run_list(e) == [(0, 1), (1, 2), (3, 2)]
    assert flow_list(e) == [(0, 3, 2), (3, 2, 1)]


def test_no_frame_accepted(eng):
    rng = np.random.default_rng(52)
    n = cref.scan_block() + 1
    frames = [damaged(f) for f in ref.finish(ref.segments(rng, ref.flow_header(rng), 5, [9] * n))]
    buf, off, ln = ref.pack(frames, lead=1)
    e = check(eng, buf, off, ln, plead=5)
    assert (e["n_runs"], e["n_flows"], e["n_accepted"], e["payload_bytes"]) == (0, 0, 0, 0)
    assert (e["st"] == 13).all() and (e["run_of"] == ref.NO_RUN).all()
    # nothing but the totals and run_of is written: runs, flows and order keep the caller's bytes
    import torch

    dev = torch.device("cuda:0")
    lib, vp = eng.lib, ctypes.c_void_p
    tb, to, tl = to_device(buf, off, ln)
    keep = [torch.full((n * w,), 0xA5, dtype=torch.uint8, device=dev) for w in (24, 32, 4)]
    pay = torch.full((64,), 0xA5, dtype=torch.uint8, device=dev)
    totals = torch.full((24,), 0xA5, dtype=torch.uint8, device=dev)
    st = lib.fs_coalesce_flows_batch(eng._ctx, vp(tb.data_ptr()), vp(to.data_ptr()), vp(tl.data_ptr()), n, 0, 0,
                                     vp(pay.data_ptr()), 64, vp(keep[0].data_ptr()), vp(keep[1].data_ptr()),
                                     vp(keep[2].data_ptr()), None, vp(totals.data_ptr()), None, None,
                                     vp(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    torch.cuda.synchronize()
    assert all(bool((k == 0xA5).all()) for k in keep) and bool((pay == 0xA5).all()) and bool((totals == 0).all())


# ---- 6. sizes ------------------------------------------------------------------------------------

def small_batch(n, n_flows, seed, reject=0.0):
    """n TCP segments of n_flows flows in random interleave, payloads of 1..40 bytes, each flow's
    Seq continuing; a share `reject` of them damaged."""
    rng = np.random.default_rng(seed)
    hdrs = [ref.flow_header(rng, 0x6000 + f) for f in range(n_flows)]
    seq = [int(rng.integers(0, 1 << 32)) for _ in range(n_flows)]
    frames = []
    for _ in range(n):
        f = int(rng.integers(0, n_flows))
        size = int(rng.integers(1, 41))
        frames.append(ref.tcp_frame(hdrs[f], seq[f], rng.integers(0, 256, size, dtype=np.uint8).tobytes(),
                                    ident=int(rng.integers(0, 1 << 16))))
        seq[f] += size
    frames = ref.finish(frames)
    return [damaged(f, 54) if rng.random() < reject else f for f in frames]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_sizes_around_the_wave_and_the_scan_block(eng, n):
    buf, off, ln = ref.pack(small_batch(n, max(1, n // 9), n, reject=0.1 if n > 1 else 0.0), lead=n % 4, seed=n)
    e = check(eng, buf, off, ln, plead=n % 7, seed=n)
    assert e["n_flows"] == len({int(x) for x in e["flows"]["first_frame"]}) <= max(1, n // 9)
    assert e["n_accepted"] == int((e["st"] == 0).sum()) and e["n_runs"] >= e["n_flows"]


BIG = 65793  # 257 scan blocks and one frame


from deliver_cases import big_batch  # noqa: E402  (the numpy builder, shared with the delivery's edge suite)


BIG_SHAPES = {
    "every frame its own flow": lambda: np.arange(BIG, dtype=np.int64),
    "one flow": lambda: np.zeros(BIG, dtype=np.int64),
    "1000 flows": lambda: np.random.default_rng(6).integers(0, 1000, BIG).astype(np.int64),
}


@pytest.mark.parametrize("shape", list(BIG_SHAPES))
def test_65793_frames(eng, shape):
    flow_of = BIG_SHAPES[shape]()
    if shape == "1000 flows":
        flow_of[:1000] = np.random.default_rng(7).permutation(1000)  # (every flow present)
    buf, off, ln = big_batch(flow_of, 60 + len(shape))
    e = check(eng, buf, off, ln, plead=1)
    assert e["n_accepted"] == BIG and e["payload_bytes"] == 10 * BIG
    if shape == "every frame its own flow":
        assert e["n_flows"] == e["n_runs"] == BIG and np.array_equal(e["order"], np.arange(BIG, dtype=np.uint32))
    elif shape == "one flow":
        assert flow_list(e) == [(0, BIG, 1)] and run_list(e) == [(0, BIG)]
    else:
        assert e["n_flows"] == e["n_runs"] == 1000 and int(e["flows"]["n_frames"].sum()) == BIG


# ---- 7. the hash-mask hook -----------------------------------------------------------------------

def test_results_do_not_depend_on_the_hash(eng):
    from seqs_amd import Engine
    from seqs_amd.framesum import TEST_LIB_PATH

    buf, off, ln = ref.pack(small_batch(300, 100, 70, reject=0.05), lead=2)
    e = check(eng, buf, off, ln, plead=3, seed=70)
    assert 90 <= e["n_flows"] <= 100
    te = Engine(0, lib_path=TEST_LIB_PATH)
    try:
        for mask in (0, 0xF, 0xFFFFFFFF):  # every key probes from slot 0; 16 starting slots; the product's
            assert te.lib.fs_test_set_flow_hash_mask(te._ctx, mask) == 0
            check(te, buf, off, ln, plead=3, seed=70, e=e)
    finally:
        te.close()


# ---- 8. payload_cap ------------------------------------------------------------------------------

def test_every_payload_cap(eng):
    rng = np.random.default_rng(80)
    a = ref.segments(rng, ref.flow_header(rng, 0x8080), 1, [7, 16, 5])
    b = ref.segments(rng, ref.flow_header(rng, 0x8181), 2, [9, 1, 20])
    buf, off, ln = ref.pack(ref.finish([a[0], b[0], b[1], a[1], a[2], b[2]]), lead=3)
    full = check(eng, buf, off, ln, plead=2)
    assert full["payload_bytes"] == 58 and list(full["order"]) == [0, 3, 4, 1, 2, 5]
    for cap in range(0, 59):
        e = check(eng, buf, off, ln, plead=2, cap=cap, seed=cap)
        assert e["payload_bytes"] == 58 and e["runs"].tobytes() == full["runs"].tobytes()
        assert e["flows"].tobytes() == full["flows"].tobytes()
        # delivery order: A0 A1 A2 B0 B1 B2 end at 7, 23, 28, 37, 38, 58
        written = max([end for end in (0, 7, 23, 28, 37, 38, 58) if end <= cap])
        assert np.array_equal(e["payload"][2 + written :], e["noise"][2 + written :])


# ---- 9. the context's scratch --------------------------------------------------------------------

@pytest.mark.parametrize("workgroups", [0, 1])
def test_back_to_back_calls_share_the_scratch(eng, workgroups):
    import torch

    from seqs_amd import Engine

    e2 = Engine(0)
    try:
        e2.set_workgroups(workgroups)
        batches = [ref.pack(small_batch(n, f, 90 + n, reject=0.1), lead=1, seed=n) for n, f in ((700, 40), (37, 5), (300, 300))]
        exp, got = [], []
        for k, (buf, off, ln) in enumerate(batches):
            room = int(ln.sum())
            noise = np.random.default_rng(90 + k).integers(0, 256, room + TAIL, dtype=np.uint8)
            exp.append(ref.expected(buf, off, ln, 0, 0, noise, 0, room))
            pt = torch.from_numpy(noise).to(torch.device("cuda:0"))
            got.append((pt, to_device(buf, off, ln), room))
        torch.cuda.synchronize()
        res = [e2.coalesce_flows_device(*dev, payload=pt[:room]) for pt, dev, room in got]  # no sync in between
        torch.cuda.synchronize()
        for e, (pt, _, _), r in zip(exp, got, res):
            compare(e, pt.cpu().numpy(), *r[1:])
    finally:
        e2.close()


# ---- 10. the host entry point and coalesce_flows_batch -------------------------------------------

def test_host_form_and_lists(eng):
    frames = two_flows()
    buf, off, ln = ref.pack(frames, lead=9)
    for cap in (None, 300):
        room = int(ln.sum()) if cap is None else cap
        noise = np.random.default_rng(61).integers(0, 256, room + TAIL, dtype=np.uint8)
        e = ref.expected(buf, off, ln, 0, 0, noise, 0, room)
        mine = noise.copy()
        pay, runs, flows, order, run_of, totals, dig, st = eng.coalesce_flows_host(buf, off, ln, payload=mine[:room])
        assert np.array_equal(mine, e["payload"]) and runs.tobytes() == e["runs"].tobytes()
        assert flows.tobytes() == e["flows"].tobytes() and np.array_equal(order, e["order"])
        assert np.array_equal(run_of, e["run_of"]) and np.array_equal(dig, e["dig"]) and np.array_equal(st, e["st"])
        assert (int(totals["payload_bytes"]), int(totals["n_runs"]), int(totals["n_flows"]), int(totals["n_accepted"]),
                int(totals["reserved"])) == (e["payload_bytes"], 2, 2, 6, 0)
    got = eng.coalesce_flows_batch(frames)
    want = []
    for members in ((0, 2, 4), (1, 3, 5)):
        f = frames[members[0]]
        want.append((6, f[26:30], f[30:34], int.from_bytes(f[34:36], "big"), 80,
                     [(ACK, b"".join(frames[i][54:] for i in members))]))
    assert got == want
    assert eng.coalesce_flows_batch([]) == []


# ---- the call's own checks -----------------------------------------------------------------------

def test_rejected_calls_and_empty_batch(eng):
    import torch

    from seqs_amd import FramesumError, split_flows

    buf, off, ln = ref.pack(two_flows(), lead=4)
    tb, to, tl = to_device(buf, off, ln)
    with pytest.raises(FramesumError):
        eng.coalesce_flows_device(tb, to, tl, flags=2)  # unknown flag bit
    with pytest.raises(FramesumError):
        eng.coalesce_flows_device(tb[1:], to, tl)  # frames not 4-byte aligned
    lib, vp = eng.lib, ctypes.c_void_p
    some = vp(tb.data_ptr())
    # a null order; n above 2^30
    assert lib.fs_coalesce_flows_batch(eng._ctx, some, some, some, 6, 0, 0, some, 8, some, some, None, None, some, None,
                                       None, None) == -1
    assert lib.fs_coalesce_flows_batch(eng._ctx, some, some, some, (1 << 30) + 1, 0, 0, some, 8, some, some, some, None,
                                       some, None, None, None) == -1
    _, runs, flows, order, run_of, totals, _, _ = eng.coalesce_flows_device(tb, to[:0], tl[:0])
    torch.cuda.synchronize()
    t = split_flows(runs, flows, order, totals)[3]
    assert bytes(t.tobytes()) == bytes(24) and run_of.numel() == 0
