"""The host-staged calls that stage through one context's shared buffers (fs_fill_batch_host,
fs_segment_batch_host, fs_coalesce_batch_host, fs_coalesce_flows_batch_host), taken together: the
buffers grow, are reused at a stale larger capacity and pass from one call to the next; the calls
recover after a host-staged digest that failed half-way; and each rejects a frame that ends past
frames_bytes. Then the eight RX entry points (the plain and the flow-aware coalesce, the delivery and
the receive call, device and host forms) through their raw prototypes, with each nullable array left
out in turn. Expected results come from the restatements the calls' own suites use
(tests/coalesce_ref.py, tests/flows_ref.py, tests/deliver_ref.py, tests/recv_ref.py,
tests/segment_ref.py, the C oracle's fill_batch), and every comparison is the WHOLE buffer byte for
byte, noise tails included."""
import numpy as np
import pytest

import coalesce_ref as cref
import flows_ref as fref
import segment_ref as sref

pytestmark = pytest.mark.gpu

FILL_CSUM, FCS_APPEND = 1, 2
TAIL = 96  # noise past the last byte a call may write


@pytest.fixture(scope="module")
def eng():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()  # (torch's runtime first, as in the other GPU suites)
    e = Engine(0)
    yield e
    e.close()


# ---- the batches ---------------------------------------------------------------------------------

def rx_frames(n, seed):
    """n finished frames, n a multiple of 4: the segments of four TCP flows taken in turn (the
    flow-aware coalesce joins what the frame-before-it rule cannot), one UDP frame among them and one
    frame with a corrupted payload."""
    rng = np.random.default_rng(seed)
    groups = [cref.segments(rng, cref.flow_header(rng, 0x6000 + k), int(rng.integers(0, 1 << 32)),
                            [int(x) for x in rng.integers(8, 200, n // 4)]) for k in range(4)]
    frames = [groups[g][i] for g, i in fref.interleave(groups)]
    frames[5] = cref.udp_frame(rng, rng.integers(0, 256, 77, dtype=np.uint8).tobytes())
    frames = cref.finish(frames)
    bad = bytearray(frames[9])
    bad[60] ^= 0x10
    frames[9] = bytes(bad)
    assert len(frames) == n
    return frames


def tx_specs(n, seed):
    """Sends that make n frames, n a multiple of 4: TCP sends of four segments each, every fourth send
    replaced by four UDP sends."""
    rng = np.random.default_rng(seed)
    specs, at = [], 1
    for k in range(n // 4):
        if k % 4 == 3:
            for _ in range(4):
                ln = int(rng.integers(0, 300))
                specs.append((sref.udp_header(rng), at, ln, 0))
                at += ln
        else:
            mss = int(rng.integers(7, 700))
            specs.append((sref.tcp_header(rng, seq=int(rng.integers(0, 1 << 32))), at, 3 * mss + 7, mss))
            at += 3 * mss + 7 + int(rng.integers(0, 3))
    return specs, rng.integers(0, 256, at + 5, dtype=np.uint8)


# ---- one call of each kind, everything compared --------------------------------------------------

def do_fill(eng, n, seed, flags):
    from oracle import coracle

    frames = rx_frames(n, seed)
    gaps = np.random.default_rng(seed).integers(4, 12, n)  # room for every FCS, at every alignment
    buf, off, ln = cref.pack_at(frames, range(n), gaps, seed=seed)
    exp = buf.copy()
    edig, est = coracle.fill_batch(exp, off, ln, 0, flags)
    got = buf.copy()
    dig, st = eng.fill_host(got, off, ln, 0, flags)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"fill n={n}: {bad.size} bytes differ, first at {bad[:8]}"
    assert np.array_equal(dig, edig) and np.array_equal(st, est)


def do_segment(eng, n, seed, flags, align):
    from seqs_amd import segment_layout

    specs, payload = tx_specs(n, seed)
    sends = sref.make_sends(specs)
    count, nbytes = segment_layout(sends, flags, align)
    assert count == n
    noise = np.random.default_rng(seed).integers(0, 256, nbytes + TAIL, dtype=np.uint8)
    ebuf, eoff, eln, edig, est = sref.expected(specs, payload, 0, flags, align, noise)
    frames = noise.copy()
    _, off, ln, dig, st = eng.segment_host(sends, payload, 0, flags, align, frames=frames)
    bad = np.flatnonzero(frames != ebuf)
    assert bad.size == 0, f"segment n={n}: {bad.size} bytes differ, first at {bad[:8]}"
    assert np.array_equal(off, eoff) and np.array_equal(ln, eln)
    assert np.array_equal(dig, edig) and np.array_equal(st, est)


def rx_case(n, seed, capped):
    """(buf, off, ln, room, noise): the batch, and the payload buffer's capacity (below the batch's
    payload total when `capped`) with its noise."""
    buf, off, ln = cref.pack(rx_frames(n, seed), lead=1 + seed % 7, seed=seed)
    room = int(ln.sum()) // 3 if capped else int(ln.sum())
    return buf, off, ln, room, np.random.default_rng(seed).integers(0, 256, room + TAIL, dtype=np.uint8)


def do_coalesce(eng, n, seed, capped):
    buf, off, ln, room, noise = rx_case(n, seed, capped)
    e = cref.expected(buf, off, ln, 0, 0, noise, 0, room)
    assert (e["payload_bytes"] > room) == capped and 1 < e["n_runs"] < n
    mine = noise.copy()
    _, runs, run_of, totals, dig, st = eng.coalesce_host(buf, off, ln, payload=mine[:room])
    bad = np.flatnonzero(mine != e["payload"])
    assert bad.size == 0, f"coalesce n={n}: {bad.size} payload bytes differ, first at {bad[:8]}"
    assert runs.tobytes() == e["runs"].tobytes() and np.array_equal(run_of, e["run_of"])
    assert np.array_equal(dig, e["dig"]) and np.array_equal(st, e["st"])
    assert (int(totals["payload_bytes"]), int(totals["n_runs"]), int(totals["reserved"])) == \
        (e["payload_bytes"], e["n_runs"], 0)


def do_flows(eng, n, seed, capped):
    buf, off, ln, room, noise = rx_case(n, seed, capped)
    e = fref.expected(buf, off, ln, 0, 0, noise, 0, room)
    assert (e["payload_bytes"] > room) == capped and e["n_flows"] == 5 and e["n_accepted"] == n - 1
    mine = noise.copy()
    _, runs, flows, order, run_of, totals, dig, st = eng.coalesce_flows_host(buf, off, ln, payload=mine[:room])
    bad = np.flatnonzero(mine != e["payload"])
    assert bad.size == 0, f"flows n={n}: {bad.size} payload bytes differ, first at {bad[:8]}"
    assert runs.tobytes() == e["runs"].tobytes() and flows.tobytes() == e["flows"].tobytes()
    assert np.array_equal(order, e["order"]) and np.array_equal(run_of, e["run_of"])
    assert np.array_equal(dig, e["dig"]) and np.array_equal(st, e["st"])
    assert (int(totals["payload_bytes"]), int(totals["n_runs"]), int(totals["n_flows"]), int(totals["n_accepted"]),
            int(totals["reserved"])) == (e["payload_bytes"], e["n_runs"], e["n_flows"], e["n_accepted"], 0)


# ---- 1. regrow and reuse on one context ----------------------------------------------------------

def test_regrow_and_reuse_on_one_context(eng):
    """16 frames, then 300, then 16 again through all four calls of ONE context: the staging buffers
    grow, then serve a smaller batch at their stale larger capacity. The calls take turns in another
    order each round, so that staging slot 0 (fill, coalesce, flows) and the device payload buffer
    (coalesce, flows) pass from each of their users to each other one. The 300-frame round gives the
    coalesce calls a payload_cap a third of the batch's payload."""
    orders = ("fill segment coalesce flows", "flows coalesce segment fill", "coalesce fill flows segment")
    for rnd, (n, order) in enumerate(zip((16, 300, 16), orders)):
        for k, call in enumerate(order.split()):
            seed = 100 * rnd + 10 * k + 1
            if call == "fill":
                do_fill(eng, n, seed, FILL_CSUM | FCS_APPEND if rnd < 2 else FILL_CSUM)
            elif call == "segment":
                do_segment(eng, n, seed, FCS_APPEND if rnd != 1 else 0, (1, 64, 4)[rnd])
            elif call == "coalesce":
                do_coalesce(eng, n, seed, capped=rnd == 1)
            else:
                do_flows(eng, n, seed, capped=rnd == 1)


# ---- 2. recovery after an injected failure -------------------------------------------------------

def two_chunk_batch():
    """128 frames of 64..1500 B in two groups of 64, the second group more than 16 MiB behind the
    first in a zero-filled buffer of 17 MiB: fs_digest_batch_host cuts it into the chunks [0, 64)
    and [64, 128) (tests/csrc/test_plan.cpp checks that on the same descriptors)."""
    ln = np.array([64 + (i * 379) % 1437 for i in range(128)], dtype=np.uint32)
    off = np.zeros(128, dtype=np.uint64)
    pos = 0
    for i in range(128):
        if i == 64:
            pos = (16 << 20) + 65536
        off[i] = pos
        pos += (int(ln[i]) + 3) & ~3
    assert int(ln.min()) >= 64 and int(ln.max()) <= 1500 and pos <= 17 << 20
    return np.zeros(17 << 20, dtype=np.uint8), off, ln


def test_calls_recover_after_a_failed_digest():
    """A host-staged digest that fails at its second chunk (the test library's fs_test_set_fault, with
    chunk 0's kernel and chunk 1's copy queued) leaves nothing behind that disturbs the segment, the
    coalesce or the flows call that follows on the same context: each is exact."""
    import torch

    from seqs_amd import Engine, FramesumError
    from seqs_amd.framesum import TEST_LIB_PATH

    assert torch.cuda.is_available(), "these tests need a GPU"
    big, boff, bln = two_chunk_batch()
    for call in (lambda e: do_segment(e, 16, 41, FCS_APPEND, 4), lambda e: do_coalesce(e, 16, 42, False),
                 lambda e: do_flows(e, 16, 43, False)):
        e = Engine(0, lib_path=TEST_LIB_PATH)
        try:
            assert e.lib.fs_test_set_fault(e._ctx, 1) == 0
            with pytest.raises(FramesumError, match="injected"):
                e.digest_host(big, boff, bln)
            assert e.lib.fs_test_last_host_path(e._ctx) == 3  # (the chunked path)
            assert e.lib.fs_test_set_fault(e._ctx, -1) == 0
            call(e)
        finally:
            e.close()
    # ... and all three in a row behind one failure
    e = Engine(0, lib_path=TEST_LIB_PATH)
    try:
        assert e.lib.fs_test_set_fault(e._ctx, 1) == 0
        with pytest.raises(FramesumError, match="injected"):
            e.digest_host(big, boff, bln)
        assert e.lib.fs_test_set_fault(e._ctx, -1) == 0
        do_segment(e, 16, 44, 0, 1)
        do_coalesce(e, 16, 45, False)
        do_flows(e, 16, 46, False)
    finally:
        e.close()


# ---- 3. out-of-range frames ----------------------------------------------------------------------

def test_frames_past_frames_bytes_are_rejected(eng):
    from seqs_amd import FramesumError

    buf, off, ln = cref.pack(rx_frames(16, 51), lead=2, tail=0)
    assert int(off[15]) + int(ln[15]) == buf.size  # the last frame ends exactly at the buffer's end
    before = buf.copy()
    for name, call in (("fs_coalesce_batch_host", eng.coalesce_host), ("fs_coalesce_flows_batch_host", eng.coalesce_flows_host)):
        call(buf, off, ln)  # in range: accepted
        with pytest.raises(FramesumError, match=f"{name}: frame 15 ends past frames_bytes"):
            call(buf[:-1], off, ln)
        far = off.copy()
        far[7] = buf.size - 10
        with pytest.raises(FramesumError, match=f"{name}: frame 7 ends past frames_bytes"):
            call(buf, far, ln)
    work = buf.copy()
    eng.fill_host(work, off, ln, 0, FILL_CSUM)
    with pytest.raises(FramesumError, match="fs_fill_batch_host: frame 15 ends past frames_bytes"):
        eng.fill_host(work[:-1], off, ln, 0, FILL_CSUM)
    # the last frame itself fits: its 4 FCS bytes alone overrun the buffer, by 4 bytes and by 1
    for room in (0, 3):
        work = np.concatenate([buf, np.zeros(room, dtype=np.uint8)])
        with pytest.raises(FramesumError, match="fs_fill_batch_host: frame 15 ends past frames_bytes"):
            eng.fill_host(work, off, ln, 0, FILL_CSUM | FCS_APPEND)
        assert np.array_equal(work[: buf.size], before)  # a rejected call writes nothing
    # ... and the context still works
    do_fill(eng, 16, 52, FILL_CSUM | FCS_APPEND)


# ---- 4. the eight RX entry points with each nullable array left out -------------------------------

RX_BASES = ("fs_coalesce_batch", "fs_coalesce_flows_batch", "fs_deliver_flows_batch", "fs_recv_flows_batch")
# (argument, the first of RX_BASES that has it): what the headers let a caller pass as NULL
RX_NULLABLE = (("run_of", 0), ("out", 0), ("status", 0), ("payload", 0), ("flows", 1), ("delivered", 2), ("code", 3))
PLEAD = 3  # the payload starts at an odd address


def rx_pin_case():
    """19 frames: three interleaved TCP flows of six segments, a UDP frame among them and one segment
    with a damaged checksum; three sockets, two with a flow of the batch and one without. n and
    n_socks are odd, so that an array lying where another should is misaligned or cut short. The
    expected results of the four call kinds come from their suites' restatements."""
    import deliver_ref as dref
    import recv_ref as rref
    from test_gpu_deliver import sock_for

    rng = np.random.default_rng(71)
    hdrs = [fref.flow_header(rng, 0x1000 + f) for f in range(3)]
    segs = [fref.segments(rng, h, 1000 * (f + 1), [100, 37, 64, 1, 90, 55]) for f, h in enumerate(hdrs)]
    frames = [segs[g][k] for g, k in fref.interleave([range(6)] * 3)]
    frames.insert(4, fref.udp_frame(rng, b"a udp datagram"))
    frames = fref.finish(frames)
    bad = bytearray(frames[9])  # flow 2's third segment
    bad[60] ^= 0x10
    frames[9] = bytes(bad)
    socks = dref.socks_of(sock_for(hdrs[2], 3000, 7, 600), sock_for(fref.flow_header(rng, 0x7777), 5, 620, 64, ring_wpos=9, ring_free=30),
                          sock_for(hdrs[0], 1000, 700, 500, ring_wpos=450))
    snd = rref.snd_of(*[((int(s["snd_nxt"]) - 100) % (1 << 32), 1000) for s in socks])
    buf, off, ln = fref.pack(frames, lead=3)
    room = int(ln.sum())
    noise = np.random.default_rng(72).integers(0, 256, PLEAD + room + TAIL, dtype=np.uint8)
    rings = np.random.default_rng(73).integers(0, 256, 1300, dtype=np.uint8)
    assert ln.size == 19 and socks.size == 3
    e = [cref.expected(buf, off, ln, 0, 0, noise, PLEAD, room), fref.expected(buf, off, ln, 0, 0, noise, PLEAD, room),
         dref.expected(buf, off, ln, 0, 0, noise, PLEAD, room, socks, rings),
         rref.expected(buf, off, ln, 0, 0, noise, PLEAD, room, socks, snd, rings)]
    assert e[3]["n_flows"] == 4 and e[3]["n_accepted"] == 18 and e[3]["st"][9] != 0
    assert [int(x) for x in e[3]["socks_out"]["n_delivered"]] == [2, 0, 6] and (e[3]["delivered"] == 2).sum() == 3
    assert int(e[3]["socks_out"]["ring_wpos"][2]) < 450 and e[3]["code"].any()  # the third socket's ring wraps
    return dict(buf=buf, off=off, ln=ln, n=19, socks=socks, snd=snd, room=room, noise=noise, rings=rings, expected=e)


def rx_pin_call(eng, kind, host, case, omit=()):
    """One call of RX_BASES[kind] (`host`: its host form) through the raw prototype, every result array
    filled with a pattern first. `omit`: the nullable arguments that go as NULL (`payload` with a cap
    of 0). Returns the bytes of every array that was passed, of `rings` and of the totals."""
    import torch

    n, n_socks = case["n"], int(case["socks"].size)
    sizes = dict(runs=24 * n, run_of=4 * n, totals=16 if kind == 0 else 24, out=8 * n, status=n)
    if kind >= 1:
        sizes.update(flows=32 * n, order=4 * n)
    if kind >= 2:
        sizes.update(socks_out=32 * n_socks, delivered=n)
    if kind == 3:
        sizes.update(snd_out=32 * n_socks, code=n)
    results = {k: np.full(v, 0xA5, dtype=np.uint8) for k, v in sizes.items()}
    results["payload"] = case["noise"].copy()
    if kind >= 2:
        results["rings"] = case["rings"].copy()
    held = dict(results, frames=case["buf"], offsets=case["off"].view(np.uint8), lengths=case["ln"].view(np.uint8))
    if host:
        at = lambda k: held[k].ctypes.data  # noqa: E731
    else:
        held = {k: torch.from_numpy(v).to("cuda:0") for k, v in held.items()}
        at = lambda k: held[k].data_ptr()  # noqa: E731
    nullable = lambda k: None if k in omit else at(k)  # noqa: E731
    args = [eng._ctx, at("frames")] + ([case["buf"].size] if host else []) + [at("offsets"), at("lengths"), n, 0, 0]
    if kind >= 2:
        args += [case["socks"].ctypes.data, n_socks, at("rings"), case["rings"].size, at("socks_out"), nullable("delivered")]
    if kind == 3:
        args += [case["snd"].ctypes.data, at("snd_out"), nullable("code")]
    args += [None, 0] if "payload" in omit else [at("payload") + PLEAD, case["room"]]
    args += [at("runs")] + ([nullable("flows"), at("order")] if kind >= 1 else [])
    args += [nullable("run_of"), at("totals"), nullable("out"), nullable("status")]
    if not host:
        args.append(torch.cuda.current_stream().cuda_stream)
    name = RX_BASES[kind] + ("_host" if host else "")
    st = getattr(eng.lib, name)(*args)
    assert st == 0, f"{name} without {omit}: {st}: {eng.lib.fs_last_error(eng._ctx).decode()}"
    if not host:
        torch.cuda.synchronize()
    return {k: held[k] if host else held[k].cpu().numpy() for k in results if k not in omit}


def rx_pin_compare(kind, got, e, n):
    """The full call's arrays against the restatement's dict: the written entries equal, the rest the
    pattern."""
    from seqs_amd.framesum import FLOW_TOTALS_DTYPE, TOTALS_DTYPE

    t = got["totals"].view(TOTALS_DTYPE if kind == 0 else FLOW_TOTALS_DTYPE)[0]
    fields = ("payload_bytes", "n_runs") + (("n_flows", "n_accepted") if kind >= 1 else ())
    assert [int(t[f]) for f in fields] == [e[f] for f in fields] and int(t["reserved"]) == 0
    written = dict(payload=e["payload"], runs=e["runs"], run_of=e["run_of"], out=e["dig"], status=e["st"])
    if kind >= 1:
        written.update(flows=e["flows"], order=e["order"])
    if kind >= 2:
        written.update(rings=e["rings"], socks_out=e["socks_out"], delivered=e["delivered"])
    if kind == 3:
        written.update(snd_out=e["snd_out"], code=e["code"])
    assert set(written) | {"totals"} == set(got)
    for k, want in written.items():
        want = np.frombuffer(want.tobytes(), dtype=np.uint8)
        assert np.array_equal(got[k][: want.size], want), (kind, k)
        assert (got[k][want.size :] == 0xA5).all(), (kind, k)
    assert e["runs"].size < n  # (some entries stay unwritten)


def test_rx_calls_with_each_nullable_array_null(eng):
    """Each of the eight RX entry points, once with every array passed (equal to the restatements of
    tests/coalesce_ref.py, flows_ref.py, deliver_ref.py and recv_ref.py), once per nullable argument
    with that argument NULL, and once with all of them NULL: every array that was passed, the rings
    and the totals equal the full call's byte for byte, the unwritten entries included."""
    case = rx_pin_case()
    for kind in range(4):
        nullable = [a for a, first in RX_NULLABLE if kind >= first]
        for host in (False, True):
            full = rx_pin_call(eng, kind, host, case)
            rx_pin_compare(kind, full, case["expected"][kind], case["n"])
            for omit in [(a,) for a in nullable] + [tuple(nullable)]:
                got = rx_pin_call(eng, kind, host, case, omit)
                assert set(got) == set(full) - set(omit)
                for k, v in got.items():
                    assert np.array_equal(v, full[k]), (RX_BASES[kind], host, omit, k)
