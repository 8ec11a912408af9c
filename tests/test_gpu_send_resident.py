"""The resident ring send on the GPU (fs_send_rings_resident) against two yardsticks: the sequential model
(tests/send_resident_ref.py, whose frames are tests/send_ref.py's) and fs_send_rings_batch of the same
library on the host copy of the built list. Every call writes into sentinel-prefilled outputs, and every
comparison is the WHOLE frames buffer, all four arrays with their untouched tails, socks_out and totals."""
import numpy as np
import pytest

import send_cases as cases
import send_ref as ref
import send_resident_cases as rcases
import send_resident_ref as rref

pytestmark = pytest.mark.gpu

FCS = ref.FCS_APPEND
TAIL = 256   # noise past the last byte the call may write
SPARE = 5    # array entries past frames_cap that the call must leave alone


@pytest.fixture(scope="module")
def eng():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()
    e = Engine(0)
    yield e
    e.close()


def sentinels(cap, seed):
    from seqs_amd.framesum import DIGEST_DTYPE

    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1 << 62, cap + SPARE).astype(np.uint64), rng.integers(0, 1 << 31, cap + SPARE).astype(np.uint32),
            rng.integers(0, 256, (cap + SPARE) * 8, dtype=np.uint8).view(DIGEST_DTYPE), rng.integers(0, 256, cap + SPARE, dtype=np.uint8))


def call(eng, recs, rings, cap, room, mtu=0, flags=0, align=1, seed=9, rings_bytes=None, so=None, sn=None, idx=None,
         writeback=False, table=None, rt=None, stream=None, skip=(), e=None):
    """One fs_send_rings_resident of `recs` (a TX_SOCK_DTYPE array; or `table`, its tensor) with frames_cap
    `cap` and frames_bytes `room` over sentinel-prefilled outputs. Returns everything on the host."""
    import torch

    from seqs_amd import split_tx, tx_socks_tensor
    from seqs_amd.framesum import DIGEST_DTYPE, _records

    e = e or eng
    dev = torch.device("cuda:0")
    noise = np.random.default_rng(seed).integers(0, 256, room + TAIL, dtype=np.uint8)
    sent = sentinels(cap, seed + 1)
    buf = torch.from_numpy(noise).to(dev)
    arrays = [torch.from_numpy(a.view(np.uint8).copy()).to(dev).view(t) for a, t in
              zip(sent, (torch.int64, torch.int32, torch.int32, torch.uint8))]
    arrays[2] = arrays[2].view(-1, 2)
    kw = {k: False for k in skip}
    for name, t in zip(("offsets", "lengths", "out", "status"), arrays):
        kw.setdefault(name, t)
    n = len(recs) if table is None else int(table.shape[0])
    outs = torch.full((n, 32), 0xEE, dtype=torch.uint8, device=dev)
    tot = torch.full((40,), 0xEE, dtype=torch.uint8, device=dev)
    table = tx_socks_tensor(recs, dev) if table is None else table
    rt = torch.from_numpy(rings).to(dev) if rt is None else rt
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)  # noqa: E731
    e.send_rings_resident(table, rt if rings_bytes is None else rt[:rings_bytes], cap, frames=buf, frames_bytes=room,
                          rx_socks_out=up(so), rx_snd_out=up(sn), rx_index=None if idx is None else up(idx).view(torch.int32),
                          writeback=writeback, mtu=mtu, flags=flags, align=align, stream=stream, socks_out=outs, totals=tot, **kw)
    torch.cuda.synchronize()
    o, t, after = split_tx(outs, tot, table)
    host = [_records(a, d) for a, d in zip(arrays, (np.uint64, np.uint32, DIGEST_DTYPE, np.uint8))]
    assert np.array_equal(rt.cpu().numpy(), rings), "the rings were written"
    return dict(frames=buf.cpu().numpy(), arrays=host, outs=o, totals=t, table=after, noise=noise, sentinels=sent, rt=rt,
                table_tensor=table)


def same_as_model(got, socks, rings, cap, room, mtu=0, flags=0, align=1, rings_bytes=None, so=None, sn=None, idx=None,
                  writeback=False, skip=()):
    e = rref.expected(socks, rings, mtu, flags, align, got["noise"], cap, room, rings_bytes, got["sentinels"], rx_socks_out=so,
                      rx_snd_out=sn, rx_index=idx)
    bad = np.flatnonzero(got["frames"] != e[0])
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8]}"
    for name, a, want, whole in zip(("offsets", "lengths", "out", "status"), got["arrays"], e[1:5], got["sentinels"]):
        assert np.array_equal(a, whole if name in skip else want), name
    assert np.array_equal(got["outs"], e[5]), f"socks_out differs at {np.flatnonzero(got['outs'] != e[5])[:8]}"
    assert got["totals"] == e[6], (got["totals"], e[6])
    p = e[7]
    want_table = ref.socks_of(p["after"] if writeback else socks)
    assert np.array_equal(got["table"], want_table), np.flatnonzero(got["table"] != want_table)[:8]
    return p


def same_as_host_call(eng, got, built_recs, built_at, mtu=0, flags=0, align=1, skip=()):
    """fs_send_rings_batch on the host copy of the built list, into the same noise: the same frames buffer,
    the same leading entries of the four arrays, the same records."""
    import torch

    buf = torch.from_numpy(got["noise"]).to("cuda:0")
    _, off, ln, out, st, outs = eng.send_rings_device(built_recs, got["rt"], mtu, flags & FCS, align, frames=buf)
    torch.cuda.synchronize()
    bad = np.flatnonzero(got["frames"] != buf.cpu().numpy())
    assert bad.size == 0, f"{bad.size} bytes differ from the host-socket call's, first at {bad[:8]}"
    k = int(off.numel())
    assert k == int(got["totals"]["n_frames"])
    for name, a, t, whole in zip(("offsets", "lengths", "out", "status"), got["arrays"], (off, ln, out, st), got["sentinels"]):
        mine = a.view(np.uint8).reshape(len(a), -1)
        if name not in skip:
            assert np.array_equal(mine[:k].reshape(-1), np.ascontiguousarray(t.cpu().numpy()).view(np.uint8).reshape(-1)), name
        assert np.array_equal(a[0 if name in skip else k :], whole[0 if name in skip else k :]), name
    assert np.array_equal(got["outs"][built_at], outs)


def check(eng, socks, rings, cap=None, room=None, mtu=0, flags=0, align=1, seed=9, e=None, **kw):
    """The call against both yardsticks. cap / room None: ample (what the whole batch needs, and a little more)."""
    model_kw = {k: v for k, v in kw.items() if k in ("rings_bytes", "so", "sn", "idx", "writeback", "skip")}
    need = rref.plan(socks, kw.get("rings_bytes", rings.size), 1 << 31, 1 << 62, flags, align, rx_socks_out=kw.get("so"),
                     rx_snd_out=kw.get("sn"), rx_index=kw.get("idx"))["totals"]
    cap = need["n_frames"] + 3 if cap is None else cap
    room = need["frames_bytes"] + 7 if room is None else room
    got = call(eng, ref.socks_of(socks), rings, cap, room, mtu, flags, align, seed, e=e, **kw)
    p = same_as_model(got, socks, rings, cap, room, mtu, flags, align, **model_kw)
    same_as_host_call(e or eng, got, ref.socks_of(p["built"]), p["built_at"], mtu, flags, align, kw.get("skip", ()))
    return got, p


COMBOS = [(0, 1, 0), (FCS, 1, 600), (0, 4, 600), (FCS, 4, 0), (0, 64, 0), (FCS, 64, 600)]


# 1 ---- parity with the host-socket call on its own suite's batches ----------------------------------------
def test_parity_wrap_sweep(eng):
    for rpos in cases.wrap_sweep_positions():
        flags, align, mtu = COMBOS[rpos % len(COMBOS)]
        check(eng, *cases.wrap_sweep(rpos), flags=flags, align=align, mtu=mtu, seed=rpos)


@pytest.mark.parametrize("flags,align,mtu", COMBOS)
@pytest.mark.parametrize("batch", ["chunk_lengths", "tiny_rings", "ring_at_the_end", "window_and_flags", "mixed", "long_socket",
                                   "rejected_frames"])
def test_parity(eng, batch, flags, align, mtu):
    socks, rings = getattr(cases, batch)()
    got, p = check(eng, socks, rings, flags=flags, align=align, mtu=1514 if batch == "rejected_frames" and mtu else mtu)
    assert int(got["totals"]["n_deferred"]) == int(got["totals"]["n_invalid"]) == 0
    if batch == "rejected_frames" and mtu:
        assert list(got["arrays"][3][:10]) == [0, 0, 0, 2, 2, 0, 10, 10, 10, 2]


# 2 ---- the scans' and the compaction's boundaries ------------------------------------------------------------
@pytest.mark.parametrize("n", rcases.BOUNDARY_SIZES)
def test_scan_boundaries(eng, n):
    for idle in ("positions", "alternate", "all"):
        got, p = check(eng, *rcases.boundary(n, idle), flags=FCS, align=4, seed=n)
        assert int(got["totals"]["n_idle"]) == p["kinds"].count(rref.IDLE) > 0
        assert int(got["totals"]["n_built"]) == (0 if idle == "all" else n // 2 if idle == "alternate" else len(p["built"]))


def test_id_stride_boundaries(eng):
    got, p = check(eng, *rcases.id_strides(), flags=FCS)
    assert [int(x) for x in got["outs"]["n_frames"]] == [x for S in rcases.STRIDE_FRAMES for x in (S, 1)]


def test_65536_bare_acks(eng):
    from seqs_amd import send_rings_layout

    recs, rings = rcases.many_acks()
    n = len(recs)
    _, nbytes, outs = send_rings_layout(recs, 0, 64)
    assert nbytes == 64 * n
    got = call(eng, recs, rings, n, nbytes, align=64)
    same_as_host_call(eng, got, recs, np.arange(n), align=64)
    assert np.array_equal(got["outs"], outs) and np.array_equal(got["outs"]["first_frame"], np.arange(n))
    t = got["totals"]
    assert [int(t[k]) for k in t.dtype.names] == [n, nbytes, 0, n, 0, 0, 0] and np.array_equal(got["table"], recs)
    # one frame and one slot short: the last socket is deferred, and nothing of it is written
    for cap, room in ((n - 1, nbytes), (n, nbytes - 1)):
        short = call(eng, recs, rings, cap, room, align=64)
        same_as_host_call(eng, short, recs[:-1], np.arange(n - 1), align=64)
        assert np.array_equal(short["frames"][64 * (n - 1) :], short["noise"][64 * (n - 1) :])
        assert int(short["outs"]["sent"][-1]) == rref.DEFERRED and np.array_equal(short["outs"][:-1], outs[:-1])
        assert [int(short["totals"][k]) for k in t.dtype.names] == [n - 1, nbytes - 64, 0, n - 1, 0, 1, 0]
        assert all(np.array_equal(a[n - 1 :], s[n - 1 :]) for a, s in zip(short["arrays"], short["sentinels"]))


# 3 ---- capacity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,align", [(0, 1), (FCS, 64)])
def test_capacity(eng, flags, align):
    socks, rings = rcases.capacity()
    ends = rcases.frame_ends(socks, flags, align)
    F, B = ends[-1]
    inside = next(ends[i][0] - 1 for i in range(1, 12) if ends[i][0] - ends[i - 1][0] >= 2)  # a cut inside a socket
    for cap in (F, F - 1, inside, ends[4][0], 0):
        got, p = check(eng, socks, rings, cap=cap, flags=flags, align=align, seed=cap)
        assert p["kinds"][8] == p["kinds"][11] == rref.IDLE and (cap == F) == (rref.DEFER not in p["kinds"])
    for room in (B, B - 1, ends[6][1] - 1, ends[4][1], 0):
        got, p = check(eng, socks, rings, room=room, flags=flags, align=align, seed=room % 1000)
        assert p["kinds"][8] == p["kinds"][11] == rref.IDLE and (room == B) == (rref.DEFER not in p["kinds"])
        assert int(got["totals"]["frames_bytes"]) <= room


def test_a_second_call_sends_the_deferred(eng):
    socks, rings = rcases.capacity()
    ends = rcases.frame_ends(socks, FCS, 1)
    whole, _ = check(eng, socks, rings, flags=FCS)
    first, p = check(eng, socks, rings, cap=ends[5][0], flags=FCS)
    rest = [s for s, k in zip(socks, p["kinds"]) if k == rref.DEFER]
    assert len(rest) == 4 and p["kinds"].count(rref.BUILT) == 5
    second, p2 = check(eng, rest, rings, flags=FCS)

    def frames_of(res):
        off, ln = res["arrays"][0], res["arrays"][1]
        return [res["frames"][int(off[f]) : int(off[f]) + int(ln[f]) + 4].tobytes() for f in range(int(res["totals"]["n_frames"]))]

    assert frames_of(first) + frames_of(second) == frames_of(whole) and len(frames_of(second)) > 4
    assert int(first["totals"]["data_bytes"]) + int(second["totals"]["data_bytes"]) == int(whole["totals"]["data_bytes"])


# 4 ---- invalid sockets -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reason", sorted(rcases.invalid_sockets()))
def test_invalid_sockets(eng, reason):
    for at in (0, 4, rcases.INVALID_N - 1):
        socks, rings, rings_bytes = rcases.with_invalid(reason, at)
        got, p = check(eng, socks, rings, rings_bytes=rings_bytes, flags=FCS, seed=reason)
        assert int(got["outs"]["sent"][at]) == rref.INVALID | reason << 16 and int(got["totals"]["n_invalid"]) == 1
        # the neighbours' frames: the host-socket call on the batch without that socket
        without = [s for i, s in enumerate(socks) if i != at]
        alone = call(eng, ref.socks_of(without), rings, 100, len(got["frames"]) - TAIL, flags=FCS, seed=reason,
                     rings_bytes=rings_bytes)
        assert np.array_equal(alone["frames"], got["frames"]) and alone["totals"]["n_frames"] == got["totals"]["n_frames"]
        same_as_host_call(eng, alone, ref.socks_of([s for s in without if ref.rule(s)["S"]]),
                          [i for i, s in enumerate(without) if ref.rule(s)["S"]], flags=FCS)


# 5 ---- the hand-off ----------------------------------------------------------------------------------------------------
def test_hand_off_records(eng):
    socks, rings, so, sn = rcases.rx_records(70)
    got, p = check(eng, socks, rings, so=so, sn=sn, flags=FCS)
    assert p["kinds"].count(rref.BUILT) > 30 and rref.IDLE in p["kinds"]
    got, p = check(eng, socks, rings, so=so, sn=sn, writeback=True, align=4)
    assert int(got["table"]["rcv_wnd"][0]) == 70000 and int(got["table"]["rcv_nxt"][0]) == 0xFFFFFFFF
    check(eng, socks, rings, so=so)               # the receive side alone: no window opens
    check(eng, socks, rings, so=so, writeback=True)


@pytest.mark.parametrize("kind", ["identity", "permuted", "holes", "range"])
def test_hand_off_index(eng, kind):
    socks, rings, so, sn = rcases.rx_records(70)
    for n_rx in (70, 100, 40):
        so_k, sn_k = (np.resize(so, n_rx), np.resize(sn, n_rx))
        idx = rcases.indices(70, n_rx, kind)
        got, p = check(eng, socks, rings, so=so_k, sn=sn_k, idx=idx, writeback=kind != "permuted", seed=n_rx)
        assert (int(got["totals"]["n_invalid"]) == 2) == (kind == "range")


def test_recv_call_outputs_straight_in(eng):
    """fs_recv_flows_batch's socks_out and snd_out tensors go into the send on the same stream, with no copy
    to the host between the two calls; the host-socket chain is computed afterwards."""
    import torch

    import deliver_ref as dref
    import flows_ref as fref
    from seqs_amd import split_snd, split_socks, tx_sock_from, tx_socks_tensor
    from seqs_amd.framesum import SND_DTYPE

    rng = np.random.default_rng(51)
    dev = torch.device("cuda:0")
    # the peers send data (the host-socket call builds their frames) ...
    peers = [ref.sock(cases.hdr(rng), 500 + 36 * i, 6000 * i, 5000, 4000 + i, 1500 + 400 * i, snd_una=0xFFFFFC00 + i,
                      snd_nxt=0xFFFFFC00 + i, rcv_nxt=1000 * (i + 1), rcv_wnd=3000) for i in range(5)]
    peer_rings = ref.filled_rings(rng, peers)
    frames, off, ln, *_ = eng.send_rings_device(ref.socks_of(peers), torch.from_numpy(peer_rings).to(dev), 0, 0, 4)
    # ... to our sockets, whose TX side has 700 unacknowledged bytes and more buffered
    rx = dref.socks_of(*(dref.sock(fref.flow_key(s["hdr"]), s["snd_nxt"], 100 + 9000 * i, 8000, snd_nxt=s["rcv_nxt"] + 700,
                                   ring_wpos=7900) for i, s in enumerate(peers)))
    snd = np.zeros(5, dtype=SND_DTYPE)
    snd["snd_una"], snd["snd_wnd"] = [s["rcv_nxt"] for s in peers], 700
    mine = [ref.sock(cases.hdr(rng), 300, 2048 * i, 2048, 2000, 900, snd_una=s["rcv_nxt"], snd_nxt=s["rcv_nxt"] + 700,
                     snd_wnd=700) for i, s in enumerate(peers)]
    mine[3]["ring_buffered"] = 0   # only the ACK that the delivery owes
    my_rings = ref.filled_rings(rng, mine)
    recs = ref.socks_of(mine)
    table, rt = tx_socks_tensor(recs, dev), torch.from_numpy(my_rings).to(dev)
    rx_rings = torch.zeros(100 + 5 * 9000, dtype=torch.uint8, device=dev)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        snd_out, _, socks_out, *_ = eng.recv_flows_device(frames, off, ln, rx, snd, rx_rings, payload=False, stream=stream)
        res = eng.send_rings_resident(table, rt, 64, frames=buf, rx_socks_out=socks_out, rx_snd_out=snd_out, stream=stream,
                                      writeback=True)
    torch.cuda.synchronize()  # the one synchronisation: both calls' results are read from here on
    so, sn = split_socks(socks_out), split_snd(snd_out)
    assert (sn["flags"] & 1).all() and list(so["bytes"]) == [1500 + 400 * i for i in range(5)]
    chain = tx_sock_from(so, recs, snd_out=sn)
    want = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    _, woff, wln, wout, wst, wouts = eng.send_rings_device(chain, rt, frames=want)
    torch.cuda.synchronize()
    k = int(woff.numel())
    assert torch.equal(buf, want) and k == 4 * 3 + 1
    for a, b in zip(res[1:5], (woff, wln, wout, wst)):
        assert torch.equal(a[:k], b)
    from seqs_amd import split_tx

    outs, tot, after = split_tx(res[5], res[6], table)
    assert np.array_equal(outs, wouts) and int(tot["n_frames"]) == k and int(tot["n_built"]) == 5
    assert int(outs["sent"][3]) == ref.TX_ACK and (after["snd_wnd"] == sn["snd_wnd"]).all() and (after["flags"] == 0).all()
    assert np.array_equal(after["rcv_nxt"], so["rcv_nxt"]) and np.array_equal(after["snd_nxt"], wouts["snd_nxt"])


# 6 ---- the write-back ----------------------------------------------------------------------------------------------------
def test_three_writeback_turns(eng):
    import torch

    from seqs_amd import tx_socks_tensor

    socks, rings, edits, caps = rcases.writeback_turns()
    dev = torch.device("cuda:0")
    table = tx_socks_tensor(ref.socks_of(socks), dev)
    model, kinds6, fins, ids = socks, [], 0, []
    for turn in range(3):
        for i, f in edits[turn].items():  # the application's edits, to the model and to the device table
            model[i] = dict(model[i], **f)
            table[i] = torch.from_numpy(ref.socks_of([model[i]]).view(np.uint8).copy()).to(dev)
        cap = caps[turn] if caps[turn] is not None else rcases.frame_ends(model)[6][0] - 1
        got = call(eng, None, rings, cap, 1 << 15, flags=FCS, seed=turn, writeback=True, table=table)
        p = same_as_model(got, model, rings, cap, 1 << 15, flags=FCS, writeback=True)
        same_as_host_call(eng, got, ref.socks_of(p["built"]), p["built_at"], flags=FCS)
        kinds6.append(p["kinds"][6])
        fins += int((got["outs"]["sent"] == ref.TX_FIN).sum())
        ids.append(int(got["outs"]["ip_id"][4]))
        model = p["after"]
    assert kinds6 == [rref.IDLE, rref.DEFER, rref.BUILT] and fins == 1 and len(set(ids)) == 3
    assert not any(s["flags"] for s in model)


# 7 ---- launch shapes and rejections ----------------------------------------------------------------------------------------
def test_one_workgroup(eng):
    from seqs_amd import Engine

    e = Engine(0)
    try:
        e.set_workgroups(1)  # one workgroup loops over the chunks and over the tiles
        check(eng, *rcases.boundary(1025), flags=FCS, e=e)
        socks, rings = cases.mixed()
        check(eng, socks, rings, cap=rcases.frame_ends(socks)[200][0], e=e)
    finally:
        e.close()


def test_eight_calls_in_flight(eng):
    import torch

    from seqs_amd import Engine, split_tx, tx_socks_tensor

    dev = torch.device("cuda:0")
    engines = [Engine(0) for _ in range(8)]
    try:
        jobs = []
        for k, e in enumerate(engines):
            socks, rings = rcases.boundary(257 + k, "positions", seed=60 + k)
            ends = rcases.frame_ends(socks)
            noise = np.random.default_rng(k).integers(0, 256, ends[-1][1] + TAIL, dtype=np.uint8)
            jobs.append((socks, rings, ends[-1][0] - k, noise, torch.from_numpy(noise).to(dev),
                         tx_socks_tensor(ref.socks_of(socks), dev), torch.from_numpy(rings).to(dev), torch.cuda.Stream(dev)))
        torch.cuda.synchronize()
        res = [e.send_rings_resident(table, rt, cap, frames=buf, stream=stream)
               for e, (socks, rings, cap, noise, buf, table, rt, stream) in zip(engines, jobs)]
        torch.cuda.synchronize()
        for r, (socks, rings, cap, noise, buf, *_) in zip(res, jobs):
            want = rref.expected(socks, rings, 0, 0, 1, noise, cap)
            outs, tot = split_tx(r[5], r[6])
            assert np.array_equal(buf.cpu().numpy(), want[0]) and np.array_equal(outs, want[5]) and tot == want[6]
            assert np.array_equal(r[1].cpu().numpy()[: want[1].size].astype(np.uint64), want[1])
    finally:
        for e in engines:
            e.close()


def test_no_sockets_and_left_out_arrays(eng):
    import torch

    from seqs_amd import split_tx

    dev = torch.device("cuda:0")
    empty = torch.zeros((0, 104), dtype=torch.uint8, device=dev)
    buf = torch.full((64,), 7, dtype=torch.uint8, device=dev)
    res = eng.send_rings_resident(empty, torch.zeros(1, dtype=torch.uint8, device=dev), 4, frames=buf,
                                  totals=torch.full((40,), 0xEE, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    outs, tot = split_tx(res[5], res[6])
    assert len(outs) == 0 and not any(int(tot[k]) for k in tot.dtype.names) and int(buf.min()) == 7
    socks, rings = rcases.capacity()
    for skip in (("offsets",), ("lengths",), ("out",), ("status",), ("offsets", "lengths", "out", "status")):
        check(eng, socks, rings, flags=FCS, skip=skip)


def test_rejected_calls(eng):
    import torch

    socks, rings = rcases.capacity()
    dev = torch.device("cuda:0")
    recs = ref.socks_of(socks)
    table = torch.from_numpy(recs.view(np.uint8).reshape(-1, 104).copy()).to(dev)
    rt, buf = torch.from_numpy(rings).to(dev), torch.full((1 << 14,), 7, dtype=torch.uint8, device=dev)
    outs, tot = torch.zeros((12, 32), dtype=torch.uint8, device=dev), torch.zeros(40, dtype=torch.uint8, device=dev)
    rx = torch.zeros((12, 32), dtype=torch.uint8, device=dev)
    idx = torch.zeros(12, dtype=torch.int32, device=dev)
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    good = dict(socks=table, n=12, so=None, sn=None, idx=None, n_rx=0, rings=rt, rings_bytes=rings.size, flags=0, align=1,
                frames=buf, frames_bytes=1 << 14, cap=100, outs=outs, tot=tot)

    def rejected(text, **kw):
        a = dict(good, **kw)
        st = eng.lib.fs_send_rings_resident(eng._ctx, P(a["socks"]), a["n"], P(a["so"]), P(a["sn"]), P(a["idx"]), a["n_rx"],
                                            P(a["rings"]), a["rings_bytes"], 0, a["flags"], a["align"], P(a["frames"]),
                                            a["frames_bytes"], a["cap"], None, None, None, None, P(a["outs"]), P(a["tot"]), None)
        msg = eng.lib.fs_last_error(eng._ctx).decode()
        assert st == (-1 if text else 0) and (text or "") in msg, (st, msg)

    rejected("flags must be FS_FCS_APPEND, FS_TX_WRITEBACK or both", flags=1)
    rejected("flags must be", flags=0x200)
    rejected("align must be a power of two from 1 to 4096", align=3)
    rejected("align must be", align=8192)
    rejected("n_socks above FS_SEND_MAX_SOCKS", n=65537)
    rejected("frames_cap above 2^31", cap=(1 << 31) + 1)
    rejected("null socks, socks_out or totals", socks=None)
    rejected("null socks, socks_out or totals", outs=None)
    rejected("null socks, socks_out or totals", tot=None)
    rejected("null rings", rings=None)
    rejected("null frames", frames=None)
    rejected("rx_snd_out without rx_socks_out", sn=rx)
    rejected("rx_index without rx_socks_out", idx=idx)
    rejected("n_rx must equal n_socks without rx_index", so=rx, n_rx=11)
    torch.cuda.synchronize()
    assert int(buf.min()) == 7 and int(outs.max()) == 0  # nothing ran
    # the boundaries pass: both flags, n_rx of its own with an index, null rings and frames of size 0
    rejected(None, flags=0x102, align=4096, so=rx, idx=idx, n_rx=1)
    rejected(None, rings=None, rings_bytes=0, frames=None, frames_bytes=0, cap=1 << 31)
    rejected(None, n=0, socks=None, outs=None, tot=None)
    torch.cuda.synchronize()
