"""The receive call on the GPU (fs_recv_flows_batch / fs_recv_flows_batch_host) against the sequential
restatement of tests/recv_ref.py, bit for bit: snd_out and code, and every output of the delivery
(tests/test_gpu_deliver.py's comparison: socks_out, delivered, the WHOLE rings buffer, the flow-aware
coalesce's arrays), which is also compared with fs_deliver_flows_batch from the same library. The
batches are tests/recv_cases.py's, which tests/test_recv_case_builders.py shows to reach what they name."""
import ctypes

import numpy as np
import pytest

import deliver_cases as dcases
import engines
import flows_ref as fref
import recv_cases as cases
import recv_ref as ref
import send_ref
from test_gpu_deliver import TAIL, compare_delivery, many_flows, sentinel, three_flows, to_device

pytestmark = pytest.mark.gpu

M32 = 1 << 32


@pytest.fixture(scope="module")
def eng():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()
    e = Engine(0)
    yield e
    e.close()


def compare_recv(e, snd_out, code):
    from seqs_amd import split_snd

    got = split_snd(snd_out)
    assert got.tobytes() == e["snd_out"].tobytes(), (got[:8], e["snd_out"][:8])
    if code is not None:
        c = code.cpu().numpy()
        bad = np.flatnonzero(c != e["code"])
        assert bad.size == 0, f"{bad.size} codes differ, first at {bad[:8]}: {c[bad[:8]]} for {e['code'][bad[:8]]}"


def check(eng, batch, socks, snd, rings_bytes, mtu=0, flags=0, payload=True, delivered=True, code=True, seed=0, e=None,
          parity=False):
    """One fs_recv_flows_batch of `batch` = (buf, off, ln) with the sockets over a sentinel-filled rings
    buffer; everything compared with the restatement (`e`: an earlier check's), and with `parity` the
    delivery's outputs with fs_deliver_flows_batch's. Returns the expected dict."""
    import torch

    from test_gpu_flows import compare

    buf, off, ln = batch
    room = int(ln.sum()) if payload else 0
    noise = np.random.default_rng(77 + seed).integers(0, 256, 3 + room + TAIL, dtype=np.uint8)
    rings = sentinel(rings_bytes, seed)
    if e is None:
        e = ref.expected(buf, off, ln, mtu, flags, noise, 3, room, socks, snd, rings)
    dev = torch.device("cuda:0")
    pt, rt = torch.from_numpy(noise).to(dev), torch.from_numpy(rings).to(dev)
    tb = to_device(buf, off, ln)
    res = eng.recv_flows_device(*tb, socks, snd, rt, mtu, flags, payload=pt[3 : 3 + room] if payload else False,
                                delivered=delivered, code=code)
    torch.cuda.synchronize()
    compare_recv(e, res[0], res[1])
    compare_delivery(e, res[2], res[3], rt)
    compare(e, pt.cpu().numpy(), *res[5:])
    if parity:
        pt2, rt2 = torch.from_numpy(noise).to(dev), torch.from_numpy(rings).to(dev)
        d = eng.deliver_flows_device(*tb, socks, rt2, mtu, flags, payload=pt2[3 : 3 + room] if payload else False,
                                     delivered=delivered)
        torch.cuda.synchronize()
        assert torch.equal(rt, rt2) and torch.equal(pt, pt2) and torch.equal(res[2], d[0])
        cuts = (None, None, e["n_runs"], e["n_flows"], e["n_accepted"], None, None, None, None)
        for x, y, cut in zip(res[3:], d[1:], cuts):
            assert (x is None and y is None) or torch.equal(x[:cut], y[:cut])
    return e


def check_case(eng, case, lead=1, **kw):
    return check(eng, fref.pack(case.frames, lead=lead), case.socks, case.snd, case.rings_bytes, **kw)


def snd_behind(socks, back=100, wnd=1000):
    """A send side for sockets that come without one: snd.UNA `back` behind snd.NXT."""
    return ref.snd_of(*[((int(s["snd_nxt"]) - back) % M32, wnd) for s in socks])


# ---- parity with the delivery ----------------------------------------------------------------------

@pytest.mark.parametrize("which", ["three flows", "wrap", "restart"])
def test_parity_with_the_delivery(eng, which):
    if which == "three flows":
        from test_gpu_deliver import sock_for

        hdrs, frames = three_flows(np.random.default_rng(11))
        socks = dcases.ref.socks_of(sock_for(hdrs[2], 3000, 7, 600), sock_for(hdrs[0], 1000, 700, 500))
        batch, rings_bytes = fref.pack(frames, lead=1), 1300
    else:
        case = dcases.wrap_splits_small() if which == "wrap" else dcases.restart_patterns()
        batch, socks, rings_bytes = case.batch, case.socks, case.rings_bytes
    e = check(eng, batch, socks, snd_behind(socks), rings_bytes, parity=True)
    assert (e["snd_out"]["n_taken"] == e["socks_out"]["n_delivered"]).all() and e["code"].any()


# ---- lane and chunk positions ----------------------------------------------------------------------

@pytest.mark.parametrize("n,code,positions", cases.LANE_FLOWS)
def test_every_code_at_the_lane_and_chunk_positions(eng, n, code, positions):
    case = cases.lane_flow(n, code, positions)
    e = check_case(eng, case, lead=code % 4, seed=n + code)
    assert all(int(e["code"][p]) == code for p in case.info["positions"])


# ---- composition, keepalive, stop, options ---------------------------------------------------------

@pytest.mark.parametrize("name", cases.COMPOSITIONS)
def test_composition(eng, name):
    case = cases.composition(name)
    e = check_case(eng, case, seed=len(name))
    assert [int(c) for c in e["code"]] == case.info["codes"] and int(e["snd_out"]["snd_una"][0]) == case.info["una"]


def test_keepalive(eng):
    case = cases.keepalives()
    e = check_case(eng, case)
    assert [int(c) for c in e["code"]] == case.info["codes"] and int(e["snd_out"]["n_keepalive"][0]) == 2


@pytest.mark.parametrize("kind", cases.STOPS)
def test_stop(eng, kind):
    case = cases.stops(kind)
    e = check_case(eng, case, lead=2)
    assert [int(c) for c in e["code"]] == case.info["codes"] and int(e["snd_out"]["flags"][0]) == case.info["flags"]


def test_options(eng):
    case = cases.geometries()
    e = check_case(eng, case, lead=3)
    assert [int(c) for c in e["code"]] == case.info["codes"] and int(e["snd_out"]["snd_wnd"][0]) == 7008


# ---- random batches --------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", engines.VARIANTS, ids=engines.IDS)
def test_random_batches(variant):
    import torch

    assert torch.cuda.is_available()
    case = cases.random_flows()
    e2 = engines.engine_for(variant)
    try:
        e = check_case(e2, case, lead=2, parity=variant == engines.VARIANTS[0])
    finally:
        e2.close()
    assert (np.bincount(e["code"], minlength=7)[1:] > 20).all()


# ---- scale -----------------------------------------------------------------------------------------

def test_300_flows_300_sockets(eng):
    batch, socks = many_flows()
    e = check(eng, batch, socks, snd_behind(socks), 40 * 300 + 8)
    assert int(e["snd_out"]["n_taken"].sum()) == 900 and (e["code"] == 1).all()
    assert (e["snd_out"]["snd_una"] == socks["snd_nxt"]).all() and (e["snd_out"]["flags"] == ref.ACK_OWED).all()


@pytest.mark.parametrize("shape", ["one flow", "1000 flows", "every frame its own flow"])
def test_more_than_65536_frames(eng, shape):
    case = dcases.big_batches(shape)
    e = check(eng, case.batch, case.socks, snd_behind(case.socks), case.rings_bytes, payload=False, seed=len(shape))
    assert int((e["code"] != 0).sum()) == int(e["socks_out"]["n_delivered"].sum() + e["socks_out"]["n_dropped"].sum())
    assert int(e["snd_out"]["n_taken"].sum()) > 65000


def test_hash_mask_and_one_workgroup(eng):
    from seqs_amd import Engine
    from seqs_amd.framesum import TEST_LIB_PATH

    case = cases.random_flows(with_sockets=50)
    batch = fref.pack(case.frames, lead=1)
    e = check(eng, batch, case.socks, case.snd, case.rings_bytes)
    lane = cases.lane_flow(258, 2)
    te = Engine(0, lib_path=TEST_LIB_PATH)
    try:
        for mask in (0, 0xF):
            assert te.lib.fs_test_set_flow_hash_mask(te._ctx, mask) == 0
            check(te, batch, case.socks, case.snd, case.rings_bytes, e=e)
        te.set_workgroups(1)
        check(te, batch, case.socks, case.snd, case.rings_bytes, e=e)
        check_case(te, lane)
    finally:
        te.close()


# ---- degenerate calls ------------------------------------------------------------------------------

def test_sockets_without_a_flow_and_empty_calls(eng):
    import torch

    from seqs_amd import split_flows, split_snd, split_socks

    case = cases.composition("una goes back")
    stranger = dcases.ref.sock(bytes([6]) + bytes(range(12)), 5, 4200, 64, snd_nxt=50)
    socks = dcases.ref.socks_of(stranger, case.socks)
    snd = ref.snd_of((40, 123), (int(case.snd["snd_una"][0]), int(case.snd["snd_wnd"][0])))
    batch = fref.pack(case.frames, lead=1)
    e = check(eng, batch, socks, snd, 4300)
    assert e["snd_out"][0].tobytes() == np.array([(40, 123, 0, 0, 0, 0, 0, 0)], dtype=e["snd_out"].dtype).tobytes()
    assert int(e["snd_out"]["snd_una"][1]) == case.info["una"]
    # code NULL, payload NULL, delivered NULL
    for kw in (dict(code=False), dict(payload=False), dict(delivered=False, code=False, payload=False)):
        e2 = check(eng, batch, socks, snd, 4300, **kw)
        assert e2["snd_out"].tobytes() == e["snd_out"].tobytes() and np.array_equal(e2["code"], e["code"])
    # n == 0: zero totals, the input state
    tb, to, tl = to_device(*batch)
    rings = torch.from_numpy(sentinel(4300)).to(tb.device)
    res = eng.recv_flows_device(tb, to[:0], tl[:0], socks, snd, rings)
    torch.cuda.synchronize()
    assert bytes(split_flows(*res[5:8], res[9])[3].tobytes()) == bytes(24) and res[1].numel() == 0
    so, sn = split_socks(res[2]), split_snd(res[0])
    for s in range(2):
        assert (int(sn[s]["snd_una"]), int(sn[s]["snd_wnd"])) == (int(snd[s]["snd_una"]), int(snd[s]["snd_wnd"]))
        assert [int(sn[s][k]) for k in ("n_taken", "n_dup", "n_unsent", "n_rejected", "n_keepalive", "flags")] == [0] * 6
        assert int(so[s]["rcv_nxt"]) == int(socks[s]["rcv_nxt"]) and int(so[s]["flow"]) == ref.NONE
    assert np.array_equal(rings.cpu().numpy(), sentinel(4300))
    # n_socks == 0: the delivery with no sockets, plus a zeroed code
    none = dcases.ref.socks_of()
    e0 = check(eng, batch, none, ref.snd_of(), 64, parity=True)
    assert not e0["code"].any() and e0["snd_out"].size == 0


# ---- back-to-back calls ----------------------------------------------------------------------------

def test_back_to_back_calls_need_no_synchronization(eng):
    import torch

    from test_gpu_flows import compare

    dev = torch.device("cuda:0")
    built = [cases.lane_flow(130, 2), cases.random_flows(8, 30, 6601), cases.composition("half in a full chunk"),
             cases.lane_flow(258, 6), cases.random_flows(64, 12, 6602), cases.keepalives(), cases.lane_flow(130, 1, (63,)),
             cases.random_flows(3, 200, 6603)]
    prepared = []
    for j, case in enumerate(built):
        buf, off, ln = fref.pack(case.frames, lead=j % 4, seed=j)
        room = int(ln.sum())
        noise = np.random.default_rng(j).integers(0, 256, room + TAIL, dtype=np.uint8)
        rings = sentinel(case.rings_bytes, j)
        e = ref.expected(buf, off, ln, 0, 0, noise, 0, room, case.socks, case.snd, rings)
        prepared.append((e, to_device(buf, off, ln), case, torch.from_numpy(noise).to(dev), torch.from_numpy(rings).to(dev), room))
    torch.cuda.synchronize()
    res = [eng.recv_flows_device(*tb, case.socks, case.snd, rt, payload=pt[:room]) for _, tb, case, pt, rt, room in prepared]
    torch.cuda.synchronize()
    for (e, _, _, pt, rt, _), r in zip(prepared, res):
        compare_recv(e, r[0], r[1])
        compare_delivery(e, r[2], r[3], rt)
        compare(e, pt.cpu().numpy(), *r[5:])


# ---- the host form ---------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["random", "lanes"])
def test_host_form_equals_the_device_form(eng, which):
    case = cases.random_flows(16, 40, 6610, with_sockets=12) if which == "random" else cases.lane_flow(258, 3)
    buf, off, ln = fref.pack(case.frames, lead=9)
    e = check(eng, (buf, off, ln), case.socks, case.snd, case.rings_bytes, seed=8)
    room = int(ln.sum())
    noise = np.random.default_rng(77 + 8).integers(0, 256, 3 + room + TAIL, dtype=np.uint8)
    rings, mine = sentinel(case.rings_bytes, 8), noise.copy()
    sn, code, so, dl, pay, runs, flows, order, run_of, totals, dig, st = eng.recv_flows_host(
        buf, off, ln, case.socks, case.snd, rings, payload=mine[3 : 3 + room])
    assert sn.tobytes() == e["snd_out"].tobytes() and np.array_equal(code, e["code"])
    assert so.tobytes() == e["socks_out"].tobytes() and np.array_equal(dl, e["delivered"]) and np.array_equal(rings, e["rings"])
    assert np.array_equal(mine, e["payload"]) and runs.tobytes() == e["runs"].tobytes() and flows.tobytes() == e["flows"].tobytes()
    assert np.array_equal(order, e["order"]) and np.array_equal(run_of, e["run_of"]) and np.array_equal(st, e["st"])
    # n of 0 on the host, and no code array
    sn = eng.recv_flows_host(buf, off[:0], ln[:0], case.socks, case.snd, rings, payload=False)[0]
    assert [int(x) for x in sn["snd_una"]] == [int(x) for x in case.snd["snd_una"]] and not sn["flags"].any()
    res = eng.recv_flows_host(buf, off, ln, case.socks, case.snd, sentinel(case.rings_bytes, 8), payload=False, code=False)
    assert res[1] is None and res[0].tobytes() == e["snd_out"].tobytes()


# ---- rejected calls --------------------------------------------------------------------------------

def test_rejected_calls(eng):
    import torch

    from seqs_amd import FramesumError

    case = cases.composition("no ACK flag")
    tb, to, tl = to_device(*fref.pack(case.frames))
    rings = torch.zeros(case.rings_bytes, dtype=torch.uint8, device=tb.device)
    good = case.socks
    snd_nxt = int(good["snd_nxt"][0])
    for snd, text in ((ref.snd_of((snd_nxt - 5, 65536)), "socket 0: snd_wnd above 65,535"),
                      (ref.snd_of((snd_nxt + 1, 10)), "socket 0: snd_una is ahead of snd_nxt"),
                      (ref.snd_of((snd_nxt + (1 << 31) - 1, 10)), "socket 0: snd_una is ahead of snd_nxt")):
        with pytest.raises(FramesumError, match=text):
            eng.recv_flows_device(tb, to, tl, good, snd, rings)
        with pytest.raises(FramesumError, match=text):
            eng.recv_flows_host(*fref.pack(case.frames), good, snd, np.zeros(case.rings_bytes, dtype=np.uint8))
    eng.recv_flows_device(tb, to, tl, good, ref.snd_of((snd_nxt + (1 << 31), 65535)), rings)  # 2^31 behind passes
    # everything the delivery rejects
    bad = good.copy()
    bad["ring_size"] = 0
    with pytest.raises(FramesumError, match="socket 0: ring_size must be"):
        eng.recv_flows_device(tb, to, tl, bad, case.snd, rings)
    with pytest.raises(FramesumError):
        eng.recv_flows_device(tb, to, tl, good, case.snd, rings, flags=2)
    # null snd or snd_out
    lib, vp = eng.lib, ctypes.c_void_p
    some, s1, n1 = vp(tb.data_ptr()), vp(good.ctypes.data), vp(case.snd.ctypes.data)
    for snd_p, out_p in ((None, some), (n1, None)):
        assert lib.fs_recv_flows_batch(eng._ctx, some, some, some, 1, 0, 0, s1, 1, some, case.rings_bytes, some, None, snd_p,
                                       out_p, None, None, 0, some, some, some, None, some, None, None, None) == -1
        assert b"null snd or snd_out" in lib.fs_last_error(eng._ctx)
    torch.cuda.synchronize()
    assert not bool(rings.any())


# ---- the round trip --------------------------------------------------------------------------------

def test_round_trip_into_the_ring_send(eng):
    import torch

    from seqs_amd import split_snd, split_socks, tx_sock_from
    from seqs_amd.framesum import TX_ACK
    from test_gpu_send_rings import check_device

    case = cases.round_trip()
    batch = fref.pack(case.frames, lead=1)
    e = check(eng, batch, case.socks, case.snd, case.rings_bytes)
    tb = to_device(*batch)
    rings = torch.from_numpy(sentinel(case.rings_bytes)).to(tb[0].device)
    res = eng.recv_flows_device(*tb, case.socks, case.snd, rings)
    torch.cuda.synchronize()
    # the TX side: 100 unsent bytes per socket, 10 in flight behind a window of 0
    rng = np.random.default_rng(97)
    tx = [send_ref.sock(fref.flow_header(rng, 0x9700 + s), 20, 1 + 130 * s, 128, 100 + s, 100, snd_una=990, snd_nxt=1000, snd_wnd=0)
          for s in range(3)]
    tx_rings = send_ref.filled_rings(rng, tx)
    got = tx_sock_from(split_socks(res[2]), send_ref.socks_of(tx), snd_out=split_snd(res[0]))
    # ... and from the reference's state
    want = []
    for s, t in enumerate(tx):
        so, sn = e["socks_out"][s], e["snd_out"][s]
        want.append(dict(t, rcv_nxt=int(so["rcv_nxt"]), rcv_wnd=int(so["ring_free"]), snd_una=int(sn["snd_una"]),
                         snd_wnd=int(sn["snd_wnd"]), flags=TX_ACK if int(sn["flags"]) & ref.ACK_OWED else 0))
    assert got.tobytes() == send_ref.socks_of(want).tobytes()
    *_, outs = check_device(eng, want, tx_rings)
    # the window a pure ACK opened sends; a duplicate's window is not taken: nothing is sent
    assert [int(x) for x in outs["bytes"]] == [55, 0, 22] and [int(x) for x in outs["n_frames"]] == [3, 0, 2]
