"""The close call on the GPU (fs_close_flows_batch / fs_close_flows_batch_host) against the sequential
restatement of tests/close_ref.py, byte for byte: closers_out, socks_close and ctl_code over a sentinel
prefill, and every output of the accept call (tests/test_gpu_accept.py's comparison), which is also compared
with fs_accept_flows_batch from the same library on the same arguments. The batches are
tests/close_cases.py's, which tests/test_close_case_builders.py shows to reach what they name."""
import ctypes

import numpy as np
import pytest

import close_cases as cases
import close_ref as ref
import engines
import flows_ref as fref
from test_gpu_accept import compare_accept, prefill
from test_gpu_deliver import TAIL, compare_delivery, sentinel, to_device
from test_gpu_recv import compare_recv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()
    e = Engine(0)
    yield e
    e.close()


def compare_close(e, res):
    from seqs_amd import split_close

    got_c, got_s, got_ctl = split_close(*res[:3])
    for name, got, want in (("closers_out", got_c, e["closers_out"]), ("socks_close", got_s, e["socks_close"])):
        bad = np.flatnonzero((got.view(np.uint8).reshape(-1, 32) != want.view(np.uint8).reshape(-1, 32)).any(axis=1))
        assert bad.size == 0, f"{bad.size} {name} differ, first at {bad[:4]}: {got[bad[:2]]} for {want[bad[:2]]}"
    if got_ctl is not None:
        bad = np.flatnonzero(got_ctl != e["ctl_code"])
        assert bad.size == 0, f"{bad.size} ctl codes differ, first at {bad[:8]}: {got_ctl[bad[:8]]} for {e['ctl_code'][bad[:8]]}"


class SentinelEmpty:
    """torch.empty stand-in for one call: uint8 result tensors come back full of sentinel bytes, so that a
    record or a code the call fails to write shows."""

    def __init__(self, seed):
        import torch

        self.torch, self.real, self.g = torch, torch.empty, torch.Generator(device="cpu").manual_seed(700 + seed)

    def __enter__(self):
        def empty(shape, dtype=None, device=None, **kw):
            t = self.real(shape, dtype=dtype, device=device, **kw)
            if dtype == self.torch.uint8 and t.numel():
                t.copy_(self.torch.randint(1, 256, tuple(t.shape), dtype=self.torch.uint8, generator=self.g).to(t.device))
            return t

        self.torch.empty = empty
        return self

    def __exit__(self, *exc):
        self.torch.empty = self.real


def check(eng, case, batch=None, mtu=0, flags=0, synack_flags=0, payload=True, seed=0, e=None, parity=True, lead=1, ctl_code=True):
    """One fs_close_flows_batch of the case's frames (or `batch` = (buf, off, ln)) over sentinel-filled result
    tensors; everything compared with the restatement (`e`: an earlier check's), and with `parity` every
    accept-call output with fs_accept_flows_batch's on the same arguments. Returns the expected dict."""
    import torch

    from test_gpu_flows import compare

    buf, off, ln = fref.pack(case.frames, lead=lead) if batch is None else batch
    n = int(ln.size)
    room = int(ln.sum()) if payload else 0
    noise = np.random.default_rng(77 + seed).integers(0, 256, 3 + room + TAIL, dtype=np.uint8)
    rings = sentinel(case.rings_bytes, seed)
    syn0, out0, st0 = prefill(len(case.slots), seed)
    if e is None:
        e = ref.expected(buf, off, ln, mtu, flags, noise, 3, room, case.socks, case.snd, rings, case.listeners, case.slots,
                         synack_flags, syn0, case.closers)
    dev = torch.device("cuda:0")
    tb = to_device(buf, off, ln)

    def run(call, **more):
        pt, rt = torch.from_numpy(noise).to(dev), torch.from_numpy(rings).to(dev)
        st, ot, stt = torch.from_numpy(syn0).to(dev), torch.from_numpy(out0).to(dev), torch.from_numpy(st0).to(dev)
        with SentinelEmpty(seed):
            res = call(*tb, case.socks, case.snd, rt, case.listeners, case.slots, mtu=mtu, flags=flags, synack_flags=synack_flags,
                       payload=pt[3 : 3 + room] if payload else False, synacks=st, synack_results=(ot, stt), **more)
        torch.cuda.synchronize()
        return res, pt, rt

    res, pt, rt = run(lambda *a, **k: eng.close_flows_device(*a[:8], case.closers, ctl_code=ctl_code, **k))
    compare_close(e, res)
    acc = res[3:]
    compare_accept(e, acc, out0, st0, n)
    compare_recv(e, acc[6], acc[7])
    compare_delivery(e, acc[8], acc[9], rt)
    compare(e, pt.cpu().numpy(), *acc[11:])
    if parity:
        r, pt2, rt2 = run(eng.accept_flows_device)
        assert torch.equal(rt, rt2) and torch.equal(pt, pt2)
        cuts = (None,) * 10 + (None, e["n_runs"], e["n_flows"], e["n_accepted"], None, None, None, None)
        assert len(acc) == len(r) == len(cuts)
        for k, (x, y, cut) in enumerate(zip(acc, r, cuts)):
            assert (x is None and y is None) or torch.equal(x[:cut], y[:cut]), f"accept-call output {k} differs"
    return e


# ---- events and codes on every side of a chunk boundary ----------------------------------------------------

@pytest.mark.parametrize("n", [130, 258])
@pytest.mark.parametrize("which", range(len(cases.TRANSITIONS)), ids=[f"{cases.NAMES[s]}-{ev}" for s, ev, _ in cases.TRANSITIONS])
def test_event_at_every_position(eng, n, which):
    case = cases.event_at_positions(n, which)
    e = check(eng, case, seed=which, parity=n == 130)
    _, event, after = cases.TRANSITIONS[which]
    if not event.startswith("syn") and after in (0, 8):
        assert (e["closers_out"]["state"] == after).all()


@pytest.mark.parametrize("n", [130, 258])
def test_code_at_every_position(eng, n):
    e = check(eng, cases.codes_at_positions(n), seed=n)
    assert set(int(x) for x in e["ctl_code"]) >= {1, 4, 5, 7, 8, 10}


def test_several_events_in_one_chunk(eng):
    e = check(eng, cases.several_events())
    assert [int(x) for x in e["closers_out"]["state"]] == [8, 8, 0, 0, 0, 6]


def test_hostile_flow_of_64_fins(eng):
    e = check(eng, cases.hostile())
    assert [int(x) for x in e["closers_out"]["n_taken"]] == [64, 130, 5]


# ---- the continuations of Established sockets ---------------------------------------------------------------

def test_established_continuations(eng):
    case = cases.established()
    e = check(eng, case)
    names = case.info["names"]
    assert {names[s]: int(x) for s, x in enumerate(e["socks_close"]["state"])} == {
        "fin at 63": 9, "fin at 64": 9, "rst passes": 0, "rst fails": 4, "syn at stop": 4, "rst first": 0, "no flow": 4,
        "rst with data": 4}


def test_closer_and_listener(eng):
    e = check(eng, cases.closer_and_listener())
    assert int(e["conns"]["used"].sum()) == 3 and (e["closers_out"]["n_taken"] == 0).all()


# ---- columns, the table, the grid ------------------------------------------------------------------------------

def test_header_geometries(eng):
    e = check(eng, cases.geometries(), lead=3)
    assert (e["closers_out"]["state"] == 8).all()


def test_hash_masks_and_one_workgroup(eng):
    from seqs_amd import Engine
    from seqs_amd.framesum import TEST_LIB_PATH

    built = [cases.established(), cases.several_events(), cases.codes_at_positions(130)]
    es = [check(eng, c, parity=False) for c in built]
    te = Engine(0, lib_path=TEST_LIB_PATH)
    try:
        for mask in (0, 0xF):
            assert te.lib.fs_test_set_flow_hash_mask(te._ctx, mask) == 0
            for c, e in zip(built, es):
                check(te, c, e=e, parity=False)
        te.set_workgroups(1)
        for c, e in zip(built, es):
            check(te, c, e=e)
    finally:
        te.close()


@pytest.mark.parametrize("variant", engines.VARIANTS, ids=engines.IDS)
def test_every_engine(variant):
    import torch

    assert torch.cuda.is_available()
    e2 = engines.engine_for(variant)
    try:
        check(e2, cases.established())
    finally:
        e2.close()


# ---- scale -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", cases.BIG_SHAPES)
def test_65793_frames(eng, shape):
    case = cases.big(shape)
    e = check(eng, case, payload=False, seed=len(shape))
    if shape == "65536 closers":
        assert (e["closers_out"]["state"] == 8).all() and int((e["ctl_code"] == 1).sum()) == 65536
    else:
        assert (e["closers_out"]["state"] == 9).all() and (e["socks_close"]["state"] == 9).all()


# ---- degenerate calls ----------------------------------------------------------------------------------------

def test_empty_calls(eng):
    import torch

    from seqs_amd import split_close

    case = cases.established()
    none = ref.closers_of()
    # nobody closes and nobody is listed: the accept call plus a zeroed ctl_code
    bare = cases.CCase(case.frames, none)
    e = check(eng, bare)
    assert not e["ctl_code"].any() and len(e["closers_out"]) == 0 and len(e["socks_close"]) == 0
    # no closers, sockets listed; closers, no sockets
    check(eng, cases.CCase(case.frames, none, socks=case.socks, snd=case.snd, rings_bytes=case.rings_bytes))
    check(eng, cases.CCase(case.frames, case.closers))
    # ctl_code left out
    check(eng, case, ctl_code=False)
    # n == 0: every record as it came in
    buf, off, ln = fref.pack(case.frames)
    tb, to, tl = to_device(buf, off, ln)
    rings = torch.zeros(case.rings_bytes, dtype=torch.uint8, device=tb.device)
    with SentinelEmpty(3):
        res = eng.close_flows_device(tb, to[:0], tl[:0], case.socks, case.snd, rings, case.listeners, case.slots, case.closers)
    torch.cuda.synchronize()
    cout, sclose, ctl = split_close(*res[:3])
    for c, o in zip(case.closers, cout):
        assert [int(x) for x in o] == [int(c["state"]), int(c["rcv_nxt"]), int(c["snd_una"]), int(c["snd_wnd"]), 0, 0, ref.NONE, 0]
    for s, sn, o in zip(case.socks, case.snd, sclose):
        assert [int(x) for x in o] == [4, int(s["rcv_nxt"]), int(sn["snd_una"]), int(sn["snd_wnd"]), 0, 0, ref.NONE, 0]
    assert ctl.size == 0 and not bool(rings.any())


def test_8_calls_in_flight(eng):
    import torch

    dev = torch.device("cuda:0")
    built = [cases.established(), cases.several_events(), cases.hostile(), cases.codes_at_positions(130), cases.geometries(),
             cases.closer_and_listener(), cases.event_at_positions(130, 0), cases.established()]
    prepared = []
    for j, case in enumerate(built):
        buf, off, ln = fref.pack(case.frames, lead=j % 4, seed=j)
        noise = np.random.default_rng(j).integers(0, 256, 3 + TAIL, dtype=np.uint8)
        rings = sentinel(case.rings_bytes, j)
        syn0, out0, st0 = prefill(len(case.slots), j)
        e = ref.expected(buf, off, ln, 0, 0, noise, 3, 0, case.socks, case.snd, rings, case.listeners, case.slots, 0, syn0,
                         case.closers)
        prepared.append((e, to_device(buf, off, ln), case, torch.from_numpy(rings).to(dev), torch.from_numpy(syn0).to(dev),
                         torch.from_numpy(out0).to(dev), torch.from_numpy(st0).to(dev), out0, st0, int(ln.size)))
    torch.cuda.synchronize()
    with SentinelEmpty(8):
        res = [eng.close_flows_device(*tb, case.socks, case.snd, rt, case.listeners, case.slots, case.closers, payload=False,
                                      synacks=st, synack_results=(ot, stt))
               for (_, tb, case, rt, st, ot, stt, _, _, _) in prepared]
    torch.cuda.synchronize()
    for (e, _, _, rt, _, _, _, out0, st0, n), r in zip(prepared, res):
        compare_close(e, r)
        compare_accept(e, r[3:], out0, st0, n)
        compare_recv(e, r[9], r[10])
        compare_delivery(e, r[11], r[12], rt)


# ---- the host form ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["established", "several events"])
def test_host_form_equals_the_device_form(eng, which):
    case = cases.established() if which == "established" else cases.several_events()
    buf, off, ln = fref.pack(case.frames, lead=9)
    e = check(eng, case, batch=(buf, off, ln), seed=8, parity=False)
    rings = sentinel(case.rings_bytes, 8)
    res = eng.close_flows_host(buf, off, ln, case.socks, case.snd, rings, case.listeners, case.slots, case.closers, payload=False)
    cout, sclose, ctl, conns, lout, of, _, _, _, sn, code, so = res[:12]
    assert cout.tobytes() == e["closers_out"].tobytes() and sclose.tobytes() == e["socks_close"].tobytes()
    assert np.array_equal(ctl, e["ctl_code"]) and conns.tobytes() == e["conns"].tobytes() and np.array_equal(of, e["accept_of"])
    assert sn.tobytes() == e["snd_out"].tobytes() and np.array_equal(code, e["code"]) and so.tobytes() == e["socks_out"].tobytes()
    assert np.array_equal(rings, e["rings"])
    # each nullable array left out
    for kw in (dict(ctl_code=False), dict(code=False), dict(delivered=False), dict(accept_of=False), dict(synack_results=False)):
        r = eng.close_flows_host(buf, off, ln, case.socks, case.snd, sentinel(case.rings_bytes, 8), case.listeners, case.slots,
                                 case.closers, payload=False, **kw)
        assert r[0].tobytes() == e["closers_out"].tobytes() and r[1].tobytes() == e["socks_close"].tobytes()
        assert (r[2] is None) == ("ctl_code" in kw) and (r[2] is None or np.array_equal(r[2], e["ctl_code"]))
    # n of 0 on the host
    r = eng.close_flows_host(buf, off[:0], ln[:0], case.socks, case.snd, rings, case.listeners, case.slots, case.closers, payload=False)
    assert (r[0]["stop"] == ref.NONE).all() and (r[0]["state"] == case.closers["state"]).all() and not r[0]["n_taken"].any()
    assert (r[1]["state"] == 4).all() and np.array_equal(r[1]["rcv_nxt"], case.socks["rcv_nxt"])
    assert np.array_equal(r[1]["snd_una"], case.snd["snd_una"]) and (r[1]["stop"] == ref.NONE).all()


# ---- rejected calls ----------------------------------------------------------------------------------------------

def test_rejected_calls_leave_the_device_alone(eng):
    import torch

    from seqs_amd import FramesumError

    case = cases.established()
    nb = fref.pack(case.frames)
    tb = to_device(*nb)
    rings = torch.zeros(case.rings_bytes, dtype=torch.uint8, device=tb[0].device)

    def bad(field, value, row=1):
        c = case.closers.copy()
        c[field][row] = value
        return c

    twice = case.closers.copy()
    twice["key"][1] = twice["key"][0]
    listed = case.closers.copy()
    listed["key"][1] = case.socks["key"][2]
    reserved = case.closers.copy()
    reserved["reserved"][1][1] = 1
    rejected = ((bad("state", 4), "closer 1: state must be 5 .. 10"), (bad("state", 11), "closer 1: state must be 5 .. 10"),
                (bad("state", 0, 0), "closer 0: state must be 5 .. 10"), (bad("snd_wnd", 65536), "closer 1: snd_wnd above 65,535"),
                (bad("reserved2", 7), "closer 1: reserved must be 0"), (reserved, "closer 1: reserved must be 0"),
                (twice, "closer 1: its key equals an earlier closer's"), (listed, "closer 1: its key equals a listed socket's"))
    for closers, text in rejected:
        with pytest.raises(FramesumError, match="fs_close_flows_batch: " + text):
            eng.close_flows_device(*tb, case.socks, case.snd, rings, case.listeners, case.slots, closers)
        with pytest.raises(FramesumError, match="fs_close_flows_batch_host: " + text):
            eng.close_flows_host(*nb, case.socks, case.snd, np.zeros(case.rings_bytes, dtype=np.uint8), case.listeners, case.slots,
                                 closers)
    not_tcp = case.closers.copy()
    not_tcp["key"][0][0] = 17
    with pytest.raises(FramesumError, match=r"closer 0: key\[0\] must be 6"):
        eng.close_flows_device(*tb, case.socks, case.snd, rings, case.listeners, case.slots, not_tcp)
    # what the accept call rejects, the close call rejects under its own name
    with pytest.raises(FramesumError, match="fs_close_flows_batch: flags must be 0 or FS_RX_FCS"):
        eng.close_flows_device(*tb, case.socks, case.snd, rings, case.listeners, case.slots, case.closers, flags=2)
    with pytest.raises(FramesumError, match="fs_close_flows_batch: listener or slot 0: synack_flags"):
        eng.close_flows_device(*tb, case.socks, case.snd, rings, case.listeners, case.slots, case.closers, synack_flags=1)
    torch.cuda.synchronize()
    assert not bool(rings.any())
    # null pointers and the count, through the C ABI
    lib, vp = eng.lib, ctypes.c_void_p
    some, c1 = vp(tb[0].data_ptr()), vp(case.closers.ctypes.data)
    head = (eng._ctx, some, some, some, 1, 0, 0, None, 0, None, 0, None, None, None, None, None, None, 0, None, 0, 0, None, None, None,
            None, None, None)
    tail = (None, 0, some, some, some, None, some, None, None, None)
    for closing, text in (((c1, 2, None, None, None), b"null closers"), ((None, 2, some, None, None), b"null closers"),
                          ((c1, 65537, some, None, None), b"n_closers above 65,536")):
        assert lib.fs_close_flows_batch(*head, *closing, *tail) == -1
        assert text in lib.fs_last_error(eng._ctx)
    s1, n1 = vp(case.socks.ctypes.data), vp(case.snd.ctypes.data)
    with_socks = (eng._ctx, some, some, some, 1, 0, 0, s1, 1, vp(rings.data_ptr()), case.rings_bytes, some, None, n1, some, None, None, 0,
                  None, 0, 0, None, None, None, None, None, None)
    assert lib.fs_close_flows_batch(*with_socks, None, 0, None, None, None, *tail) == -1  # null socks_close with a socket
    assert b"socks_close" in lib.fs_last_error(eng._ctx)
