"""The connect call on the GPU (fs_connect_flows_batch / fs_connect_flows_batch_host) against the sequential
restatement of tests/connect_ref.py, byte for byte: openers_out, the whole replies buffer, reply_out,
reply_status and ctl_code over sentinel prefills, and every output of the close call (tests/test_gpu_close.py's
comparison), which is also compared with fs_close_flows_batch from the same library on the same arguments. The
batches are tests/connect_cases.py's, which tests/test_connect_case_builders.py shows to reach what they
name."""
import ctypes

import numpy as np
import pytest

import close_ref
import connect_cases as cases
import connect_ref as ref
import engines
import flows_ref as fref
from test_gpu_accept import compare_accept, prefill
from test_gpu_close import SentinelEmpty, compare_close
from test_gpu_deliver import TAIL, compare_delivery, sentinel, to_device
from test_gpu_recv import compare_recv

pytestmark = pytest.mark.gpu
REPLY_TAIL = 9  # bytes behind the last opener's 64, which no call may touch


@pytest.fixture(scope="module")
def eng():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()
    e = Engine(0)
    yield e
    e.close()


def reply_prefill(n_openers, seed):
    return np.random.default_rng(1300 + seed).integers(1, 256, n_openers * 64 + REPLY_TAIL, dtype=np.uint8)


def compare_connect(e, res):
    """openers_out, replies, reply_out and reply_status (res[:4]) against the restatement."""
    from seqs_amd import split_connect

    got, dig, st = split_connect(res[0], res[2], res[3])
    want = e["openers_out"]
    bad = np.flatnonzero((got.view(np.uint8).reshape(-1, 48) != want.view(np.uint8).reshape(-1, 48)).any(axis=1))
    assert bad.size == 0, f"{bad.size} openers_out differ, first at {bad[:4]}: {got[bad[:2]]} for {want[bad[:2]]}"
    bad = np.flatnonzero(res[1].cpu().numpy() != e["replies"])
    assert bad.size == 0, f"{bad.size} reply bytes differ, first at {bad[:8]} (openers {bad[:8] // 64})"
    if dig is not None:
        assert dig.tobytes() == e["reply_out"].tobytes(), (dig[:4], e["reply_out"][:4])
        assert np.array_equal(st, e["reply_status"]), (st[:16], e["reply_status"][:16])


def check(eng, case, batch=None, mtu=0, flags=0, reply_flags=None, payload=True, seed=0, e=None, parity=True, lead=1,
          ctl_code=True, reply_results=True):
    """One fs_connect_flows_batch of the case's frames (or `batch` = (buf, off, ln)) over sentinel-filled
    result tensors and a sentinel-filled replies buffer; everything compared with the restatement (`e`: an
    earlier check's), and with `parity` every close-call output with fs_close_flows_batch's on the same
    arguments. Returns the expected dict."""
    import torch

    from test_gpu_flows import compare

    buf, off, ln = fref.pack(case.frames, lead=lead) if batch is None else batch
    n = int(ln.size)
    room = int(ln.sum()) if payload else 0
    reply_flags = case.reply_flags if reply_flags is None else reply_flags
    noise = np.random.default_rng(77 + seed).integers(0, 256, 3 + room + TAIL, dtype=np.uint8)
    rings = sentinel(case.rings_bytes, seed)
    syn0, out0, st0 = prefill(len(case.slots), seed)
    rep0 = reply_prefill(len(case.openers), seed)
    if e is None:
        e = ref.expected(buf, off, ln, mtu, flags, noise, 3, room, case.socks, case.snd, rings, case.listeners, case.slots, 0, syn0,
                         case.closers, case.openers, reply_flags, rep0)
    dev = torch.device("cuda:0")
    tb = to_device(buf, off, ln)

    def run(call, **more):
        pt, rt = torch.from_numpy(noise).to(dev), torch.from_numpy(rings).to(dev)
        st, ot, stt = torch.from_numpy(syn0).to(dev), torch.from_numpy(out0).to(dev), torch.from_numpy(st0).to(dev)
        with SentinelEmpty(seed):
            res = call(*tb, case.socks, case.snd, rt, case.listeners, case.slots, case.closers, mtu=mtu, flags=flags,
                       payload=pt[3 : 3 + room] if payload else False, synacks=st, synack_results=(ot, stt), ctl_code=ctl_code, **more)
        torch.cuda.synchronize()
        return res, pt, rt

    res, pt, rt = run(lambda *a, **k: eng.connect_flows_device(*a, case.openers, reply_flags=reply_flags,
                                                               replies=torch.from_numpy(rep0).to(dev),
                                                               reply_results=reply_results, **k))
    compare_connect(e, res)
    cl = res[4:]
    compare_close(e, cl)
    acc = cl[3:]
    compare_accept(e, acc, out0, st0, n)
    compare_recv(e, acc[6], acc[7])
    compare_delivery(e, acc[8], acc[9], rt)
    compare(e, pt.cpu().numpy(), *acc[11:])
    if parity:
        r, pt2, rt2 = run(eng.close_flows_device)
        assert torch.equal(rt, rt2) and torch.equal(pt, pt2)
        # the close call's own codes: this call's with the openers' flows zeroed
        if ctl_code:
            assert np.array_equal(r[2].cpu().numpy(), e["close_ctl_code"])
        cuts = (None, None, 0) + (None,) * 10 + (None, e["n_runs"], e["n_flows"], e["n_accepted"], None, None, None, None)
        assert len(cl) == len(r) == len(cuts)
        for k, (x, y, cut) in enumerate(zip(cl, r, cuts)):
            assert (x is None and y is None) or torch.equal(x[:cut], y[:cut]), f"close-call output {k} differs"
    return e


def replies_through_the_digest(eng, e, reply_flags):
    """The replies as a batch of their own through fs_digest_batch (fs_digest_batch_fcs with the FCS): every
    one is accepted, and its digest is the call's reply_out."""
    import torch

    from seqs_amd import split_digests

    owing = np.flatnonzero(e["openers_out"]["reply"] != 0)
    size = 58 if reply_flags & 2 else 54
    dev = torch.device("cuda:0")
    frames = torch.from_numpy(np.ascontiguousarray(e["replies"])).to(dev)
    off = torch.from_numpy((owing * 64).astype(np.int64)).to(dev)
    ln = torch.full((owing.size,), size, dtype=torch.int32, device=dev)
    out, st = (eng.digest_fcs_device if reply_flags & 2 else eng.digest_device)(frames, off, ln)
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any()
    crc, ipc, l4c = split_digests(out.cpu().numpy())
    want = e["reply_out"][owing]
    assert np.array_equal(crc, want["crc32"]) and np.array_equal(ipc, want["ip_csum"]) and np.array_equal(l4c, want["l4_csum"])
    return owing.size


# ---- every rule on every side of a chunk boundary -----------------------------------------------------------

@pytest.mark.parametrize("n", [130, 258])
@pytest.mark.parametrize("which", range(len(cases.RULES)), ids=[f"rule{r}-{kind}" for r, kind, _ in cases.RULES])
def test_rule_at_every_position(eng, n, which):
    case = cases.rule_at_positions(n, which)
    e = check(eng, case, seed=which, parity=n == 130, reply_flags=2 * (which % 2))
    _, _, what = cases.RULES[which]
    if what in ("rst", "syn", 11):
        assert (e["openers_out"]["state"] == 3).all() and not (e["ctl_code"] == 1).any()  # untouched behind `stop`
    if what == 1:
        assert (e["openers_out"]["frame"] != ref.NONE).all()


def test_two_events_in_one_chunk_and_across_a_boundary(eng):
    e = check(eng, cases.two_events())
    assert [int(x) for x in e["openers_out"]["state"]] == [4, 2, 3, 4, 3, 3, 4]


def test_extremes_of_iss_seq_window_and_rcv_wnd(eng):
    e = check(eng, cases.extremes(), seed=2)
    assert {int(x) for x in e["openers_out"]["state"]} == {2, 3, 4}


@pytest.mark.parametrize("reply_flags", [0, 2])
def test_replies_back_through_the_digest(eng, reply_flags):
    case = cases.send_syn()
    e = check(eng, case, reply_flags=reply_flags, seed=reply_flags)
    assert replies_through_the_digest(eng, e, reply_flags) == 5
    case = cases.two_events()
    e = check(eng, case, reply_flags=reply_flags, seed=4, parity=False)
    assert replies_through_the_digest(eng, e, reply_flags) == 6


@pytest.mark.parametrize("mtu", [53, 54])
def test_mtu_verdict_of_the_replies(eng, mtu):
    # (at 53 the batch's own frames exceed the MTU too: nothing is accepted, and the flagged openers owe their SYNs)
    case = cases.send_syn()
    e = check(eng, case, mtu=mtu, seed=mtu)
    owing = e["openers_out"]["reply"] != 0
    assert owing.sum() == 5 and (e["reply_status"][owing] == (2 if mtu == 53 else 0)).all() and (e["n_accepted"] == 0) == (mtu == 53)


def test_send_syn(eng):
    case = cases.send_syn()
    e = check(eng, case)
    assert [int(x) for x in e["openers_out"]["reply"]] == case.info["replies"]


def test_header_geometries_and_mss_kinds(eng):
    case = cases.geometries()
    e = check(eng, case, lead=3)
    assert [int(x) for x in e["openers_out"]["peer_mss"]] == case.info["mss"]


def test_opener_and_listener(eng):
    e = check(eng, cases.opener_and_listener())
    assert int(e["conns"]["used"].sum()) == 3 and (e["openers_out"]["state"] == 2).all()


def test_openers_beside_sockets_closers_and_listeners(eng):
    e = check(eng, cases.mixed())
    assert [int(x) for x in e["openers_out"]["state"]] == [4, 2, 3, 3] and e["close_ctl_code"].any()


def test_keys_one_bit_away(eng):
    e = check(eng, cases.near_keys())
    assert [int(x) for x in np.flatnonzero(e["ctl_code"])] == [0, 1]


# ---- columns, the table, the grid ------------------------------------------------------------------------------

def test_hash_masks_and_one_workgroup(eng):
    from seqs_amd import Engine
    from seqs_amd.framesum import TEST_LIB_PATH

    built = [cases.mixed(), cases.two_events(), cases.rule_at_positions(130, 11)]
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


def test_three_lists_in_one_call(eng):
    """Listed sockets, closers and openers in one call (cases.three_lists: the three instantiations of the one
    match kernel, and the one gather behind the closers' and behind the openers' match), the first of each
    list with a flow of 66 slots: the device form under the hash masks 0, 1 and all ones with the workgroup cap
    at 1 and at its default, and the host form, whose arrays keep the caller's bytes outside the written entries."""
    from seqs_amd import Engine
    from seqs_amd.framesum import TEST_LIB_PATH

    case = cases.three_lists()
    e = check(eng, case, seed=21)
    te = Engine(0, lib_path=TEST_LIB_PATH)
    try:
        for workgroups in (1, 0):
            te.set_workgroups(workgroups)
            for mask in (0, 1, 0xFFFFFFFF):
                assert te.lib.fs_test_set_flow_hash_mask(te._ctx, mask) == 0
                check(te, case, seed=21, e=e, parity=False)
                host_form_of_three_lists(te, case, e)
    finally:
        te.close()


def host_form_of_three_lists(eng, case, e, seed=21):
    """fs_connect_flows_batch_host on check()'s batch and prefills: every array against the restatement `e`."""
    buf, off, ln = fref.pack(case.frames, lead=1)
    room = int(ln.sum())
    noise = np.random.default_rng(77 + seed).integers(0, 256, 3 + room + TAIL, dtype=np.uint8)
    rings, rep0 = sentinel(case.rings_bytes, seed), reply_prefill(len(case.openers), seed)
    syn0, out0, st0 = prefill(len(case.slots), seed)
    from seqs_amd.framesum import DIGEST_DTYPE

    syn_out, syn_st = out0.copy().view(DIGEST_DTYPE).reshape(-1), st0.copy()
    r = eng.connect_flows_host(buf, off, ln, case.socks, case.snd, rings, case.listeners, case.slots, case.closers, case.openers,
                               replies=rep0, payload=noise[3 : 3 + room], synacks=syn0, synack_results=(syn_out, syn_st))
    oout, replies, rout, rst, cout, sclose, ctl, conns, lout, of, synacks, _, _, snd_out, codes, socks_out, marks = r[:17]
    payload, runs, flows, order, run_of, totals, out, status = r[17:]
    assert oout.tobytes() == e["openers_out"].tobytes() and np.array_equal(replies, e["replies"])  # (the sentinel tail too)
    assert rout.tobytes() == e["reply_out"].tobytes() and np.array_equal(rst, e["reply_status"])
    assert cout.tobytes() == e["closers_out"].tobytes() and sclose.tobytes() == e["socks_close"].tobytes()
    assert np.array_equal(ctl, e["ctl_code"])
    assert conns.tobytes() == e["conns"].tobytes() and lout.tobytes() == e["listeners_out"].tobytes()
    assert np.array_equal(of, e["accept_of"]) and np.array_equal(synacks, e["synacks"])
    assert syn_out.tobytes() == out0.tobytes() and np.array_equal(syn_st, st0)  # no slot is filled: the caller's bytes
    assert snd_out.tobytes() == e["snd_out"].tobytes() and np.array_equal(codes, e["code"])
    assert socks_out.tobytes() == e["socks_out"].tobytes() and np.array_equal(marks, e["delivered"])
    assert np.array_equal(rings, e["rings"]) and np.array_equal(noise, e["payload"])
    assert (int(totals["payload_bytes"]), int(totals["n_runs"]), int(totals["n_flows"]), int(totals["n_accepted"])) == \
        (e["payload_bytes"], e["n_runs"], e["n_flows"], e["n_accepted"])
    assert runs.tobytes() == e["runs"].tobytes() and flows.tobytes() == e["flows"].tobytes()
    assert np.array_equal(order, e["order"]) and np.array_equal(run_of, e["run_of"])
    assert out.tobytes() == e["dig"].tobytes() and np.array_equal(status, e["st"])


@pytest.mark.parametrize("variant", engines.VARIANTS, ids=engines.IDS)
def test_every_engine(variant):
    import torch

    assert torch.cuda.is_available()
    e2 = engines.engine_for(variant)
    try:
        check(e2, cases.mixed())
    finally:
        e2.close()


# ---- scale -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", cases.BIG_SHAPES)
def test_65793_frames(eng, shape):
    case = cases.big(shape)
    e = check(eng, case, payload=False, seed=len(shape))
    out = e["openers_out"]
    if shape == "65536 openers":
        assert int((out["state"] == 4).sum()) == 65536 - 4096 and int((e["ctl_code"] == 11).sum()) == 4096
        assert int((e["ctl_code"] == 1).sum()) == 65536 - 4096
    else:
        assert (out["reply"] != 0).all() and (e["socks_close"]["state"] == 9).all() and int((out["state"] == 4).sum()) > 900


# ---- degenerate calls ----------------------------------------------------------------------------------------

def test_empty_calls(eng):
    import torch

    from seqs_amd import split_close, split_connect

    case = cases.mixed()
    none = ref.openers_of()
    # nobody dials: the close call; no launch is added (the openers' arrays are not touched: there are none)
    bare = cases.NCase(case.frames, none, closers=case.closers, listeners=case.listeners, slots=case.slots, socks=case.socks,
                       snd=case.snd, rings_bytes=case.rings_bytes)
    e = check(eng, bare)
    assert np.array_equal(e["ctl_code"], e["close_ctl_code"]) and len(e["openers_out"]) == 0
    # openers alone
    check(eng, cases.NCase(case.frames, case.openers))
    # ctl_code and the reply results left out
    check(eng, case, ctl_code=False)
    check(eng, case, reply_results=False)
    # n == 0: every record as it came in, and the flagged openers' first SYNs
    flagged = cases.send_syn()
    buf, off, ln = fref.pack(flagged.frames)
    tb, to, tl = to_device(buf, off, ln)
    rings = torch.zeros(64, dtype=torch.uint8, device=tb.device)
    rep0 = reply_prefill(len(flagged.openers), 5)
    e0 = ref.contract([], dict(), flagged.openers, 2, 0, rep0, np.zeros(0, np.uint8))
    with SentinelEmpty(3):
        res = eng.connect_flows_device(tb, to[:0], tl[:0], flagged.socks, flagged.snd, rings, flagged.listeners, flagged.slots,
                                       flagged.closers, flagged.openers, reply_flags=2, replies=torch.from_numpy(rep0).to(tb.device))
    torch.cuda.synchronize()
    compare_connect(e0, res)
    out, _, _ = split_connect(res[0])
    for o, r in zip(flagged.openers, out):
        iss = int(o["iss"])
        assert [int(x) for x in r] == [3, 0, 0, iss, iss + 1, 1, 0, 0, ref.NONE, ref.NONE, 0, 4 * int(o["flags"]), 0, 0]
    assert int((out["reply"] == ref.REPLY_SYN).sum()) == 5 and split_close(*res[4:7])[2].size == 0 and not bool(rings.any())
    assert replies_through_the_digest(eng, e0, 2) == 5


def test_8_calls_in_flight(eng):
    import torch

    dev = torch.device("cuda:0")
    built = [cases.mixed(), cases.two_events(), cases.send_syn(), cases.rule_at_positions(130, 11), cases.geometries(),
             cases.opener_and_listener(), cases.rule_at_positions(130, 7), cases.near_keys()]
    prepared = []
    for j, case in enumerate(built):
        buf, off, ln = fref.pack(case.frames, lead=j % 4, seed=j)
        noise = np.random.default_rng(j).integers(0, 256, 3 + TAIL, dtype=np.uint8)
        rings = sentinel(case.rings_bytes, j)
        syn0, out0, st0 = prefill(len(case.slots), j)
        rep0 = reply_prefill(len(case.openers), j)
        e = ref.expected(buf, off, ln, 0, 0, noise, 3, 0, case.socks, case.snd, rings, case.listeners, case.slots, 0, syn0,
                         case.closers, case.openers, 2 * (j % 2), rep0)
        prepared.append((e, to_device(buf, off, ln), case, torch.from_numpy(rings).to(dev), torch.from_numpy(syn0).to(dev),
                         torch.from_numpy(out0).to(dev), torch.from_numpy(st0).to(dev), out0, st0, int(ln.size),
                         torch.from_numpy(rep0).to(dev), 2 * (j % 2)))
    torch.cuda.synchronize()
    with SentinelEmpty(8):
        res = [eng.connect_flows_device(*tb, case.socks, case.snd, rt, case.listeners, case.slots, case.closers, case.openers,
                                        reply_flags=rf, replies=rp, payload=False, synacks=st, synack_results=(ot, stt))
               for (_, tb, case, rt, st, ot, stt, _, _, _, rp, rf) in prepared]
    torch.cuda.synchronize()
    for (e, _, _, rt, _, _, _, out0, st0, n, _, _), r in zip(prepared, res):
        compare_connect(e, r)
        compare_close(e, r[4:])
        compare_accept(e, r[7:], out0, st0, n)
        compare_recv(e, r[13], r[14])
        compare_delivery(e, r[15], r[16], rt)


# ---- the host form ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["mixed", "two events"])
def test_host_form_equals_the_device_form(eng, which):
    case = cases.mixed() if which == "mixed" else cases.two_events()
    buf, off, ln = fref.pack(case.frames, lead=9)
    e = check(eng, case, batch=(buf, off, ln), seed=8, parity=False, payload=False)
    rings = sentinel(case.rings_bytes, 8)
    rep0 = reply_prefill(len(case.openers), 8)
    res = eng.connect_flows_host(buf, off, ln, case.socks, case.snd, rings, case.listeners, case.slots, case.closers, case.openers,
                                 replies=rep0.copy(), payload=False)
    oout, replies, rout, rst, cout, sclose, ctl, conns = res[:8]
    assert oout.tobytes() == e["openers_out"].tobytes() and np.array_equal(replies, e["replies"])
    assert rout.tobytes() == e["reply_out"].tobytes() and np.array_equal(rst, e["reply_status"])
    assert cout.tobytes() == e["closers_out"].tobytes() and sclose.tobytes() == e["socks_close"].tobytes()
    assert np.array_equal(ctl, e["ctl_code"]) and conns.tobytes() == e["conns"].tobytes() and np.array_equal(rings, e["rings"])
    # each nullable array left out
    for kw in (dict(reply_results=False), dict(ctl_code=False), dict(code=False), dict(delivered=False), dict(accept_of=False),
               dict(synack_results=False)):
        r = eng.connect_flows_host(buf, off, ln, case.socks, case.snd, sentinel(case.rings_bytes, 8), case.listeners, case.slots,
                                   case.closers, case.openers, replies=rep0.copy(), payload=False, **kw)
        assert r[0].tobytes() == e["openers_out"].tobytes() and np.array_equal(r[1], e["replies"])
        assert (r[2] is None) == ("reply_results" in kw) and (r[6] is None) == ("ctl_code" in kw)
    # n of 0 on the host: the records as they came in, the flagged openers' SYNs built on the device
    flagged = case.openers.copy()
    flagged["flags"][::2] = 1
    e0 = ref.contract([], dict(), flagged, 0, 0, rep0, np.zeros(0, np.uint8))
    r = eng.connect_flows_host(buf, off[:0], ln[:0], case.socks, case.snd, rings, case.listeners, case.slots, case.closers, flagged,
                               replies=rep0.copy(), payload=False)
    assert r[0].tobytes() == e0["openers_out"].tobytes() and np.array_equal(r[1], e0["replies"])
    assert r[2].tobytes() == e0["reply_out"].tobytes() and np.array_equal(r[3], e0["reply_status"])
    assert (r[0]["reply"][::2] == ref.REPLY_SYN).all() and (r[4]["stop"] == close_ref.NONE).all()


# ---- rejected calls ----------------------------------------------------------------------------------------------

def test_rejected_calls_leave_the_device_alone(eng):
    import torch

    from seqs_amd import FramesumError

    case = cases.mixed()
    nb = fref.pack(case.frames)
    tb = to_device(*nb)
    rings = torch.zeros(case.rings_bytes, dtype=torch.uint8, device=tb[0].device)

    def bad(field, value, row=1):
        c = case.openers.copy()
        c[field][row] = value
        return c

    twice = case.openers.copy()
    twice["key"][1] = twice["key"][0]
    listed = case.openers.copy()
    listed["key"][1] = case.socks["key"][2]
    closing = case.openers.copy()
    closing["key"][2] = case.closers["key"][0]
    reserved = case.openers.copy()
    reserved["reserved"][1][1] = 1
    rejected = ((bad("flags", 2), "opener 1: flags must be 0 or FS_CN_SEND_SYN"), (bad("flags", 255, 0), "opener 0: flags must be 0"),
                (bad("reserved2", 7), "opener 1: reserved must be 0"), (reserved, "opener 1: reserved must be 0"),
                (twice, "opener 1: its key equals an earlier opener's"), (listed, "opener 1: its key equals a listed socket's"),
                (closing, "opener 2: its key equals a closer's"))
    for openers, text in rejected:
        with pytest.raises(FramesumError, match="fs_connect_flows_batch: " + text):
            eng.connect_flows_device(*tb, case.socks, case.snd, rings, case.listeners, case.slots, case.closers, openers)
        with pytest.raises(FramesumError, match="fs_connect_flows_batch_host: " + text):
            eng.connect_flows_host(*nb, case.socks, case.snd, np.zeros(case.rings_bytes, dtype=np.uint8), case.listeners, case.slots,
                                   case.closers, openers)
    not_tcp = case.openers.copy()
    not_tcp["key"][0][0] = 17
    with pytest.raises(FramesumError, match=r"opener 0: key\[0\] must be 6"):
        eng.connect_flows_device(*tb, case.socks, case.snd, rings, case.listeners, case.slots, case.closers, not_tcp)
    with pytest.raises(FramesumError, match="fs_connect_flows_batch: opener 0: reply_flags must be 0 or FS_FCS_APPEND"):
        eng.connect_flows_device(*tb, case.socks, case.snd, rings, case.listeners, case.slots, case.closers, case.openers, reply_flags=1)
    # what the close call rejects, the connect call rejects under its own name
    with pytest.raises(FramesumError, match="fs_connect_flows_batch: flags must be 0 or FS_RX_FCS"):
        eng.connect_flows_device(*tb, case.socks, case.snd, rings, case.listeners, case.slots, case.closers, case.openers, flags=2)
    worse = case.closers.copy()
    worse["state"][0] = 4
    with pytest.raises(FramesumError, match="fs_connect_flows_batch: closer 0: state must be 5 .. 10"):
        eng.connect_flows_device(*tb, case.socks, case.snd, rings, case.listeners, case.slots, worse, case.openers)
    torch.cuda.synchronize()
    assert not bool(rings.any())
    # null pointers and the count, through the C ABI
    lib, vp = eng.lib, ctypes.c_void_p
    some, o1 = vp(tb[0].data_ptr()), vp(case.openers.ctypes.data)
    head = (eng._ctx, some, some, some, 1, 0, 0, None, 0, None, 0, None, None, None, None, None, None, 0, None, 0, 0, None, None, None,
            None, None, None, None, 0, None, None, None)
    tail = (None, 0, some, some, some, None, some, None, None, None)
    for opening, text in (((o1, 2, 0, None, some, None, None), b"null openers"), ((None, 2, 0, some, some, None, None), b"null openers"),
                          ((o1, 2, 0, some, None, None, None), b"null openers"),
                          ((o1, 65537, 0, some, some, None, None), b"n_openers above 65,536")):
        assert lib.fs_connect_flows_batch(*head, *opening, *tail) == -1
        assert text in lib.fs_last_error(eng._ctx)
