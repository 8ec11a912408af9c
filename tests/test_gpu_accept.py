"""The accept call on the GPU (fs_accept_flows_batch / fs_accept_flows_batch_host) against the sequential
restatement of tests/accept_ref.py, byte for byte: conns, listeners_out, accept_of, the WHOLE synacks buffer
and synack_out / synack_status over a sentinel prefill (so that the bytes that must stay unwritten are
compared too), and every output of the receive call (tests/test_gpu_recv.py's comparison), which is also
compared with fs_recv_flows_batch from the same library on the same arguments. The batches are
tests/accept_cases.py's, which tests/test_accept_case_builders.py shows to reach what they name."""
import ctypes

import numpy as np
import pytest

import accept_cases as cases
import accept_ref as ref
import engines
import flows_ref as fref
import recv_ref
from test_gpu_deliver import TAIL, compare_delivery, sentinel, to_device
from test_gpu_recv import compare_recv

pytestmark = pytest.mark.gpu

SYN_TAIL = 40  # sentinel bytes behind the last slot's 64


@pytest.fixture(scope="module")
def eng():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()
    e = Engine(0)
    yield e
    e.close()


def prefill(n_slots, seed):
    """(synacks, synack_out as (n_slots, 2) int32, synack_status) full of sentinel bytes."""
    rng = np.random.default_rng(900 + seed)
    return (rng.integers(0, 256, n_slots * ref.STRIDE + SYN_TAIL, dtype=np.uint8),
            rng.integers(-2**31, 2**31, (n_slots, 2), dtype=np.int64).astype(np.int32),
            rng.integers(0, 256, n_slots, dtype=np.uint8))


def want_results(e, out0, st0):
    """synack_out (as raw bytes per slot) and synack_status: the prefill, the filled slots' entries in."""
    used = e["conns"]["used"] == 1
    out = np.ascontiguousarray(out0).view(np.uint8).reshape(-1, 8).copy()
    out[used] = e["synack_out"].view(np.uint8).reshape(-1, 8)[used]
    st = st0.copy()
    st[used] = e["synack_status"][used]
    return out, st


def compare_accept(e, res, out0, st0, n):
    from seqs_amd import split_accept

    conns, lout, of, synacks, syn_out, syn_st = res[:6]
    got_c, got_l, got_of = split_accept(conns, lout, of)
    bad = np.flatnonzero((got_c.view(np.uint8).reshape(-1, 48) != e["conns"].view(np.uint8).reshape(-1, 48)).any(axis=1))
    assert bad.size == 0, f"{bad.size} conns differ, first at {bad[:4]}: {got_c[bad[:2]]} for {e['conns'][bad[:2]]}"
    assert got_l.tobytes() == e["listeners_out"].tobytes(), (got_l[:8], e["listeners_out"][:8])
    if got_of is not None:
        bad = np.flatnonzero(got_of[:n] != e["accept_of"])
        assert bad.size == 0, f"{bad.size} accept_of differ, first at {bad[:8]}: {got_of[bad[:8]]} for {e['accept_of'][bad[:8]]}"
    bad = np.flatnonzero(synacks.cpu().numpy() != e["synacks"])
    assert bad.size == 0, f"{bad.size} synack bytes differ, first at {bad[:8]}"
    if syn_out is not None:
        want_out, want_st = want_results(e, out0, st0)
        assert np.array_equal(syn_out.cpu().numpy().view(np.uint8).reshape(-1, 8), want_out)
        assert np.array_equal(syn_st.cpu().numpy(), want_st)


def check(eng, case, batch=None, mtu=0, flags=0, synack_flags=0, payload=True, seed=0, e=None, parity=False, lead=1,
          accept_of=True, synack_results=True):
    """One fs_accept_flows_batch of the case's frames (or `batch` = (buf, off, ln)); everything compared with
    the restatement (`e`: an earlier check's), and with `parity` the receive call's outputs with
    fs_recv_flows_batch's. Returns the expected dict."""
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
                         synack_flags, syn0)
    dev = torch.device("cuda:0")
    pt, rt = torch.from_numpy(noise).to(dev), torch.from_numpy(rings).to(dev)
    st, ot, stt = torch.from_numpy(syn0).to(dev), torch.from_numpy(out0).to(dev), torch.from_numpy(st0).to(dev)
    tb = to_device(buf, off, ln)
    res = eng.accept_flows_device(*tb, case.socks, case.snd, rt, case.listeners, case.slots, mtu, flags, synack_flags,
                                  payload=pt[3 : 3 + room] if payload else False, accept_of=accept_of, synacks=st,
                                  synack_results=(ot, stt) if synack_results else False)
    torch.cuda.synchronize()
    compare_accept(e, res, out0, st0, n)
    compare_recv(e, res[6], res[7])
    compare_delivery(e, res[8], res[9], rt)
    compare(e, pt.cpu().numpy(), *res[11:])
    if parity:
        pt2, rt2 = torch.from_numpy(noise).to(dev), torch.from_numpy(rings).to(dev)
        r = eng.recv_flows_device(*tb, case.socks, case.snd, rt2, mtu, flags, payload=pt2[3 : 3 + room] if payload else False)
        torch.cuda.synchronize()
        assert torch.equal(rt, rt2) and torch.equal(pt, pt2)
        cuts = (None, None, None, None, None, e["n_runs"], e["n_flows"], e["n_accepted"], None, None, None, None)
        for x, y, cut in zip(res[6:], r, cuts):
            assert (x is None and y is None) or torch.equal(x[:cut], y[:cut])
    return e


def filled(e):
    return [int(s) for s in np.flatnonzero(e["conns"]["used"])]


# ---- one listener: ranks across wave and scan-block boundaries, every slot count ---------------------

@pytest.mark.parametrize("n_slots", [9, 8, 1, 0])
def test_one_listener_candidates_across_the_boundaries(eng, n_slots):
    case = cases.lanes(n_slots)
    e = check(eng, case, parity=n_slots == 9, seed=n_slots)
    took = [int(e["accept_of"][f]) for f in cases.LANE_CANDIDATES]
    assert took == list(range(n_slots)) + [ref.FULL] * (9 - n_slots) and filled(e) == list(range(n_slots))
    assert [int(x) for x in e["listeners_out"][0]] == [9, n_slots, 9 - n_slots, 0]
    assert int((e["accept_of"] == ref.NONE).sum()) == 300 - 9


def test_three_listeners_interleaved(eng):
    case = cases.three_listeners()
    e = check(eng, case, parity=True, synack_flags=ref.FCS_APPEND)
    assert [int(x) for x in e["listeners_out"]["n_syn"]] == case.info["n_syn"]
    assert [int(x) for x in e["listeners_out"]["n_accepted"]] == case.info["n_accepted"]
    assert filled(e) == [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14]


# ---- what is no candidate -------------------------------------------------------------------------

def test_socket_second_frame_and_bad_checksum(eng):
    case = cases.near_misses()
    e = check(eng, case, parity=True)
    assert [int(x) for x in e["accept_of"][:3]] == case.info["accept_of"] and e["n_flows"] == 3 and int(e["st"][3]) == 13
    assert filled(e) == [0] and int(e["conns"]["frame"][0]) == 4


def test_grid_of_first_frames(eng):
    case = cases.grid()
    for flags in (0, ref.FCS_APPEND):
        e = check(eng, case, synack_flags=flags, seed=flags)
        m = case.info["misses"]
        assert (e["accept_of"][:m] == ref.NONE).all() and list(e["accept_of"][m : len(case.frames)]) == list(range(len(cases.GRID_GOOD)))


def test_header_geometries_and_mss(eng):
    case = cases.geometries()
    e = check(eng, case, lead=3)
    assert [int(x) for x in e["conns"]["peer_mss"]] == case.info["mss"] and (e["conns"]["used"] == 1).all()


# ---- the SYN-ACKs through the digest ----------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, ref.FCS_APPEND])
def test_synacks_through_the_digest(eng, flags):
    import torch

    from seqs_amd import split_digests

    case = cases.three_listeners()
    e = check(eng, case, synack_flags=flags, seed=3)
    slots = filled(e)
    size = 58 if flags else 54
    buf = np.ascontiguousarray(e["synacks"][: len(case.slots) * ref.STRIDE])
    off = np.array(slots, dtype=np.uint64) * np.uint64(ref.STRIDE)
    ln = np.full(len(slots), size, dtype=np.uint32)
    tb = to_device(buf, off, ln)
    out, st = (eng.digest_fcs_device if flags else eng.digest_device)(*tb)
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any()
    crc, ipc, l4c = split_digests(out.cpu().numpy())
    want = e["synack_out"][slots]
    assert np.array_equal(crc, want["crc32"]) and np.array_equal(ipc, want["ip_csum"]) and np.array_equal(l4c, want["l4_csum"])


def test_mtu_53(eng):
    # a SYN has at least the SYN-ACK's 54 bytes: at an mtu of 53 no frame of the batch is accepted, so no
    # flow is a candidate and no slot is filled; at 54 the SYNs without options and their SYN-ACKs pass
    e = check(eng, cases.three_listeners(), mtu=53, seed=4)
    assert not e["n_accepted"] and not filled(e) and not e["listeners_out"]["n_syn"].any()
    e = check(eng, cases.three_listeners(), mtu=54, seed=5)
    assert not e["synack_status"].any() and len(filled(e)) == 13


# ---- the result does not depend on the hash, the grid or the digest kernel ----------------------------

def test_hash_masks_and_one_workgroup(eng):
    from seqs_amd import Engine
    from seqs_amd.framesum import TEST_LIB_PATH

    three, lanes = cases.three_listeners(), cases.lanes()
    e3, el = check(eng, three), check(eng, lanes)
    te = Engine(0, lib_path=TEST_LIB_PATH)
    try:
        for mask in (0, 0xF):
            assert te.lib.fs_test_set_flow_hash_mask(te._ctx, mask) == 0
            check(te, three, e=e3)
            check(te, lanes, e=el)
        te.set_workgroups(1)
        check(te, three, e=e3)
        check(te, lanes, e=el)
    finally:
        te.close()


@pytest.mark.parametrize("variant", engines.VARIANTS, ids=engines.IDS)
def test_every_engine(variant):
    import torch

    assert torch.cuda.is_available()
    e2 = engines.engine_for(variant)
    try:
        check(e2, cases.lanes(8), parity=True)
    finally:
        e2.close()


# ---- scale -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", cases.BIG_SHAPES)
def test_65793_syn_flows(eng, shape):
    case = cases.big(shape)
    e = check(eng, case, payload=False, seed=len(shape))
    assert int(e["listeners_out"]["n_full"].sum()) == case.info["n_full"]
    assert int((e["accept_of"] == ref.FULL).sum()) == case.info["n_full"]
    assert int(e["conns"]["used"].sum()) == cases.BIG - case.info["n_full"]


# ---- degenerate calls ------------------------------------------------------------------------------

def test_empty_calls(eng):
    import torch

    from seqs_amd import split_accept

    case = cases.lanes()
    none_l, none_s = ref.listeners_of(), ref.slots_of()
    # no listeners: the receive call, zeroed conns, accept_of all NONE; slots without listeners stay free
    for slots in (none_s, case.slots):
        c0 = cases.ACase(case.frames, none_l, slots)
        e = check(eng, c0, parity=True)
        assert (e["accept_of"] == ref.NONE).all() and not e["conns"]["used"].any()
    # listeners without slots: every candidate FULL
    c1 = cases.ACase(case.frames, ref.listeners_of((cases.local(80), cases.MAC, 0, 0)), none_s)
    e = check(eng, c1)
    assert int((e["accept_of"] == ref.FULL).sum()) == 9
    # n == 0: zeroed conns and listeners_out
    buf, off, ln = fref.pack(case.frames)
    tb, to, tl = to_device(buf, off, ln)
    rings = torch.zeros(64, dtype=torch.uint8, device=tb.device)
    res = eng.accept_flows_device(tb, to[:0], tl[:0], case.socks, case.snd, rings, case.listeners, case.slots)
    torch.cuda.synchronize()
    conns, lout, of = split_accept(*res[:3])
    assert not conns.view(np.uint8).any() and not lout.view(np.uint8).any() and of.size == 0
    assert not res[3].cpu().numpy().any()
    # each nullable array left out
    check(eng, case, accept_of=False)
    check(eng, case, synack_results=False)


def test_8_calls_in_flight(eng):
    import torch

    dev = torch.device("cuda:0")
    built = [cases.lanes(9), cases.three_listeners(), cases.grid(), cases.lanes(1), cases.geometries(), cases.near_misses(),
             cases.lanes(0), cases.three_listeners()]
    prepared = []
    for j, case in enumerate(built):
        buf, off, ln = fref.pack(case.frames, lead=j % 4, seed=j)
        noise = np.random.default_rng(j).integers(0, 256, 3 + TAIL, dtype=np.uint8)
        rings = sentinel(case.rings_bytes, j)
        syn0, out0, st0 = prefill(len(case.slots), j)
        e = ref.expected(buf, off, ln, 0, 0, noise, 3, 0, case.socks, case.snd, rings, case.listeners, case.slots, j % 2 * 2, syn0)
        prepared.append((e, to_device(buf, off, ln), case, torch.from_numpy(rings).to(dev), torch.from_numpy(syn0).to(dev),
                         torch.from_numpy(out0).to(dev), torch.from_numpy(st0).to(dev), out0, st0, int(ln.size)))
    torch.cuda.synchronize()
    res = [eng.accept_flows_device(*tb, case.socks, case.snd, rt, case.listeners, case.slots, synack_flags=j % 2 * 2,
                                   payload=False, synacks=st, synack_results=(ot, stt))
           for j, (_, tb, case, rt, st, ot, stt, _, _, _) in enumerate(prepared)]
    torch.cuda.synchronize()
    for (e, _, _, rt, _, _, _, out0, st0, n), r in zip(prepared, res):
        compare_accept(e, r, out0, st0, n)
        compare_recv(e, r[6], r[7])
        compare_delivery(e, r[8], r[9], rt)


# ---- the host form ---------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["three listeners", "near misses"])
def test_host_form_equals_the_device_form(eng, which):
    case = cases.three_listeners() if which == "three listeners" else cases.near_misses()
    buf, off, ln = fref.pack(case.frames, lead=9)
    e = check(eng, case, batch=(buf, off, ln), synack_flags=ref.FCS_APPEND, seed=8)
    syn0, out0, st0 = prefill(len(case.slots), 8)
    from seqs_amd.framesum import DIGEST_DTYPE

    rings, mine = sentinel(case.rings_bytes, 8), syn0.copy()
    out_h, st_h = np.ascontiguousarray(out0).view(DIGEST_DTYPE).reshape(-1).copy(), st0.copy()
    res = eng.accept_flows_host(buf, off, ln, case.socks, case.snd, rings, case.listeners, case.slots,
                                synack_flags=ref.FCS_APPEND, payload=False, synacks=mine, synack_results=(out_h, st_h))
    conns, lout, of, synacks, syn_out, syn_st, sn, code, so = res[:9]
    assert conns.tobytes() == e["conns"].tobytes() and lout.tobytes() == e["listeners_out"].tobytes()
    assert np.array_equal(of, e["accept_of"]) and np.array_equal(synacks, e["synacks"]) and synacks is mine
    want_out, want_st = want_results(e, out0, st0)
    assert np.array_equal(syn_out.view(np.uint8).reshape(-1, 8), want_out) and np.array_equal(syn_st, want_st)
    assert sn.tobytes() == e["snd_out"].tobytes() and np.array_equal(code, e["code"]) and so.tobytes() == e["socks_out"].tobytes()
    assert np.array_equal(rings, e["rings"])
    # n of 0 on the host, and the nullable arrays left out
    res = eng.accept_flows_host(buf, off[:0], ln[:0], case.socks, case.snd, rings, case.listeners, case.slots, payload=False)
    assert not res[0].view(np.uint8).any() and not res[1].view(np.uint8).any()
    res = eng.accept_flows_host(buf, off, ln, case.socks, case.snd, sentinel(case.rings_bytes, 8), case.listeners, case.slots,
                                synack_flags=ref.FCS_APPEND, payload=False, accept_of=False, synack_results=False)
    assert res[2] is None and res[4] is None and res[0].tobytes() == e["conns"].tobytes()
    assert np.array_equal(res[3][: len(case.slots) * 64].reshape(-1, 64)[:, :58][e["conns"]["used"] == 1],
                          e["synacks"][: len(case.slots) * 64].reshape(-1, 64)[:, :58][e["conns"]["used"] == 1])


# ---- rejected calls --------------------------------------------------------------------------------

def test_rejected_calls_leave_the_device_alone(eng):
    import torch

    from seqs_amd import FramesumError

    case = cases.lanes()
    tb, to, tl = to_device(*fref.pack(case.frames))
    rings = torch.zeros(64, dtype=torch.uint8, device=tb.device)
    synacks = torch.zeros(len(case.slots) * 64, dtype=torch.uint8, device=tb.device)
    bad = case.listeners.copy()
    bad["n_slots"] = 10
    with pytest.raises(FramesumError, match="slot range ends past n_slots"):
        eng.accept_flows_device(tb, to, tl, case.socks, case.snd, rings, bad, case.slots, synacks=synacks)
    with pytest.raises(FramesumError, match="synack_flags"):
        eng.accept_flows_device(tb, to, tl, case.socks, case.snd, rings, case.listeners, case.slots, synack_flags=1, synacks=synacks)
    twice = ref.listeners_of((cases.local(80), cases.MAC, 0, 4), (cases.local(80), cases.MAC, 4, 5))
    with pytest.raises(FramesumError, match="fs_accept_flows_batch: listener or slot 1: its local equals an earlier listener's"):
        eng.accept_flows_device(tb, to, tl, case.socks, case.snd, rings, twice, case.slots, synacks=synacks)
    over = ref.listeners_of((cases.local(80), cases.MAC, 0, 5), (cases.local(81), cases.MAC, 4, 5))
    with pytest.raises(FramesumError, match="listener or slot 1: its slot range overlaps another listener's"):
        eng.accept_flows_device(tb, to, tl, case.socks, case.snd, rings, over, case.slots, synacks=synacks)
    # what the receive call rejects, the accept call rejects under its own name, in both forms: the send
    # side's checks, the delivery's checks of the sockets, the flags
    near = cases.near_misses()
    nb = fref.pack(near.frames)
    ntb = to_device(*nb)
    nrings = torch.zeros(near.rings_bytes, dtype=torch.uint8, device=tb.device)
    nsyn = torch.zeros(len(near.slots) * 64, dtype=torch.uint8, device=tb.device)
    snd_nxt = int(near.socks["snd_nxt"][0])
    two = np.concatenate([near.socks, near.socks])
    two["key"][1][12] ^= 1
    cases_bad = ((near.socks, recv_ref.snd_of((snd_nxt - 5, 65536)), 0, "fs_accept_flows_batch{}: socket 0: snd_wnd above 65,535"),
                 (near.socks, recv_ref.snd_of((snd_nxt + 1, 10)), 0, "fs_accept_flows_batch{}: socket 0: snd_una is ahead of snd_nxt"),
                 (two, recv_ref.snd_of((0x7000, 500), (0x7000, 500)), 0, "fs_accept_flows_batch{}: socket 1: its ring overlaps another socket's"),
                 (near.socks, near.snd, 2, "fs_accept_flows_batch{}: flags must be 0 or FS_RX_FCS"))
    for socks, snd, flags, text in cases_bad:
        with pytest.raises(FramesumError, match=text.format("")):
            eng.accept_flows_device(*ntb, socks, snd, nrings, near.listeners, near.slots, flags=flags, synacks=nsyn)
        with pytest.raises(FramesumError, match=text.format("_host")):
            eng.accept_flows_host(*nb, socks, snd, np.zeros(near.rings_bytes, dtype=np.uint8), near.listeners, near.slots, flags=flags)
    torch.cuda.synchronize()
    assert not bool(synacks.any()) and not bool(nsyn.any()) and not bool(nrings.any())
    # null conns with slots, through the C ABI
    lib, vp = eng.lib, ctypes.c_void_p
    some, l1, s1 = vp(tb.data_ptr()), vp(case.listeners.ctypes.data), vp(case.slots.ctypes.data)
    assert lib.fs_accept_flows_batch(eng._ctx, some, some, some, 1, 0, 0, None, 0, None, 0, None, None, None, None, None, l1, 1,
                                     s1, 9, 0, None, some, None, some, None, None, None, 0, some, some, some, None, some, None,
                                     None, None) == -1
    assert b"null listeners" in lib.fs_last_error(eng._ctx)
