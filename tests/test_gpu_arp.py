"""The ARP call on the GPU (fs_arp_flows_batch / fs_arp_flows_batch_host) against tests/arp_ref.py, whole arrays
over sentinel prefills: hosts_out, queries_out, every byte of arp_frames, arp_out, arp_status, arp_code and arp_of;
and every output of the UDP call against fs_udp_flows_batch of the same library on the same arguments. The
verdicts the reference takes are the CPU oracle's. The batches are tests/arp_cases.py's, which
tests/test_arp_case_builders.py shows to reach what they name."""
import re

import numpy as np
import pytest

import arp_cases as cases
import arp_ref as ref
import engines
import flows_ref as fref
from test_gpu_close import SentinelEmpty
from test_gpu_deliver import to_device
from test_gpu_udp import Lists, oracle_status

pytestmark = pytest.mark.gpu
NAMES = ("hosts_out", "queries_out", "arp_frames", "arp_out", "arp_status", "arp_code", "arp_of")
NO_PORTS = (np.zeros(0, dtype=np.dtype([("local", "u1", (6,)), ("reserved", "u1", (2,)), ("n_cells", "<u4"), ("cell_size", "<u4"),
                                        ("cells_off", "<u8"), ("wcell", "<u4"), ("free", "<u4")])), 8)


@pytest.fixture(scope="module")
def eng():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()
    e = Engine(0)
    yield e
    e.close()


def prefill(slots, seed):
    rng = np.random.default_rng(60 + seed)
    return (rng.integers(1, 256, slots * 64 + 24, dtype=np.uint8), rng.integers(1, 256, slots * 8, dtype=np.uint8).view(ref.DIGEST_DTYPE),
            rng.integers(1, 256, slots, dtype=np.uint8))


def differences(got, want, asked=(True, True, True)):
    """The arrays of a call's first seven results that differ from the reference's, as text."""
    bad = []
    views = (ref.HOST_OUT_DTYPE, ref.QUERY_OUT_DTYPE, np.uint8, ref.DIGEST_DTYPE, np.uint8, np.uint8, np.uint32)
    want_results, want_code, want_of = asked
    there = (True, True, True, want_results, want_results, want_code, want_of)
    for name, g, w, view, has in zip(NAMES, got, want, views, there):
        if not has:
            if g is not None:
                bad.append(f"{name} is not None")
            continue
        g = np.ascontiguousarray(g.cpu().numpy() if hasattr(g, "cpu") else g).reshape(-1).view(np.uint8)
        w = np.ascontiguousarray(w).reshape(-1).view(np.uint8)
        if g.size != w.size:
            bad.append(f"{name}: {g.size} bytes for {w.size}")
            continue
        at = np.flatnonzero(g != w)
        if at.size:
            k = int(at[0]) // np.dtype(view).itemsize
            bad.append(f"{name}: {at.size} bytes differ, first in entry {k}: {g.view(view)[k : k + 2]} for {w.view(view)[k : k + 2]}")
    return bad


def check(eng, case, lead=1, seed=0, parity=True, results=True, arp_code=True, arp_of=True):
    """One fs_arp_flows_batch of the case over sentinel-filled result tensors; everything it adds compared with the
    reference, and with `parity` every UDP-call output with fs_udp_flows_batch's on the same arguments. Returns
    (the expected tuple, the call's tuple)."""
    import torch

    from seqs_amd.framesum import FLOW_TOTALS_DTYPE

    frames = case.frames
    lists = Lists(case.lists) if case.lists is not None else Lists()
    batch = case.batch
    if batch is None and len(frames) == 0:
        batch = (np.zeros(64, dtype=np.uint8), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    buf, off, ln = fref.pack(frames, lead=lead) if batch is None else batch
    fcs = bool(case.flags & 1)
    status = case.status
    if status is None:
        status = oracle_status(buf, off, ln, case.mtu, fcs) if len(frames) else np.zeros(0, dtype=np.uint8)
    slots = case.n_reply_slots + len(case.queries)
    frames0, out0, st0 = prefill(slots, seed)
    want = ref.expected(frames, status, case.hosts, case.queries, case.n_reply_slots, case.arp_flags, frames0, out0, st0, mtu=case.mtu,
                        fcs=fcs)
    case.reaches(ref.expected(frames, status, case.hosts, case.queries, case.n_reply_slots, case.arp_flags, mtu=case.mtu, fcs=fcs))
    dev = torch.device("cuda:0")
    tb = to_device(buf, off, ln)
    ports, cells_bytes = case.ports if case.ports is not None else NO_PORTS
    rings0 = np.random.default_rng(41 + seed).integers(0, 256, lists.rings_bytes, dtype=np.uint8)
    cells0 = np.random.default_rng(42 + seed).integers(1, 256, cells_bytes, dtype=np.uint8)
    room = int(ln.sum())

    def run(call, **more):
        rt, ct = torch.from_numpy(rings0).to(dev), torch.from_numpy(cells0).to(dev)
        pt = torch.zeros(room + 8, dtype=torch.uint8, device=dev)
        with SentinelEmpty(seed):
            res = call(*tb, lists.socks, lists.snd, rt, lists.listeners, lists.slots, lists.closers, lists.openers, ports, ct,
                       mtu=case.mtu, flags=case.flags, payload=pt[:room], **more)
        torch.cuda.synchronize()
        return res, pt, rt, ct

    ft = torch.from_numpy(frames0).to(dev)
    pair = (torch.from_numpy(out0.view(np.int32).reshape(-1, 2).copy()).to(dev), torch.from_numpy(st0).to(dev)) if results else False
    res, pt, rt, ct = run(eng.arp_flows_device, hosts=case.hosts, queries=case.queries, n_reply_slots=case.n_reply_slots,
                          arp_flags=case.arp_flags, arp_frames=ft[: slots * 64], arp_results=pair, arp_code=arp_code, arp_of=arp_of)
    got = (res[0], res[1], ft, res[3], res[4], res[5], res[6])
    bad = differences(got, want, (results, arp_code, arp_of))
    assert not bad, "\n".join(bad)
    if parity:
        r, pt2, rt2, ct2 = run(eng.udp_flows_device)
        mine = res[7:]
        assert len(mine) == len(r) == 28
        assert torch.equal(rt, rt2) and torch.equal(pt, pt2) and torch.equal(ct, ct2)
        t = mine[25].cpu().numpy().view(FLOW_TOTALS_DTYPE)[0]
        cuts = {20: 0, 21: int(t["n_runs"]), 22: int(t["n_flows"]), 23: int(t["n_accepted"])}  # payload: compared above
        for k, (x, y) in enumerate(zip(mine, r)):
            cut = cuts.get(k)
            assert (x is None and y is None) or torch.equal(x[:cut], y[:cut]), f"UDP-call output {k} differs"
    return want, res


# ---- requests ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("free", [0, 1, 63, 64, 65, 300])
def test_rank_and_admission(eng, free):
    check(eng, cases.rank(free), seed=free)


def test_three_hosts_interleave(eng):
    check(eng, cases.three_hosts())


def test_two_hosts_sharing_a_mac(eng):
    check(eng, cases.shared_mac())


# ---- replies ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pos", [0, 63, 64, 257])
def test_the_lowest_reply_resolves_the_query(eng, pos):
    check(eng, cases.replies(pos), seed=pos)


def test_a_flagged_query_stays_unanswered_and_near_senders_are_ignored(eng):
    check(eng, cases.flagged_and_near())


# ---- frames -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lead", range(64))
def test_frame_lengths_at_every_alignment_and_every_flag(eng, lead):
    check(eng, cases.lengths(lead % 4), lead=lead, seed=lead, parity=lead < 4)


@pytest.mark.parametrize("arp_flags", range(4))
def test_built_frames_digest_as_arp_and_feed_a_second_call(eng, arp_flags):
    """The built frames through fs_digest_batch (with their FCS: fs_digest_batch_fcs), whose digests and verdicts
    are the call's own arp_out and arp_status; then as the input of a second call on the other side of the wire."""
    import torch

    case = cases.lengths(arp_flags)
    want, res = check(eng, case, seed=arp_flags, parity=False)
    slots = [0, 1, 2, 6]
    size = (60 if arp_flags & ref.PAD else 42) + (4 if arp_flags & ref.FCS_APPEND else 0)
    dev = torch.device("cuda:0")
    off = torch.tensor([64 * s for s in slots], dtype=torch.int64, device=dev)
    ln = torch.full((4,), size, dtype=torch.int32, device=dev)
    built = res[2].contiguous()
    out, st = (eng.digest_fcs_device if arp_flags & ref.FCS_APPEND else eng.digest_device)(built, off, ln)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [ref.FS_ARP] * 4 == res[4].cpu()[slots].tolist()
    assert torch.equal(out.cpu(), res[3].cpu()[slots])
    # the other side: the three senders' hosts hear their replies, the asked address answers the request
    wire = [bytes(built.cpu().numpy()[64 * s : 64 * s + size]) for s in slots]
    rows = [ref.host_row(cases.source(k), cases.source_mac(k), free=1) for k in range(3)] + [ref.host_row("10.0.1.99", "02:00:00:00:01:63", free=1)]
    hosts, n_reply = ref.hosts_of(rows)
    queries = ref.queries_of([ref.query_row(k, cases.US) for k in range(3)])

    def reaches(w):
        assert list(w[5]) == [ref.RESOLVED] * 3 + [ref.ANSWERED] and [bytes(m) for m in w[1]["mac"]] == [ref.mac6(cases.US_MAC)] * 3
        assert bytes(w[2][3 * 64 : 3 * 64 + 6]) == ref.mac6(cases.US_MAC)
    check(eng, cases.Case(wire, hosts, queries, n_reply, reaches, flags=1 if arp_flags & ref.FCS_APPEND else 0), parity=False)


def test_frames_with_their_fcs(eng):
    check(eng, cases.with_fcs())


def test_keys_one_bit_away(eng):
    check(eng, cases.near_keys())


def test_an_mtu_below_the_padded_frame_refuses_it(eng):
    case = cases.lengths(ref.PAD)
    case.mtu = 59
    case.reaches = lambda w: None  # (the 60-byte and 1,500-byte inputs exceed it too)
    want, _ = check(eng, case, parity=False)
    assert list(want[5]) == [ref.ANSWERED, ref.RESOLVED, 0, 0, 0, 0] and want[4][0] == 2 and want[3][0]["ip_csum"] == 0 and want[4][6] == 2


# ---- launch shapes ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask", [0, 0xF, 0xFFFFFFFF])
def test_hash_masks(mask):
    """The result does not depend on the hash: 300 hosts and 300 queries under a hash cut to nothing, to 4 bits, and whole."""
    from seqs_amd import Engine
    from seqs_amd.framesum import TEST_LIB_PATH

    te = Engine(0, lib_path=TEST_LIB_PATH)
    try:
        assert te.lib.fs_test_set_flow_hash_mask(te._ctx, mask) == 0
        check(te, cases.table_load(), parity=mask == 0xF)
    finally:
        te.close()


def test_one_workgroup_grid():
    from seqs_amd import Engine

    e = Engine(0)
    try:
        e.set_workgroups(1)
        check(e, cases.two_hosts())
    finally:
        e.close()


@pytest.mark.parametrize("variant", engines.VARIANTS, ids=engines.IDS)
def test_every_engine_column(variant):
    e = engines.engine_for(variant)
    try:
        check(e, cases.columns(), parity=False)
    finally:
        e.close()


# ---- mixed and large batches --------------------------------------------------------------------------------------

def test_hosts_and_queries_beside_sockets_listeners_closers_openers_and_ports(eng):
    check(eng, cases.mixed())


@pytest.mark.parametrize("n_hosts", [1, 1000, 65536])
def test_large_batches(eng, n_hosts):
    check(eng, cases.big(n_hosts), parity=n_hosts == 1000)


# ---- calls --------------------------------------------------------------------------------------------------------

def test_empty_calls(eng):
    check(eng, cases.empty_batch())  # n == 0: the input state, and the flagged query's request
    check(eng, cases.no_hosts())     # n_hosts == 0: the codes alone
    check(eng, cases.Case([], cases.NO_HOSTS, cases.NO_QUERIES, 0, lambda w: None))


def test_each_nullable_array_left_out(eng):
    case = cases.replies(64)
    for results, code, of in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        check(eng, case, results=results, arp_code=code, arp_of=of, parity=False)
    check(eng, cases.no_hosts(), arp_code=False, parity=False)
    check(eng, cases.no_hosts(), arp_of=False, parity=False)
    check(eng, cases.no_hosts(), arp_code=False, arp_of=False, parity=False)


def test_eight_calls_in_flight(eng):
    import torch

    dev = torch.device("cuda:0")
    lists = Lists()
    calls = []
    for k in range(8):
        case = cases.in_flight(k)
        buf, off, ln = fref.pack(case.frames, lead=k)
        frames0 = np.full(64 * (case.n_reply_slots + 1), 0xA0 + k, dtype=np.uint8)
        calls.append((case, frames0, (buf, off, ln), torch.from_numpy(frames0).to(dev), to_device(buf, off, ln),
                      torch.zeros(8, dtype=torch.uint8, device=dev), torch.zeros(8, dtype=torch.uint8, device=dev)))
    results = [eng.arp_flows_device(*tb, lists.socks, lists.snd, rt, lists.listeners, lists.slots, lists.closers, lists.openers,
                                    NO_PORTS[0], ct, case.hosts, case.queries, arp_flags=case.arp_flags, arp_frames=ft)
               for case, frames0, batch, ft, tb, rt, ct in calls]
    torch.cuda.synchronize()
    for (case, frames0, batch, ft, tb, rt, ct), res in zip(calls, results):
        want = ref.expected(case.frames, oracle_status(*batch), case.hosts, case.queries, case.n_reply_slots, case.arp_flags, frames0)
        case.reaches(want)
        bad = differences((res[0], res[1], ft, res[3], res[4], res[5], res[6]), want)
        assert not bad, "\n".join(bad)


def test_host_form(eng):
    lists = Lists()
    case = cases.host_form()
    buf, off, ln = fref.pack(case.frames, lead=3)
    slots = case.n_reply_slots + len(case.queries)
    frames0, out0, st0 = prefill(slots, 9)
    status = oracle_status(buf, off, ln)
    want = ref.expected(case.frames, status, case.hosts, case.queries, case.n_reply_slots, case.arp_flags, frames0, out0, st0)
    case.reaches(want)

    def call(b, o, l, arp_frames, **kw):
        return eng.arp_flows_host(b, o, l, lists.socks, lists.snd, np.zeros(8, dtype=np.uint8), lists.listeners, lists.slots, lists.closers,
                                  lists.openers, NO_PORTS[0], np.zeros(8, dtype=np.uint8), case.hosts, case.queries,
                                  n_reply_slots=case.n_reply_slots, arp_flags=case.arp_flags, arp_frames=arp_frames, **kw)

    mine = frames0.copy()
    res = call(buf, off, ln, mine[: slots * 64], arp_results=(out0.copy(), st0.copy()))
    bad = differences((res[0], res[1], mine, res[3], res[4], res[5], res[6]), want)
    assert not bad, "\n".join(bad)
    other = eng.udp_flows_host(buf, off, ln, lists.socks, lists.snd, np.zeros(8, dtype=np.uint8), lists.listeners, lists.slots,
                               lists.closers, lists.openers, NO_PORTS[0], np.zeros(8, dtype=np.uint8))
    for k, (x, y) in enumerate(zip(res[7:], other)):
        assert (x is None and y is None) or np.asarray(x).tobytes() == np.asarray(y).tobytes(), f"UDP-call output {k} differs"
    # each nullable array left out
    for results, code, of in ((False, True, True), (True, False, True), (True, True, False)):
        mine = frames0.copy()
        res = call(buf, off, ln, mine[: slots * 64], arp_results=(out0.copy(), st0.copy()) if results else False, arp_code=code, arp_of=of)
        bad = differences((res[0], res[1], mine, res[3], res[4], res[5], res[6]), want, (results, code, of))
        assert not bad, "\n".join(bad)
    # the empty host call: the state comes back as it went in, and the flagged query's request is built
    want = ref.expected([], [], case.hosts, case.queries, case.n_reply_slots, case.arp_flags, frames0, out0, st0)
    mine = frames0.copy()
    res = call(buf[:0], off[:0], ln[:0], mine[: slots * 64], arp_results=(out0.copy(), st0.copy()))
    bad = differences((res[0], res[1], mine, res[3], res[4], res[5], res[6]), want)
    assert not bad, "\n".join(bad)
    assert res[1]["state"].tolist() == [ref.Q_WAIT, ref.Q_SENT] and mine[64 * 41 : 64 * 41 + 6].tolist() == [255] * 6


@pytest.mark.parametrize("which", range(len(cases.REJECTIONS)))
def test_every_rejection_with_its_text(eng, which):
    import torch

    from seqs_amd import FramesumError

    lists = Lists()
    hosts, queries, n_reply = cases.rejected_lists()
    change, text = cases.REJECTIONS[which]
    change(hosts, queries)
    buf, off, ln = fref.pack(list(cases.noisy()[:4]))
    dev = torch.device("cuda:0")
    ft = torch.full((64 * (n_reply + 3),), 0x5A, dtype=torch.uint8, device=dev)
    rt, ct = torch.zeros(8, dtype=torch.uint8, device=dev), torch.zeros(8, dtype=torch.uint8, device=dev)
    for host in (False, True):
        with pytest.raises(FramesumError, match=re.escape(text)):
            if host:
                eng.arp_flows_host(buf, off, ln, lists.socks, lists.snd, np.zeros(8, dtype=np.uint8), lists.listeners, lists.slots,
                                   lists.closers, lists.openers, NO_PORTS[0], np.zeros(8, dtype=np.uint8), hosts, queries,
                                   n_reply_slots=n_reply)
            else:
                eng.arp_flows_device(*to_device(buf, off, ln), lists.socks, lists.snd, rt, lists.listeners, lists.slots, lists.closers,
                                     lists.openers, NO_PORTS[0], ct, hosts, queries, n_reply_slots=n_reply, arp_frames=ft)
    torch.cuda.synchronize()
    assert bool((ft == 0x5A).all())  # checked on the host before any device work


def test_null_arrays_counts_and_flags_are_rejected(eng):
    import ctypes

    lib, ctx = eng.lib, eng._ctx
    none = ctypes.c_void_p()
    some = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(4096)))
    head = (ctx, none, none, none, 0, 0, 0, none, 0, none, 0, none, none, none, none, none)
    listen = (none, 0, none, 0, 0, none, none, none, none, none, none)
    closing = (none, 0, none, none, none)
    opening = (none, 0, 0, none, none, none, none)
    udp = (none, 0, none, 0, none, none, none)
    tail = (none, 0, none, none, none, none, some, none, none, none)
    hrow, qrow = ref.host_row(cases.US, cases.US_MAC), ref.query_row(0, cases.PEER)
    hp, qp = ctypes.c_void_p(hrow.ctypes.data), ctypes.c_void_p(qrow.ctypes.data)
    rest = (none, none, none, none)
    for arp, text in (((none, 1, none, 0, 1, 0, some, none, some), "host or query 0: null hosts, hosts_out or arp_frames"),
                      ((hp, 1, none, 0, 1, 0, none, none, some), "host or query 0: null hosts, hosts_out or arp_frames"),
                      ((hp, 1, none, 0, 1, 0, some, none, none), "host or query 0: null hosts, hosts_out or arp_frames"),
                      ((hp, 1, none, 1, 1, 0, some, some, some), "host or query 0: null queries, queries_out or arp_frames"),
                      ((hp, 1, qp, 1, 1, 0, some, none, some), "host or query 0: null queries, queries_out or arp_frames"),
                      ((hp, 65537, none, 0, 1, 0, some, none, some), "host or query 0: n_hosts above 65,536"),
                      ((hp, 1, qp, 65537, 1, 0, some, some, some), "host or query 0: n_queries above 65,536"),
                      ((hp, 1, qp, 1, 65537, 0, some, some, some), "host or query 0: n_reply_slots above 65,536"),
                      ((hp, 1, qp, 1, 1, 4, some, some, some), "host or query 0: arp_flags must lie in FS_ARP_PAD | FS_FCS_APPEND"),
                      ((none, 0, qp, 1, 0, 0, none, some, some), "host or query 0: its host is not below n_hosts")):
        assert lib.fs_arp_flows_batch(*head, *listen, *closing, *opening, *udp, *arp, *rest, *tail) == -1
        assert lib.fs_last_error(ctx).decode() == "fs_arp_flows_batch: " + text
    # what the UDP call rejects, this call rejects with its own name
    good = (none, 0, none, 0, 0, 0, none, none, none)
    bad_flags = head[:6] + (2,) + head[7:]
    assert lib.fs_arp_flows_batch(*bad_flags, *listen, *closing, *opening, *udp, *good, *rest, *tail) == -1
    assert lib.fs_last_error(ctx).decode() == "fs_arp_flows_batch: flags must be 0 or FS_RX_FCS"
    bad_port = (some, 65537, some, 4096, some, none, none)
    assert lib.fs_arp_flows_batch(*head, *listen, *closing, *opening, *bad_port, *good, *rest, *tail) == -1
    assert lib.fs_last_error(ctx).decode() == "fs_arp_flows_batch: port 0: n_ports above 65,536"
