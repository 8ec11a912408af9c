"""The UDP call on the GPU (fs_udp_flows_batch / fs_udp_flows_batch_host) against tests/udp_ref.py, whole arrays
over sentinel prefills: ports_out, port_of, cell_of and every byte of `cells`; and every output of the connect
call against fs_connect_flows_batch of the same library on the same arguments. The verdicts the reference
takes are the CPU oracle's. The batches are tests/udp_cases.py's, which tests/test_udp_case_builders.py shows to
reach what they name."""
import re

import numpy as np
import pytest

import engines
import flows_ref as fref
import udp_cases as cases
import udp_ref as ref
from test_gpu_close import SentinelEmpty
from test_gpu_deliver import to_device

pytestmark = pytest.mark.gpu
CELL_TAIL = 24  # bytes of `cells` behind cells_bytes, which no call may touch


@pytest.fixture(scope="module")
def eng():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()
    e = Engine(0)
    yield e
    e.close()


class Lists:
    """The connect call's lists; empty unless a connect case supplies them."""

    def __init__(self, case=None):
        from seqs_amd.framesum import (ACCEPT_SLOT_DTYPE, CLOSER_DTYPE, LISTENER_DTYPE, OPENER_DTYPE, SND_DTYPE, SOCK_DTYPE)

        def of(name, dtype):
            return np.zeros(0, dtype=dtype) if case is None else np.ascontiguousarray(getattr(case, name), dtype=dtype)

        self.socks, self.snd = of("socks", SOCK_DTYPE), of("snd", SND_DTYPE)
        self.listeners, self.slots = of("listeners", LISTENER_DTYPE), of("slots", ACCEPT_SLOT_DTYPE)
        self.closers, self.openers = of("closers", CLOSER_DTYPE), of("openers", OPENER_DTYPE)
        self.rings_bytes = 8 if case is None else max(8, int(case.rings_bytes))


def oracle_status(buf, off, ln, mtu=0, fcs=False):
    from oracle import coracle

    return (coracle.digest_fcs_batch if fcs else coracle.digest_batch)(buf, off, ln, mtu)[1]


def check(eng, frames, ports, cells_bytes, lists=None, mtu=0, flags=0, lead=1, seed=0, port_of=True, cell_of=True, parity=True,
          batch=None):
    """One fs_udp_flows_batch of `frames` over sentinel-filled result tensors and a sentinel-filled `cells`;
    everything it adds compared with the reference, and with `parity` every connect-call output with
    fs_connect_flows_batch's on the same arguments. Returns the expected tuple."""
    import torch

    from seqs_amd.framesum import FLOW_TOTALS_DTYPE, UDP_PORT_OUT_DTYPE

    lists = lists or Lists()
    if batch is None and len(frames) == 0:
        batch = (np.zeros(64, dtype=np.uint8), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    buf, off, ln = fref.pack(frames, lead=lead) if batch is None else batch
    fcs = bool(flags & 1)
    cells0 = np.random.default_rng(40 + seed).integers(1, 256, cells_bytes + CELL_TAIL, dtype=np.uint8)
    status = oracle_status(buf, off, ln, mtu, fcs) if len(frames) else np.zeros(0, dtype=np.uint8)
    want = ref.expected(frames, status, ports, cells0, fcs)
    dev = torch.device("cuda:0")
    tb = to_device(buf, off, ln)
    rings0 = np.random.default_rng(41 + seed).integers(0, 256, lists.rings_bytes, dtype=np.uint8)
    room = int(ln.sum())

    def run(call, **more):
        rt = torch.from_numpy(rings0).to(dev)
        pt = torch.zeros(room + 8, dtype=torch.uint8, device=dev)
        with SentinelEmpty(seed):
            res = call(*tb, lists.socks, lists.snd, rt, lists.listeners, lists.slots, lists.closers, lists.openers, mtu=mtu,
                       flags=flags, payload=pt[:room], **more)
        torch.cuda.synchronize()
        return res, pt, rt

    ct = torch.from_numpy(cells0).to(dev)
    res, pt, rt = run(lambda *a, **k: eng.udp_flows_device(*a, ports, ct[:cells_bytes], port_of=port_of, cell_of=cell_of, **k))
    got_out = res[0].cpu().numpy().reshape(-1).view(UDP_PORT_OUT_DTYPE)
    bad = np.flatnonzero((got_out.view(np.uint8).reshape(-1, 32) != want[0].view(np.uint8).reshape(-1, 32)).any(axis=1))
    assert bad.size == 0, f"{bad.size} ports_out differ, first at {bad[:4]}: {got_out[bad[:2]]} for {want[0][bad[:2]]}"
    for name, t, w, asked in (("port_of", res[1], want[1], port_of), ("cell_of", res[2], want[2], cell_of)):
        assert (t is None) == (not asked)
        if asked:
            g = t.cpu().numpy().view(np.uint32)
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, f"{bad.size} {name} differ, first at {bad[:4]}: {g[bad[:4]]} for {w[bad[:4]]}"
    g = ct.cpu().numpy()
    bad = np.flatnonzero(g != want[3])
    assert bad.size == 0, f"{bad.size} cell bytes differ, first at {bad[:8]}"
    if parity:
        r, pt2, rt2 = run(eng.connect_flows_device)
        mine = res[3:]
        assert len(mine) == len(r) == 25
        assert torch.equal(rt, rt2) and torch.equal(pt, pt2)
        t = mine[22].cpu().numpy().view(FLOW_TOTALS_DTYPE)[0]
        cuts = {17: 0, 18: int(t["n_runs"]), 19: int(t["n_flows"]), 20: int(t["n_accepted"])}  # payload: compared above
        for k, (x, y) in enumerate(zip(mine, r)):
            cut = cuts.get(k)
            assert (x is None and y is None) or torch.equal(x[:cut], y[:cut]), f"connect-call output {k} differs"
    return want


def check_case(eng, case, **kw):
    """check() of one of tests/udp_cases.py's batches; what the batch reaches is asserted on the reference's tuple."""
    want = check(eng, case.frames, case.ports, case.cells_bytes, lists=Lists(case.lists) if case.lists is not None else None,
                 mtu=case.mtu, flags=case.flags, batch=case.batch, **kw)
    case.reaches(want)
    return want


# ---- rank -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("free", [0, 1, 63, 64, 65, 300])
def test_rank_and_admission(eng, free):
    check_case(eng, cases.rank(free), seed=free)


@pytest.mark.parametrize("n_cells", [1, 5])
def test_wrap_from_the_last_cell(eng, n_cells):
    check_case(eng, cases.wrap(n_cells))


def test_three_ports_interleave(eng):
    check_case(eng, cases.three_ports())


# ---- copy and truncation ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell_size", [1504, 96], ids=["16 lanes", "4 lanes"])
@pytest.mark.parametrize("lead", range(8))
def test_payload_lengths_at_every_alignment(eng, lead, cell_size):
    check_case(eng, cases.payload_lengths(cell_size), lead=lead, parity=lead == 0)


@pytest.mark.parametrize("cell_size", [40, 48, 1504])
def test_truncation_by_one(eng, cell_size):
    check_case(eng, cases.truncation(cell_size))


def test_largest_datagram(eng):
    check_case(eng, cases.largest())


# ---- headers and key matching -------------------------------------------------------------------------------------

@pytest.mark.parametrize("listed", ["exact", "wildcard", "both"])
def test_header_geometries_and_the_wildcard(eng, listed):
    check_case(eng, cases.headers(listed))


def test_frames_with_their_fcs(eng):
    check_case(eng, cases.with_fcs())


def test_keys_one_bit_away(eng):
    check_case(eng, cases.near_keys())


# ---- launch shapes ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask", [0, 0xF, 0xFFFFFFFF])
def test_hash_masks(mask):
    """The result does not depend on the hash: 300 ports under a hash cut to nothing, to 4 bits, and whole."""
    from seqs_amd import Engine
    from seqs_amd.framesum import TEST_LIB_PATH

    te = Engine(0, lib_path=TEST_LIB_PATH)
    try:
        assert te.lib.fs_test_set_flow_hash_mask(te._ctx, mask) == 0
        check_case(te, cases.table_load(), parity=mask == 0xF)
    finally:
        te.close()


def test_one_workgroup_grid():
    from seqs_amd import Engine

    e = Engine(0)
    try:
        e.set_workgroups(1)
        check_case(e, cases.two_queues())
    finally:
        e.close()


@pytest.mark.parametrize("variant", engines.VARIANTS, ids=engines.IDS)
def test_every_engine_column(variant):
    e = engines.engine_for(variant)
    try:
        check_case(e, cases.columns(), parity=False)
    finally:
        e.close()


# ---- mixed and large batches --------------------------------------------------------------------------------------

def test_ports_beside_sockets_listeners_closers_and_openers(eng):
    check_case(eng, cases.mixed())


@pytest.mark.parametrize("n_ports", [1, 1000, 65536])
def test_benchmark_shape(eng, n_ports):
    check_case(eng, cases.benchmark(n_ports), parity=n_ports == 1000)


# ---- calls --------------------------------------------------------------------------------------------------------

def test_empty_calls(eng):
    check_case(eng, cases.empty_batch())  # n == 0: the input state, zero counts
    check_case(eng, cases.no_ports())     # n_ports == 0: the two fills alone
    check(eng, [], np.zeros(0, dtype=ref.PORT_DTYPE), 8)


def test_each_nullable_array_left_out(eng):
    case = cases.wrap(5)
    for port_of, cell_of in ((False, True), (True, False), (False, False)):
        check_case(eng, case, port_of=port_of, cell_of=cell_of, parity=False)


def test_eight_calls_in_flight(eng):
    import torch

    from seqs_amd.framesum import UDP_PORT_OUT_DTYPE

    dev = torch.device("cuda:0")
    lists = Lists()
    calls = []
    for k in range(8):
        case = cases.in_flight(k)
        buf, off, ln = fref.pack(case.frames, lead=k)
        cells0 = np.full(case.cells_bytes, 0xA0 + k, dtype=np.uint8)
        calls.append((case, cells0, (buf, off, ln), torch.from_numpy(cells0).to(dev), to_device(buf, off, ln),
                      torch.zeros(8, dtype=torch.uint8, device=dev)))
    results = [eng.udp_flows_device(*tb, lists.socks, lists.snd, rt, lists.listeners, lists.slots, lists.closers, lists.openers,
                                    case.ports, ct) for case, cells0, batch, ct, tb, rt in calls]
    torch.cuda.synchronize()
    for (case, cells0, batch, ct, tb, rt), res in zip(calls, results):
        want = ref.expected(case.frames, oracle_status(*batch), case.ports, cells0)
        case.reaches(want)
        assert res[0].cpu().numpy().reshape(-1).view(UDP_PORT_OUT_DTYPE).tobytes() == want[0].tobytes()
        assert np.array_equal(res[2].cpu().numpy().view(np.uint32), want[2]) and np.array_equal(ct.cpu().numpy(), want[3])


def test_host_form_with_a_cell_span_above_zero(eng):
    lists = Lists()
    case = cases.host_span()
    ports, cells_bytes = case.ports, case.cells_bytes
    buf, off, ln = fref.pack(case.frames, lead=3)
    cells0 = np.random.default_rng(8).integers(1, 256, cells_bytes + CELL_TAIL, dtype=np.uint8)
    want = ref.expected(case.frames, oracle_status(buf, off, ln), ports, cells0)
    cells = cells0.copy()
    res = eng.udp_flows_host(buf, off, ln, lists.socks, lists.snd, np.zeros(8, dtype=np.uint8), lists.listeners, lists.slots,
                             lists.closers, lists.openers, ports, cells[:cells_bytes])
    assert res[0].tobytes() == want[0].tobytes() and np.array_equal(res[1], want[1]) and np.array_equal(res[2], want[2])
    assert np.array_equal(cells, want[3]) and np.array_equal(cells[:4096], cells0[:4096])
    other = eng.connect_flows_host(buf, off, ln, lists.socks, lists.snd, np.zeros(8, dtype=np.uint8), lists.listeners, lists.slots,
                                   lists.closers, lists.openers)
    for k, (x, y) in enumerate(zip(res[3:], other)):
        assert (x is None and y is None) or np.asarray(x).tobytes() == np.asarray(y).tobytes(), f"connect-call output {k} differs"
    # the empty host call needs no device: the state comes back as it went in
    res = eng.udp_flows_host(buf[:0], off[:0], ln[:0], lists.socks, lists.snd, np.zeros(8, dtype=np.uint8), lists.listeners, lists.slots,
                             lists.closers, lists.openers, ports, cells[:cells_bytes])
    assert list(res[0]["wcell"]) == [39, 0] and list(res[0]["free"]) == [40, 50] and (res[0]["first"] == ref.NONE).all()
    assert np.array_equal(cells, want[3])


@pytest.mark.parametrize("which", range(len(cases.REJECTIONS)))
def test_every_rejection_with_its_text(eng, which):
    import torch

    from seqs_amd import FramesumError

    lists = Lists()
    ports, cells_bytes = cases.rejected_ports()
    change, text = cases.REJECTIONS[which]
    change(ports)
    buf, off, ln = fref.pack(list(cases.noisy()[:4]))
    dev = torch.device("cuda:0")
    ct = torch.full((cells_bytes,), 0x5A, dtype=torch.uint8, device=dev)
    rt = torch.zeros(8, dtype=torch.uint8, device=dev)
    for host in (False, True):
        with pytest.raises(FramesumError, match=re.escape(text)):
            if host:
                eng.udp_flows_host(buf, off, ln, lists.socks, lists.snd, np.zeros(8, dtype=np.uint8), lists.listeners, lists.slots,
                                   lists.closers, lists.openers, ports, np.full(cells_bytes, 0x5A, dtype=np.uint8))
            else:
                eng.udp_flows_device(*to_device(buf, off, ln), lists.socks, lists.snd, rt, lists.listeners, lists.slots, lists.closers,
                                     lists.openers, ports, ct)
    torch.cuda.synchronize()
    assert bool((ct == 0x5A).all())  # checked on the host before any device work


def test_null_arrays_and_too_many_ports_are_rejected(eng):
    import ctypes

    lib, ctx = eng.lib, eng._ctx
    none = ctypes.c_void_p()
    some = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(4096)))
    head = (ctx, none, none, none, 0, 0, 0, none, 0, none, 0, none, none, none, none, none)
    listen = (none, 0, none, 0, 0, none, none, none, none, none, none)
    closing = (none, 0, none, none, none)
    opening = (none, 0, 0, none, none, none, none)
    tail = (none, 0, none, none, none, none, some, none, none, none)
    row = ref.port_row(cases.US, 67, 4, 48)
    rp = ctypes.c_void_p(row.ctypes.data)
    for udp, text in (((none, 1, some, 4096, some, none, none), "port 0: null ports, cells or ports_out"),
                      ((rp, 1, none, 4096, some, none, none), "port 0: null ports, cells or ports_out"),
                      ((rp, 1, some, 4096, none, none, none), "port 0: null ports, cells or ports_out"),
                      ((rp, 65537, some, 4096, some, none, none), "port 0: n_ports above 65,536")):
        assert lib.fs_udp_flows_batch(*head, *listen, *closing, *opening, *udp, *tail) == -1
        assert lib.fs_last_error(ctx).decode() == "fs_udp_flows_batch: " + text
    # what the connect call rejects, this call rejects with its own name
    bad_flags = head[:6] + (2,) + head[7:]
    assert lib.fs_udp_flows_batch(*bad_flags, *listen, *closing, *opening, none, 0, none, 0, none, none, none, *tail) == -1
    assert lib.fs_last_error(ctx).decode() == "fs_udp_flows_batch: flags must be 0 or FS_RX_FCS"
