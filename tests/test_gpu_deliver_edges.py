"""The in-order TCP delivery on the GPU at the shapes tests/test_gpu_deliver.py does not reach: the
batches of tests/deliver_cases.py (tests/test_deliver_case_builders.py shows without a GPU that each
reaches what it names) through test_gpu_deliver.check: socks_out, delivered, the whole rings buffer over
the sentinel and every coalesce output against tests/deliver_ref.py, bit for bit. Then 40 calls in
flight at once, and the host form without sockets and with a ring span that starts above 0."""
import numpy as np
import pytest

import deliver_cases as dc
import deliver_ref as ref
import engines
import flows_ref as fref
from test_gpu_deliver import TAIL, check, compare_delivery, eng, three_flows, to_device  # noqa: F401  (eng: the fixture)

pytestmark = pytest.mark.gpu


def run(engine, case, e=None, **kw):
    return check(engine, None, case.socks, case.rings_bytes, flags=case.flags, batch=case.batch, e=e, **kw)


def one_workgroup():
    from seqs_amd import Engine

    e = Engine(0)
    e.set_workgroups(1)
    return e


# ---- a. to h. ------------------------------------------------------------------------------------

@pytest.mark.parametrize("interleaved", [False, True], ids=["contiguous", "round robin"])
def test_flow_ends_at_every_lane(eng, interleaved):
    case = dc.flow_ends_at_every_lane(interleaved)
    e = run(eng, case)
    assert (e["socks_out"]["n_dropped"] == 1).all() and e["n_flows"] == 69
    one = one_workgroup()
    try:
        run(one, case, e=e)
    finally:
        one.close()


def test_events_at_chunk_positions(eng):
    case = dc.events_at_chunk_positions()
    e = run(eng, case, payload=False)
    assert e["n_flows"] == 160 and len(set(e["socks_out"]["stop"].tolist())) == 80
    one = one_workgroup()
    try:
        run(one, case, e=e, payload=False)
    finally:
        one.close()


def test_restart_patterns(eng):
    case = dc.restart_patterns()
    e = run(eng, case)
    assert [int(x) for x in e["socks_out"]["n_dropped"]] == [sum(dc.PATTERN_DROPS[p]) for p in dc.PATTERNS]


def test_wrap_splits_small(eng):
    case = dc.wrap_splits_small()
    e = run(eng, case)
    assert (e["socks_out"]["n_delivered"] == 1).all() and case.socks.size == 860


def test_wrap_splits_large(eng):
    case = dc.wrap_splits_large()
    e = run(eng, case, payload=False)
    assert int(e["socks_out"]["n_delivered"][case.info["jumbo_sock"]]) == 40


@pytest.mark.parametrize("variant", engines.VARIANTS, ids=engines.IDS)
def test_header_geometries(variant):
    import torch

    assert torch.cuda.is_available()
    e2 = engines.engine_for(variant)
    try:
        for fcs in (False, True):
            e = None
            for lead in range(16):
                e = run(e2, dc.header_case(fcs, lead), e=e)  # (the result does not depend on where the frames lie)
            assert list(e["st"]) == [0] * 122 and list(e["delivered"]) == [1] * 122
    finally:
        e2.close()


def test_near_miss_keys(eng):
    from seqs_amd import Engine
    from seqs_amd.framesum import TEST_LIB_PATH

    case = dc.near_miss_keys()
    e = run(eng, case)
    assert e["n_flows"] == 16 and [int(x) for x in e["socks_out"]["flow"]] == [15, 14, ref.NONE]
    te = Engine(0, lib_path=TEST_LIB_PATH)
    try:
        for mask in (0, 0xF, 0xFFFFFFFF):
            assert te.lib.fs_test_set_flow_hash_mask(te._ctx, mask) == 0
            run(te, case, e=e)
    finally:
        te.close()


@pytest.mark.parametrize("shape", ["one flow", "1000 flows", "every frame its own flow"])
def test_big_batches(eng, shape):
    case = dc.big_batches(shape)
    e = run(eng, case, payload=False)
    assert e["n_accepted"] == 65793 and int(e["socks_out"]["bytes"].sum()) == (655360 if shape.startswith("every") else 657930)


# ---- more calls in flight than the context has staged blocks -------------------------------------

def test_40_calls_without_a_synchronization(eng):
    import torch

    from test_gpu_flows import compare

    rings0, calls = dc.chained_calls()
    assert len(calls) == 40
    dev = torch.device("cuda:0")
    rt = torch.from_numpy(rings0).to(dev)
    batches = [to_device(*batch) for batch, _, _ in calls]
    pts = [torch.from_numpy(np.random.default_rng(j).integers(0, 256, 3 + TAIL, dtype=np.uint8)).to(dev) for j in range(40)]
    torch.cuda.synchronize()
    # call j's sockets are call j - 1's expected socks_out: nothing is read back in between
    res = [eng.deliver_flows_device(*b, socks, rt, payload=False) for b, (_, socks, _), pt in zip(batches, calls, pts)]
    torch.cuda.synchronize()
    for j, ((_, _, e), r, pt) in enumerate(zip(calls, res, pts)):
        last = dict(e, rings=calls[-1][2]["rings"])  # the rings buffer is read once, after the last call
        compare_delivery(last, r[0], r[1], rt)
        compare(e, pt.cpu().numpy(), *r[3:])


# ---- the host form -------------------------------------------------------------------------------

def host_call(eng, case, rings, room):
    buf, off, ln = case.batch
    noise = np.random.default_rng(61).integers(0, 256, room + TAIL, dtype=np.uint8)
    e = ref.expected(buf, off, ln, 0, case.flags, noise, 0, room, case.socks, rings)
    mine, got_rings = noise.copy(), rings.copy()
    so, dl, pay, runs, flows, order, run_of, totals, dig, st = eng.deliver_flows_host(
        buf, off, ln, case.socks, got_rings, 0, case.flags, payload=mine[:room] if room else False)
    assert so.tobytes() == e["socks_out"].tobytes() and np.array_equal(dl, e["delivered"])
    bad = np.flatnonzero(got_rings != e["rings"])
    assert bad.size == 0, f"{bad.size} ring bytes differ, first at {bad[:8]}"
    assert np.array_equal(mine, e["payload"]) and runs.tobytes() == e["runs"].tobytes()
    assert flows.tobytes() == e["flows"].tobytes() and np.array_equal(order, e["order"])
    assert np.array_equal(run_of, e["run_of"]) and np.array_equal(dig, e["dig"]) and np.array_equal(st, e["st"])
    assert (int(totals["payload_bytes"]), int(totals["n_runs"]), int(totals["n_flows"]), int(totals["n_accepted"])) == \
        (e["payload_bytes"], e["n_runs"], e["n_flows"], e["n_accepted"])
    return e, (so, dl, pay, runs, flows, order, run_of, totals, dig, st)


def test_host_form_without_sockets(eng):
    from test_gpu_deliver import sentinel

    _, frames = three_flows(np.random.default_rng(83))
    case = dc.Case(fref.pack(frames, lead=7), ref.socks_of(), 100)
    room = int(case.batch[2].sum())
    rings = sentinel(100, 3)
    e, got = host_call(eng, case, rings, room)
    assert got[0].size == 0 and got[1].size == len(frames) and not got[1].any() and e["n_flows"] == 4
    pay = np.random.default_rng(61).integers(0, 256, room + TAIL, dtype=np.uint8)
    plain = eng.coalesce_flows_host(*case.batch, payload=pay[:room])
    assert np.array_equal(pay, e["payload"])
    for x, y in zip(plain[1:], got[3:]):
        assert x.tobytes() == y.tobytes()


def test_host_form_of_the_jumbo_flow(eng):
    from test_gpu_deliver import sentinel

    case = dc.jumbo_flow()
    lo = int(case.socks["ring_off"].min())
    assert lo == 4099 and case.rings_bytes > int((case.socks["ring_off"] + case.socks["ring_size"]).max()) + 400
    e, got = host_call(eng, case, sentinel(case.rings_bytes, 4), 0)
    assert list(got[1]) == [1] * 40 + [2] * 24 and int(got[0]["bytes"][0]) == 40 * dc.JUMBO
    assert int(got[0]["flow"][1]) == ref.NONE
