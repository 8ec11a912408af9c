"""The receive call on the GPU at the shapes tests/test_gpu_recv.py leaves out, against the same
restatement (tests/recv_ref.py) and through the same comparison (test_gpu_recv.check: snd_out, code,
every output of the delivery, the WHOLE rings buffer): state that changes in every chunk of rounds 2
to 5 of a socket's walk, four waves of one workgroup walking 5, 3, 2 and 1 rounds, a chunk of 64
constants, admitted data segments and late chunks at the half point, payloads above 2^15 bytes, and
frames of a socket's flow that RecvEth drops. The batches are tests/recv_cases.py's, which
tests/test_recv_case_builders.py shows to reach what they name. Every batch is valid input."""
import numpy as np
import pytest

import flows_ref as fref
import recv_cases as cases
import recv_ref as ref
from test_gpu_deliver import TAIL, compare_delivery, sentinel, to_device
from test_gpu_recv import check_case, compare_recv

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


@pytest.fixture(scope="module")
def one_workgroup(eng):
    """A test-library engine whose every launch is one workgroup (tests/test_gpu_recv.py's
    test_hash_mask_and_one_workgroup)."""
    from seqs_amd import Engine
    from seqs_amd.framesum import TEST_LIB_PATH

    te = Engine(0, lib_path=TEST_LIB_PATH)
    te.set_workgroups(1)
    yield te
    te.close()


def check_host(eng, case, e, lead=1, seed=0):
    """fs_recv_flows_batch_host of the case over the buffers check_case(..., lead=lead, seed=seed) made:
    every output against that check's expected dict `e`."""
    buf, off, ln = fref.pack(case.frames, lead=lead)
    room = int(ln.sum())
    mine = np.random.default_rng(77 + seed).integers(0, 256, 3 + room + TAIL, dtype=np.uint8)
    rings = sentinel(case.rings_bytes, seed)
    sn, code, so, dl, pay, runs, flows, order, run_of, totals, dig, st = eng.recv_flows_host(
        buf, off, ln, case.socks, case.snd, rings, payload=mine[3 : 3 + room])
    assert sn.tobytes() == e["snd_out"].tobytes(), (sn[:4], e["snd_out"][:4])
    bad = np.flatnonzero(code != e["code"])
    assert bad.size == 0, f"{bad.size} codes differ, first at {bad[:8]}: {code[bad[:8]]} for {e['code'][bad[:8]]}"
    assert so.tobytes() == e["socks_out"].tobytes() and np.array_equal(dl, e["delivered"]) and np.array_equal(rings, e["rings"])
    assert np.array_equal(mine, e["payload"]) and runs.tobytes() == e["runs"].tobytes() and flows.tobytes() == e["flows"].tobytes()
    assert np.array_equal(order, e["order"]) and np.array_equal(run_of, e["run_of"]) and np.array_equal(st, e["st"])


# ---- a. rounds 2 to 5 of one socket's walk ---------------------------------------------------------

@pytest.mark.parametrize("n,code,positions", cases.LONG_LANE_FLOWS)
def test_every_code_in_the_later_rounds(eng, n, code, positions):
    case = cases.lane_flow(n, code, positions)
    e = check_case(eng, case, lead=code % 4, seed=code)
    assert [int(e["code"][p]) for p in positions] == [code] * len(positions) and int(e["socks_out"]["stop"][0]) == 1030


# ---- b. four waves of one workgroup, 5, 3, 2 and 1 rounds -------------------------------------------

def test_four_long_flows_in_one_workgroup(eng, one_workgroup):
    case = cases.four_long_flows()
    e = check_case(eng, case, lead=2, seed=1)
    assert [int(s) for s in e["socks_out"]["stop"]] == [1030, 1552, 1873, 1943]
    check_case(one_workgroup, case, lead=2, seed=1, e=e)
    check_host(eng, case, e, lead=2, seed=1)


# ---- c. a chunk of 64 constants --------------------------------------------------------------------

@pytest.mark.parametrize("dense", cases.DENSE)
def test_dense_constants(eng, one_workgroup, dense):
    case = cases.dense_constants(dense)
    e = check_case(eng, case, lead=3, seed=2)
    assert [int(c) for c in e["code"][:dense]] == [1] * dense and int(e["snd_out"]["snd_una"][0]) == case.info["una"]
    check_case(one_workgroup, case, lead=3, seed=2, e=e)


# ---- d. the half point -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", cases.HALF_SMALL)
def test_data_segments_at_the_half_point(eng, one_workgroup, name):
    case = cases.half_small(name)
    e = check_case(eng, case, seed=3)
    assert [int(c) for c in e["code"]] == case.info["codes"] and [int(d) for d in e["delivered"]] == case.info["delivered"]
    assert tuple(int(x) for x in e["snd_out"][0]) == case.info["snd_out"]
    check_case(one_workgroup, case, seed=3, e=e)


def test_half_points_in_a_late_partial_chunk(eng, one_workgroup):
    case = cases.half_long()
    e = check_case(eng, case, lead=1, seed=4)
    assert {k: int(e["code"][k]) for k in case.info["at"]} == case.info["at"] and int(e["snd_out"]["snd_wnd"][0]) == 503
    check_case(one_workgroup, case, lead=1, seed=4, e=e)
    check_host(eng, case, e, lead=1, seed=4)


# ---- e. payloads above 2^15 ------------------------------------------------------------------------

def test_jumbo_payloads(eng):
    case = cases.jumbo()
    e = check_case(eng, case, lead=1, seed=5)
    assert [int(c) for c in e["code"]] == [1, 1, 5] * 5 and tuple(int(x) for x in e["snd_out"][0]) == case.info["snd_out"]
    assert int(e["socks_out"]["rcv_nxt"][0]) == 227_405


# ---- f. frames of the flow that are not slots ------------------------------------------------------

@pytest.mark.parametrize("name", list(cases.NOT_SLOTS))
def test_frames_that_are_not_slots(eng, name):
    case = cases.not_slots(name)
    e = check_case(eng, case, lead=2, seed=6)
    hit = [case.info["mine"][k] for k in case.info["damaged"]]
    assert (e["st"][hit] != 0).all() and not e["code"][hit].any() and not e["code"][case.info["foreign"]].any()
    assert int(e["socks_out"]["stop"][0]) == 130 - len(hit)
    check_host(eng, case, e, lead=2, seed=6)


# ---- back-to-back calls whose scratch grows and shrinks --------------------------------------------

def test_back_to_back_calls_of_very_different_sizes(eng):
    import torch

    from test_gpu_flows import compare

    dev = torch.device("cuda:0")
    built = [cases.composition("una goes back"), cases.lane_flow(1030, 4, cases.LONG_POSITIONS), cases.dense_constants(64),
             cases.jumbo(), cases.composition("una goes back"), cases.lane_flow(1030, 2, cases.LONG_POSITIONS),
             cases.half_small(cases.HALF_SMALL[0]), cases.dense_constants(48)]
    assert [len(c.frames) for c in built] == [5, 1030, 150, 15, 5, 1030, 6, 150]
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
