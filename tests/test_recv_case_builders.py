"""The batches of tests/recv_cases.py reach what they name: shown on the CPU with the restatement of
tests/recv_ref.py alone, so that tests/test_gpu_recv.py, which compares the GPU against that same
restatement, is known to exercise every code at every lane position it claims."""
import numpy as np
import pytest

import flows_ref as fref
import recv_cases as cases
import recv_ref as ref


def reference(case):
    buf, off, ln = fref.pack(case.frames, lead=1)
    rings = np.zeros(case.rings_bytes, dtype=np.uint8)
    e = ref.expected(buf, off, ln, 0, 0, np.zeros(int(ln.sum()), dtype=np.uint8), 0, None, case.socks, case.snd, rings)
    assert (e["st"] == 0).all(), "every frame of a case passes RecvEth"
    return e


@pytest.mark.parametrize("n,code,positions", cases.LANE_FLOWS)
def test_lane_flows_place_their_code(n, code, positions):
    case = cases.lane_flow(n, code, positions)
    e = reference(case)
    assert len(case.frames) == n and int(e["socks_out"]["stop"][0]) == n
    at = case.info["positions"]
    assert all(int(e["code"][p]) == code for p in at), [int(e["code"][p]) for p in at]
    others = [int(c) for k, c in enumerate(e["code"]) if k not in at]
    assert code not in others and set(others) <= {1, 2}
    o = e["snd_out"][0]
    if positions is None:
        assert set(at) == {p for p in cases.POSITIONS if p < n} and {0, 63, 64, 127, 128} <= set(at)
    if code == 1:
        # the window is the last special slot's, which lies in an earlier chunk than the flow's end
        assert int(o["snd_wnd"]) == 2000 + max(at) and int(o["n_taken"]) == len(at)
        if positions is not None:
            assert max(at) // 64 < (n - 1) // 64
    else:
        assert int(o["n_taken"]) == n - len(at) and int(o["snd_una"]) == (0x20000 - 5000 + n - len(at)) % (1 << 32)
    if code == 6:
        assert int(e["socks_out"]["n_dropped"][0]) == len(at)
    # rcv.NXT crosses 2^32 inside the flow (the data segments are admitted)
    if code != 1:
        assert int(e["socks_out"]["rcv_nxt"][0]) < 1000 and int(e["socks_out"]["n_delivered"][0]) > 10


def test_lane_flows_cover_every_code_at_every_position():
    seen = {(code, p) for n, code, positions in cases.LANE_FLOWS if positions is None
            for p in cases.lane_flow(n, code).info["positions"]}
    assert seen == {(code, p) for code in range(1, 7) for p in cases.POSITIONS}


@pytest.mark.parametrize("build", [*(lambda n=n: cases.composition(n) for n in cases.COMPOSITIONS), cases.keepalives,
                                   *(lambda k=k: cases.stops(k) for k in cases.STOPS), cases.geometries],
                         ids=[*cases.COMPOSITIONS, "keepalives", *cases.STOPS, "geometries"])
def test_small_cases_expect_what_the_reference_gives(build):
    case = build()
    e = reference(case)
    o = e["snd_out"][0]
    assert [int(c) for c in e["code"]] == case.info["codes"]
    assert (int(o["snd_una"]), int(o["snd_wnd"]), int(o["flags"])) == (case.info["una"], case.info["wnd"], case.info["flags"])
    if "n_keepalive" in case.info:
        assert int(o["n_keepalive"]) == case.info["n_keepalive"]


def test_half_in_a_full_chunk_is_the_point():
    case = cases.composition("half in a full chunk")
    segs = [ref.fields(f) for f in case.frames]
    # at slot 31 una == snd_nxt and the Ack lies exactly 2^31 behind: min() over distances would drop it
    codes, una, _, _ = ref.contract(segs[:31], [False] * 31, int(case.snd["snd_una"][0]), 0, 500, 5, 65535)
    assert una == 5 and (5 - segs[31][1]) % (1 << 32) == 1 << 31 and len(case.frames) > 64


def test_geometries_cover_the_header_grid():
    case = cases.geometries()
    seen = {(f[14] & 15, f[14 + 4 * (f[14] & 15) + 12] >> 4) for f in case.frames}
    assert seen >= {(i, d) for i in (5, 6, 15) for d in (5, 6, 15)}


def test_random_flows_reach_every_code():
    case = cases.random_flows()
    e = reference(case)
    counts = np.bincount(e["code"], minlength=7)
    assert (counts[1:] > 20).all(), counts
    assert len(case.socks) == 64 and (e["socks_out"]["flow"] != ref.NONE).all()
    assert {int(f) for f in e["snd_out"]["flags"]} >= {0, 1} or {int(f) for f in e["snd_out"]["flags"]} == {1}
    # snd.UNA ends on both sides of 2^32, and some socket's moved backwards
    una = e["snd_out"]["snd_una"].astype(np.int64)
    assert (una < 1000).any() and (una > (1 << 32) - 1000).any()


def test_round_trip_case():
    case = cases.round_trip()
    e = reference(case)
    assert [int(c) for c in e["code"]] == [1, 2, 1]
    assert [int(x) for x in e["snd_out"]["snd_wnd"]] == [60, 0, 30] and [int(x) for x in e["snd_out"]["snd_una"]] == [995, 990, 992]
    assert [int(x) for x in e["snd_out"]["flags"]] == [0, 0, ref.ACK_OWED]
