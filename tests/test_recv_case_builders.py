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


# ==== the edge suite's batches (tests/test_gpu_recv_edges.py) =====================================

def reference_any(case):
    """reference() for a case whose frames need not all pass RecvEth."""
    buf, off, ln = fref.pack(case.frames, lead=1)
    rings = np.zeros(case.rings_bytes, dtype=np.uint8)
    return ref.expected(buf, off, ln, 0, 0, np.zeros(int(ln.sum()), dtype=np.uint8), 0, None, case.socks, case.snd, rings)


def codes_of(e, at=None):
    return [int(c) for c in (e["code"] if at is None else e["code"][at])]


@pytest.mark.parametrize("n,code,positions", cases.LONG_LANE_FLOWS)
def test_long_lane_flows_place_their_code(n, code, positions):
    case = cases.lane_flow(n, code, positions)
    e = reference(case)
    assert len(case.frames) == n == 1030 and int(e["socks_out"]["stop"][0]) == 1030 and len(positions) == 20
    assert [int(e["code"][p]) for p in positions] == [code] * 20
    others = [int(c) for k, c in enumerate(e["code"]) if k not in positions]
    assert others == [2 if code == 1 else 1] * 1010


def test_long_positions_lie_in_every_chunk_behind_the_first_round():
    """Round 2 at its first and last slot of all four chunks; rounds 3 and 4 at their first and last
    chunk (round 3 also at chunk 1); the last round's partial chunk of 6 slots at both ends. The frames
    between the positions move snd.UNA and rcv.NXT in every chunk of every round."""
    seen = {cases.round_and_chunk(p) for p in cases.LONG_POSITIONS}
    assert {(2, c) for c in range(4)} <= seen and {(3, 0), (3, 1), (3, 3), (4, 0), (4, 3), (5, 0)} <= seen
    assert {c for r, c in seen if r in (2, 3, 4)} == {0, 1, 2, 3} and {r for r, _ in seen} == {1, 2, 3, 4, 5}
    assert {256, 319, 320, 383, 384, 447, 448, 511, 512, 767, 768, 1023} <= set(cases.LONG_POSITIONS)
    assert cases.round_and_chunk(1029) == (5, 0) and 1029 % 64 == 5 and {1024, 1029} <= set(cases.LONG_POSITIONS)
    # the other frames of a flow whose special code is not 1: a new Ack in every slot, data in every chunk
    case = cases.lane_flow(1030, 2, cases.LONG_POSITIONS)
    segs = [ref.fields(f) for f in case.frames]
    for chunk in range(0, 1030, 64):
        mine = segs[chunk : chunk + 64]
        assert len({s[1] for s in mine}) >= len(mine) - 3 and sum(1 for s in mine if s[4]) >= 1


def test_four_long_flows_walk_5_3_2_and_1_rounds():
    import deliver_cases as dcases

    case = cases.four_long_flows()
    e = reference(case)
    dcases.check_layout(case.socks, case.rings_bytes)
    assert [int(s) for s in e["socks_out"]["stop"]] == [1030, 1552, 1873, 1943] and len(case.frames) == 1943
    assert [int(f) for f in e["socks_out"]["flow"]] == [0, 1, 2, 3]
    first = [0, 1030, 1552, 1873]
    assert [-(-(int(s) - f) // 256) for s, f in zip(e["socks_out"]["stop"], first)] == [5, 3, 2, 1]
    assert len({spec[1] for spec in cases.FOUR_FLOWS}) == 4
    for g, part in enumerate(case.info["parts"]):
        alone = reference(part)
        assert codes_of(e, case.info["mine"][g]) == codes_of(alone)
        assert e["snd_out"][g].tobytes() == alone["snd_out"][0].tobytes()


@pytest.mark.parametrize("dense", cases.DENSE)
def test_dense_constants_fill_a_chunk(dense):
    case = cases.dense_constants(dense)
    e = reference(case)
    segs = [ref.fields(f) for f in case.frames]
    codes = codes_of(e)
    assert len(segs) == 150 and int(e["socks_out"]["stop"][0]) == 150
    # the first `dense` slots: admitted data segments with ACK, each a constant of the scan
    assert all(s[4] == 1 and s[3] & ref.ACK for s in segs[:dense]) and codes[:dense] == [1] * dense
    assert (e["delivered"][:dense] == 1).all() and segs[dense][4] == 0
    sock, una0 = case.socks[0], int(case.snd["snd_una"][0])
    snd_nxt = int(sock["snd_nxt"])
    admitted = [s[4] == 1 for s in segs]
    unas = [ref.contract(segs[:k], admitted[:k], una0, 0, int(sock["rcv_nxt"]), snd_nxt, 65535)[1] for k in range(dense + 1)]
    assert sum(1 for a, b in zip(unas, unas[1:]) if ref.less_than(b, a)) >= (20 if dense == 64 else 15)
    assert all(0 <= (snd_nxt - s[1]) % (1 << 32) <= 900 for s in segs[:dense]) and len({s[2] for s in segs}) == 150
    # the first pure ACK is newer than the snd.UNA behind all the constants, and would be a duplicate behind
    # the constants from slot 31 on taken as a minimum of distances (a count of constants that stops at 32)
    assert codes[dense] == 1 and ref.less_than(unas[dense], segs[dense][1])
    assert any(not ref.less_than(u, segs[dense][1]) for u in unas[32:dense])
    # the chunks behind them: pure ACKs on both sides of the snd.UNA before them
    for lo, hi in ((64, 128), (128, 150)):
        pure = [k for k in range(lo, hi) if segs[k][4] == 0]
        assert sum(1 for k in pure if codes[k] == 1) >= 8 and sum(1 for k in pure if codes[k] == 2) >= 8
        assert {codes[k] for k in range(lo, hi)} == {1, 2} and any(segs[k][4] for k in range(lo, hi))
    if dense == 64:
        assert sum(1 for k in range(64) if segs[k][4] and codes[k] == 1) == 64  # 64 code-1 constants in chunk 0
    else:
        pure = [k for k in range(dense, 64) if segs[k][4] == 0]
        assert sum(1 for k in pure if codes[k] == 1) >= 4 and sum(1 for k in pure if codes[k] == 2) >= 4
        assert sum(1 for s in segs[:64] if s[4]) == 52
    o = e["snd_out"][0]
    last = max(k for k in range(150) if codes[k] == 1)
    assert int(o["snd_wnd"]) == segs[last][2] == case.info["windows"][last] and int(o["snd_una"]) == case.info["una"] % (1 << 32)
    assert int(e["socks_out"]["rcv_nxt"][0]) < 100  # rcv.NXT has crossed 2^32


@pytest.mark.parametrize("name", cases.HALF_SMALL)
def test_half_small_is_what_it_is_pinned_to(name):
    case = cases.half_small(name)
    e = reference(case)
    assert codes_of(e) == case.info["codes"] and [int(d) for d in e["delivered"]] == case.info["delivered"]
    assert tuple(int(x) for x in e["snd_out"][0]) == case.info["snd_out"]
    segs = [ref.fields(f) for f in case.frames]
    pure_half = [k for k, s in enumerate(segs) if s[4] == 0 and (1000 - s[1]) % (1 << 32) == 1 << 31]
    assert pure_half == ([3] if name == cases.HALF_SMALL[0] else [])
    # the data segments at the half point are admitted, and the frame behind each meets a snd.UNA 2^31 behind
    assert [k for k, s in enumerate(segs) if s[4] and (1000 - s[1]) % (1 << 32) == 1 << 31] == [0, 2] and e["delivered"][0] == e["delivered"][2] == 1


def test_half_long_has_its_points_in_a_late_partial_chunk():
    case = cases.half_long()
    e = reference(case)
    first, stop = int(e["flows"][0]["first_frame"]), int(e["socks_out"]["stop"][0])
    assert {k: int(e["code"][k]) for k in (390, 393, 395, 396)} == case.info["at"] == {390: 1, 393: 1, 395: 1, 396: 2}
    assert (390 - first) // 64 == 6 and stop - (first + 6 * 64) == 16 and stop == 400
    segs = [ref.fields(f) for f in case.frames]
    snd_nxt = int(case.socks["snd_nxt"][0])
    una = ref.contract(segs[:390], [False] * 390, int(case.snd["snd_una"][0]), 0, 500, snd_nxt, 65535)[1]
    assert una == snd_nxt and all((snd_nxt - segs[k][1]) % (1 << 32) == 1 << 31 for k in (390, 395, 396))
    assert segs[393][4] == 3 and segs[393][1] == snd_nxt and int(e["delivered"][393]) == 1
    assert codes_of(e).count(1) == 398 and codes_of(e).count(2) == 2
    o = e["snd_out"][0]
    assert (int(o["snd_una"]), int(o["snd_wnd"])) == (case.info["una"], case.info["wnd"])


def test_jumbo_is_what_it_is_pinned_to():
    import deliver_cases as dcases

    case = cases.jumbo()
    e = reference(case)
    assert codes_of(e) == case.info["codes"] == [1, 1, 5] * 5
    assert tuple(int(x) for x in e["snd_out"][0]) == case.info["snd_out"] == (910, 64, 10, 0, 0, 0, 5, ref.ACK_OWED)
    assert int(e["socks_out"]["rcv_nxt"][0]) == case.info["rcv_nxt_out"] == 227_405
    assert [ref.fields(f)[4] for f in case.frames[::3]] == [dcases.JUMBO] * 5 and dcases.JUMBO >= 1 << 15
    assert [ref.fields(f)[2] for f in case.frames] == [w + k for k in range(5) for w in (50, 60, 70)]
    assert case.rings_bytes <= 400 * 1024 and int(e["socks_out"]["ring_wpos"][0]) < int(case.socks["ring_wpos"][0])  # the ring wrapped


@pytest.mark.parametrize("name", list(cases.NOT_SLOTS))
def test_frames_that_are_not_slots(name):
    case = cases.not_slots(name)
    e = reference_any(case)
    mine, foreign, damaged = case.info["mine"], case.info["foreign"], case.info["damaged"]
    assert len(mine) == 130 and len(foreign) == 50 and not e["code"][foreign].any() and (e["st"][foreign] == 0).all()
    assert {case.frames[i][23] for i in foreign} == {6, 17}
    assert all(case.frames[i][26:38] == case.frames[mine[0]][26:38] for i in foreign if case.frames[i][23] == 17)
    hit = [mine[k] for k in damaged]
    assert (e["st"][hit] != 0).all() and not e["code"][hit].any() and int((e["st"] != 0).sum()) == len(damaged)
    assert int(e["socks_out"]["stop"][0]) == 130 - len(damaged) and int(e["socks_out"]["flow"][0]) == 0
    codes = codes_of(e, mine)
    alone = codes_of(reference(case.info["base"]))
    if name == "damaged pure ACKs":
        # the damaged frames were duplicates: the others keep their codes, one or two lanes lower
        assert alone[63] == alone[64] == 2
        assert [c for k, c in enumerate(codes) if k not in damaged] == [c for k, c in enumerate(alone) if k not in damaged]
        assert int(e["snd_out"]["n_dup"][0]) == alone.count(2) - 2
    else:
        assert np.bincount(e["code"][mine], minlength=7).tolist() == [3, 8, 2, 0, 117, 0, 0]
        assert codes[:10] == alone[:10] and set(codes[11:63] + codes[65:]) == {4}
        assert int(e["socks_out"]["n_delivered"][0]) == 1 and int(e["socks_out"]["n_dropped"][0]) == 17
        assert int(e["socks_out"]["stop"][0]) == 127
