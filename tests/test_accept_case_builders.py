"""The batches of tests/accept_cases.py reach what they name, shown with the reference model alone
(tests/accept_ref.py's contract over tests/recv_ref.py): no GPU, no library call."""
import numpy as np
import pytest

import accept_cases as cases
import accept_ref as ref
import flows_ref as fref


def expect(case, mtu=0, synack_flags=0):
    buf, off, ln = fref.pack(case.frames, lead=1)
    noise = np.zeros(8, dtype=np.uint8)
    rings = np.zeros(case.rings_bytes, dtype=np.uint8)
    synacks = np.full(len(case.slots) * ref.STRIDE, 0xEE, dtype=np.uint8)
    return ref.expected(buf, off, ln, mtu, 0, noise, 0, 0, case.socks, case.snd, rings, case.listeners, case.slots,
                        synack_flags, synacks)


def filled(e):
    return [int(s) for s in np.flatnonzero(e["conns"]["used"])]


@pytest.mark.parametrize("n_slots", [9, 8, 1, 0])
def test_lanes_put_the_candidates_at_the_boundaries(n_slots):
    case = cases.lanes(n_slots)
    e = expect(case)
    assert e["n_flows"] == 300 and e["n_accepted"] == 300  # one-frame flows: flow f is frame f
    assert [int(e["conns"]["flow"][s]) for s in filled(e)] == list(cases.LANE_CANDIDATES[:n_slots])
    assert [int(e["accept_of"][f]) for f in cases.LANE_CANDIDATES] == list(range(n_slots)) + [ref.FULL] * (9 - n_slots)
    assert int((e["accept_of"] == ref.NONE).sum()) == 291
    # the candidates lie on both sides of a wave's and of a scan block's last lane
    assert {63, 64} <= set(cases.LANE_CANDIDATES) and {255, 256} <= set(cases.LANE_CANDIDATES)
    # the others are what the builder says: ACKs and data and UDP to the listener's own address and port
    kinds = {(fr[23], ref.local_of(fr) == cases.local(80), ref.is_first_syn(fr)) for fr in case.frames}
    assert kinds == {(6, True, True), (6, True, False), (17, True, False), (6, False, True)}
    # Seq crosses 2^32 among the candidates, and the odd ones carry an MSS option
    assert int(e["conns"]["rcv_nxt"][0]) == (1 << 32) - 2 if n_slots else True
    if n_slots == 9:
        assert [int(x) for x in e["conns"]["peer_mss"]] == [0, 1460, 0, 1460, 0, 1460, 1460, 0, 1460]
        assert 0 in [int(x) for x in e["conns"]["irs"]] or (1 << 32) - 3 in [int(x) for x in e["conns"]["irs"]]


def test_three_listeners_interleave():
    case = cases.three_listeners()
    e = expect(case, synack_flags=ref.FCS_APPEND)
    assert [int(x) for x in e["listeners_out"]["n_syn"]] == [3, 7, 5]
    assert [int(x) for x in e["listeners_out"]["n_full"]] == [0, 0, 2]
    assert filled(e) == [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14] and not e["conns"]["used"][[3, 11, 15]].any()
    # consecutive flows go to different listeners: the ranks interleave
    owners = [ref.local_of(f) for f in case.frames[:6]]
    assert owners[0] != owners[1] != owners[2] and owners[0] == owners[3]
    # a SYN-ACK: 58 bytes written, the rest of the slot's 64 untouched, the listener's own MAC
    slot = int(e["accept_of"][0])
    row = e["synacks"][slot * 64 : slot * 64 + 64]
    assert bytes(row[58:]) == b"\xEE" * 6 and bytes(row[6:12]) == cases.MAC and row[47] == 0x12
    assert bytes(e["synacks"][3 * 64 : 4 * 64]) == b"\xEE" * 64


def test_near_misses():
    case = cases.near_misses()
    e = expect(case)
    assert e["n_flows"] == 3 and int(e["st"][3]) == 13 and [int(x) for x in e["accept_of"][:3]] == [ref.NONE, ref.NONE, 0]
    assert ref.is_first_syn(case.frames[0]) and fref.flow_key(case.frames[0]) == bytes(case.socks["key"][0])
    assert not ref.is_first_syn(case.frames[1]) and ref.is_first_syn(case.frames[2])
    assert fref.flow_key(case.frames[1]) == fref.flow_key(case.frames[2])
    assert int(e["socks_out"]["stop"][0]) == 0  # the SYN ends the socket's walk at once


def test_grid_reaches_every_case():
    case = cases.grid()
    e = expect(case)
    m = case.info["misses"]
    assert m == 10 and (e["accept_of"][:m] == ref.NONE).all() and e["n_flows"] == len(case.frames)
    assert list(e["accept_of"][m : len(case.frames)]) == list(range(len(cases.GRID_GOOD)))
    windows = {int.from_bytes(bytes(e["synacks"][s * 64 + 48 : s * 64 + 50]), "big") for s in filled(e)}
    assert windows == {0, 65535} and {int(x) for x in e["conns"]["snd_wnd"]} == {0, 1, 65535}
    assert {int(x) for x in e["conns"]["rcv_nxt"]} == {8, 0}


def test_geometries():
    case = cases.geometries()
    e = expect(case)
    assert len(case.frames) == 36 and (e["conns"]["used"] == 1).all()
    assert [int(x) for x in e["conns"]["peer_mss"]] == case.info["mss"]
    assert {len(f) for f in case.frames} == {54 + 4 * a + 4 * b for a in (0, 1, 10) for b in (0, 1, 10)}


@pytest.mark.parametrize("shape", cases.BIG_SHAPES)
def test_big_shapes(shape):
    case = cases.big(shape)
    e = expect(case)
    assert int((e["st"] != 0).sum()) == 0
    assert int(e["listeners_out"]["n_syn"].sum()) == cases.BIG
    assert int(e["listeners_out"]["n_full"].sum()) == case.info["n_full"] == int((e["accept_of"] == ref.FULL).sum())
    if shape == "among established frames":
        assert int(e["snd_out"]["n_taken"].sum()) == 65536 and e["n_flows"] == cases.BIG + 64
