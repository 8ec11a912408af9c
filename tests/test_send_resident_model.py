"""The sequential model of the resident ring send (tests/send_resident_ref.py) without a GPU: it equals
tx_sock_from + fs_send_rings_layout of the loaded library wherever nothing is deferred or invalid; its
deferred set is the stated suffix at every capacity; two write-back turns equal the host chain through
socks_out; and the batches of the GPU suite (tests/send_resident_cases.py) reach what they name."""
import numpy as np
import pytest

from seqs_amd import abi
from seqs_amd.framesum import send_rings_layout, tx_sock_from

import send_cases as cases
import send_ref as ref
import send_resident_cases as rcases
import send_resident_ref as rref

AMPLE = dict(frames_cap=1 << 31, frames_bytes=1 << 62)


def test_constants_are_the_bindings():
    assert (rref.WRITEBACK, rref.DEFERRED, rref.INVALID, rref.NO_RX) == (abi.TX_WRITEBACK, abi.TX_DEFERRED, abi.TX_INVALID,
                                                                        abi.TX_NO_RX)
    assert rref.ACK_OWED == abi.RECV_ACK_OWED and rref.BAD_ETHERTYPE == abi.TX_BAD_ETHERTYPE == 1
    assert rref.BAD_RING_RANGE == abi.TX_BAD_RING_RANGE == 11 and rref.BAD_RX_INDEX == abi.TX_BAD_RX_INDEX == 12


# ---- 1: the model is tx_sock_from + the layout call where nothing is deferred or invalid ------------------

def host_records(socks, flags, align, so=None, sn=None):
    recs = ref.socks_of(socks)
    if so is not None:
        recs = tx_sock_from(so, recs, snd_out=sn)
    return recs, send_rings_layout(recs, flags, align)


@pytest.mark.parametrize("flags,align", [(0, 1), (ref.FCS_APPEND, 4), (0, 64)])
def test_model_is_the_layout_call(flags, align):
    batches = [(s, r, None, None) for s, r in list(cases.oracle_cases()) + [cases.rejected_frames()]]
    batches += [rcases.rx_records(16), rcases.rx_records(9)[:3] + (None,)]
    for socks, rings, so, sn in batches:
        p = rref.plan(socks, rings.size, flags=flags, align=align, rx_socks_out=so, rx_snd_out=sn, **AMPLE)
        assert set(p["kinds"]) <= {rref.BUILT, rref.IDLE}
        recs, (n, nbytes, outs) = host_records(socks, flags, align, so, sn)
        assert (p["totals"]["n_frames"], p["totals"]["frames_bytes"]) == (n, nbytes)
        assert p["totals"]["n_built"] == int((outs["n_frames"] > 0).sum()) and p["totals"]["data_bytes"] == int(outs["bytes"].sum())
        assert p["totals"]["n_idle"] == len(socks) - p["totals"]["n_built"]
        _, built_outs = ref.frames_of(p["built"], rings)
        assert np.array_equal(rref.socks_out_of(socks, p, built_outs), outs)
        assert np.array_equal(ref.socks_of(p["built"]), recs[p["built_at"]])  # (the hand-off is tx_sock_from)


# ---- 2: the deferred set is the suffix the header states ---------------------------------------------------

def stated_kinds(socks, ends, cap, nbytes):
    first = next((i for i, (s, (F, B)) in enumerate(zip(socks, ends)) if ref.rule(s)["S"] and (F > cap or B > nbytes)),
                 len(socks))
    return [rref.IDLE if ref.rule(s)["S"] == 0 else rref.BUILT if i < first else rref.DEFER for i, s in enumerate(socks)]


@pytest.mark.parametrize("flags,align", [(0, 1), (ref.FCS_APPEND, 64)])
def test_deferred_set_is_the_suffix(flags, align):
    socks, rings = rcases.capacity()
    assert len(socks) == 12
    ends = rcases.frame_ends(socks, flags, align)
    total_f, total_b = ends[-1]
    seen = set()
    for cap in range(0, total_f + 2):
        p = rref.plan(socks, rings.size, cap, 1 << 62, flags, align)
        assert p["kinds"] == stated_kinds(socks, ends, cap, 1 << 62), cap
        built = [e for e, k in zip(ends, p["kinds"]) if k == rref.BUILT]
        assert p["totals"]["n_frames"] == (built[-1][0] if built else 0) <= cap
        seen.add(p["totals"]["n_deferred"])
    assert seen == set(range(0, 10))  # every number of deferred sockets, none to all nine with frames
    for _, B in ends:
        for nbytes in (B - 1, B, B + 1):
            p = rref.plan(socks, rings.size, 1 << 31, nbytes, flags, align)
            assert p["kinds"] == stated_kinds(socks, ends, 1 << 31, nbytes), nbytes
            assert p["totals"]["frames_bytes"] <= nbytes
    # an idle socket behind the cut stays idle; a deferred one's state is unchanged
    p = rref.plan(socks, rings.size, ends[4][0], 1 << 62, flags, align)
    assert p["kinds"][8] == p["kinds"][11] == rref.IDLE and p["kinds"][5] == rref.DEFER and p["after"][5] == socks[5]


# ---- 3: two write-back turns are the host chain through socks_out -------------------------------------------

def host_turn(recs):
    """One turn as a stack on the host-socket call does it (tests/conversation.py): the layout call, then
    socks_out into the records."""
    _, _, outs = send_rings_layout(recs)
    nxt = recs.copy()
    for k in ("snd_nxt", "ring_rpos", "ring_buffered"):
        nxt[k] = outs[k]
    nxt["hdr"][:, 18], nxt["hdr"][:, 19] = outs["ip_id"] >> 8, outs["ip_id"] & 0xFF
    nxt["flags"] &= ~np.where(outs["sent"] == ref.TX_FIN, ref.TX_FIN, 0).astype(np.uint32)
    nxt["flags"] &= ~np.where(outs["n_frames"] > 0, ref.TX_ACK, 0).astype(np.uint32)
    return nxt, outs


def test_two_writeback_turns_are_the_host_chain():
    socks, rings = cases.window_and_flags()
    for s in socks:
        s["max_frames"] = 2
    recs = ref.socks_of(socks)
    table = socks
    for turn in range(2):
        p = rref.plan(table, rings.size, **AMPLE)
        recs, outs = host_turn(recs)
        _, built_outs = ref.frames_of(p["built"], rings)
        assert np.array_equal(rref.socks_out_of(table, p, built_outs), outs), turn
        table = p["after"]
        assert np.array_equal(ref.socks_of(table), recs), turn
    assert not any(s["flags"] & ref.TX_ACK for s in table) and any(s["flags"] & ref.TX_FIN for s in table)


# ---- 4: the GPU suite's batches reach what they name ---------------------------------------------------------

def kinds_of(socks, rings_bytes, **kw):
    return rref.plan(socks, rings_bytes, **{**AMPLE, **kw})["kinds"]


def test_boundary_batches():
    for n in rcases.BOUNDARY_SIZES:
        socks, rings = rcases.boundary(n)
        kinds = kinds_of(socks, rings.size)
        assert len(socks) == n and kinds[-1] == rref.IDLE
        for i in rcases.IDLE_POSITIONS:
            assert i >= n or kinds[i] == rref.IDLE
        assert n < 3 or rref.BUILT in kinds
        quiet, q_rings = rcases.boundary(n, "all")
        assert kinds_of(quiet, q_rings.size) == [rref.IDLE] * n
        alt, a_rings = rcases.boundary(n, "alternate")
        assert kinds_of(alt, a_rings.size) == [rref.IDLE if i % 2 == 0 else rref.BUILT for i in range(n)]


def test_stride_and_ack_batches():
    socks, rings = rcases.id_strides()
    assert [ref.rule(s)["S"] for s in socks] == [x for S in rcases.STRIDE_FRAMES for x in (S, 1)]
    recs, rings = rcases.many_acks(1000)
    _, _, outs = send_rings_layout(recs)
    assert (outs["n_frames"] == 1).all() and (outs["sent"] == ref.TX_ACK).all() and (outs["bytes"] == 0).all()
    assert rcases.dicts_of(recs[:3])[2]["flags"] == ref.TX_ACK and rref.check(rcases.dicts_of(recs[:1])[0], rings.size) == 0


def test_invalid_batches():
    for reason in rcases.invalid_sockets():
        for at in (0, 4, rcases.INVALID_N - 1):
            socks, rings, rings_bytes = rcases.with_invalid(reason, at)
            p = rref.plan(socks, rings_bytes, **AMPLE)
            assert p["reasons"][at] == reason and p["kinds"][at] == rref.BAD and p["kinds"].count(rref.BAD) == 1
            assert p["kinds"][5] in (rref.IDLE, rref.BAD) and p["totals"]["n_built"] >= 6
            assert all(s["ring_off"] + s["ring_size"] <= rings.size for s in socks if s["ring_size"] <= 128)
    assert sorted(rcases.invalid_sockets()) == list(range(1, 12))


def test_hand_off_batches():
    socks, rings, so, sn = rcases.rx_records(16)
    bare = rref.plan(socks, rings.size, **AMPLE)
    assert set(bare["kinds"]) == {rref.IDLE}  # no window room, no ACK: the RX records make every frame
    p = rref.plan(socks, rings.size, rx_socks_out=so, rx_snd_out=sn, **AMPLE)
    b = dict(zip(p["built_at"], p["built"]))
    assert b[0]["rcv_wnd"] == 70000 and b[0]["rcv_nxt"] == 0xFFFFFFFF and b[0]["flags"] & ref.TX_ACK and ref.rule(b[0])["data"]
    assert ref.rule(b[1])["data"] == 0 and ref.rule(b[1])["sent"] == ref.TX_ACK and p["kinds"][3] == rref.IDLE
    assert ref.rule(b[2])["data"] and b[2]["rcv_wnd"] == 65536
    only_rcv = rref.plan(socks, rings.size, rx_socks_out=so, **AMPLE)
    assert set(only_rcv["kinds"]) == {rref.IDLE} and only_rcv["after"][0]["rcv_wnd"] == 70000
    for kind in ("identity", "permuted", "holes", "range"):
        idx = rcases.indices(16, 16, kind)
        q = rref.plan(socks, rings.size, rx_socks_out=so, rx_snd_out=sn, rx_index=idx, **AMPLE)
        assert (q["kinds"] == p["kinds"]) == (kind == "identity")
        assert (rref.BAD_RX_INDEX in q["reasons"]) == (kind == "range") and (rref.NO_RX in idx) == (kind == "holes")
        assert kind != "range" or q["reasons"].count(rref.BAD_RX_INDEX) == 2 and q["reasons"][15] == 0
    assert len(rcases.indices(8, 16, "permuted")) == 8 and rcases.indices(24, 16, "permuted").max() < 16


def test_writeback_turns_batch():
    socks, rings, edits, caps = rcases.writeback_turns()
    table, fins, ids = socks, 0, []
    for turn in range(3):
        for i, f in edits[turn].items():
            table[i] = dict(table[i], **f)
        cap = caps[turn]
        if cap is None:  # one frame short of socket 6's bare ACK
            cap = rcases.frame_ends(table)[6][0] - 1
        p = rref.plan(table, rings.size, cap, 1 << 62)
        fins += sum(ref.rule(s)["fin"] for s in p["built"])
        ids.append(int.from_bytes(table[4]["hdr"][18:20], "big"))
        assert p["kinds"][6] == (rref.IDLE, rref.DEFER, rref.BUILT)[turn] and p["kinds"][4] == rref.BUILT
        assert p["kinds"][2] == (rref.BUILT if turn == 0 else rref.IDLE)
        table = p["after"]
        assert bool(table[6]["flags"] & ref.TX_ACK) == (turn == 1)
    assert fins == 1 and len(set(ids)) == 3 and not table[1]["flags"] and table[1]["ring_buffered"] == 0
