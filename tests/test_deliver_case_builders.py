"""The builders of tests/deliver_cases.py run through tests/deliver_ref.py alone (no GPU): each batch
reaches the lanes, chunks, events, splits and sizes it names, without which tests/test_gpu_deliver_edges.py
would pass because its input missed the case. Every check is an equality on the reference's output.
deliver_ref.walk itself is checked against closed forms on the all-in-order flows."""
import collections
import functools

import numpy as np
import pytest

import deliver_cases as dc
import deliver_ref as ref
import flows_ref as fref

M32 = 1 << 32


@functools.lru_cache(maxsize=None)
def expected(builder, *args):
    return dc.reference(getattr(dc, builder)(*args))


def outs(e, s):
    o = e["socks_out"][s]
    return {k: int(o[k]) for k in o.dtype.names}


def first_frame(e, s):
    return int(e["flows"]["first_frame"][int(e["socks_out"]["flow"][s])])


def slot_marks(e, s, count):
    """The `delivered` marks of socket s's flow, slot by slot from its first."""
    first = first_frame(e, s)
    return e["delivered"][e["order"][first : first + count]]


def outside_writes_hold_the_sentinel(case, e, seed=0):
    """Every ring byte outside an admitted write is the sentinel's: the writes of each socket are the
    `bytes` bytes before its final wpos."""
    from test_gpu_deliver import sentinel

    untouched = np.ones(case.rings_bytes, dtype=bool)
    for sk, o in zip(case.socks, e["socks_out"]):
        size, lo = int(sk["ring_size"]), int(sk["ring_off"])
        at = (int(sk["ring_wpos"]) + np.arange(int(o["bytes"]))) % size
        assert (int(sk["ring_wpos"]) + int(o["bytes"])) % size == int(o["ring_wpos"])
        untouched[lo + at] = False
    assert np.array_equal(e["rings"][untouched], sentinel(case.rings_bytes, seed)[untouched])
    return int((~untouched).sum())


# ---- a. ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("interleaved", [False, True])
def test_flows_end_at_every_lane(oracle_lib, interleaved):
    case, e = dc.flow_ends_at_every_lane(interleaved), expected("flow_ends_at_every_lane", interleaved)
    lengths = case.info["lengths"]
    assert len(lengths) == 69 == case.socks.size == e["n_flows"] and {192, 256, 257, 1, 2, 64} <= set(lengths)
    ends = [outs(e, s)["stop"] - first_frame(e, s) for s in range(69)]
    assert ends == lengths and [outs(e, s)["flow"] for s in range(69)] == list(range(69))
    long = [x for x in ends if x >= 192]
    assert {x % 64 for x in long} == set(range(64)) and {x // 64 for x in long} == {3, 4}
    assert all(outs(e, s)["n_dropped"] == 1 and outs(e, s)["n_delivered"] == lengths[s] - 1 for s in range(69))
    # every flow but the first starts behind another flow's last slot, at a varying lane of that flow's chunk
    firsts = [first_frame(e, s) for s in range(69)]
    assert firsts == [sum(lengths[:s]) for s in range(69)] and len({f % 64 for f in firsts}) > 32
    if interleaved:
        assert not np.array_equal(e["order"], np.arange(e["n_accepted"])) and list(e["order"][:3]) == [0, 69, 137]  # (the one-frame flow drops out of the second round)
    else:
        assert np.array_equal(e["order"], np.arange(e["n_accepted"]))
    for s in range(69):
        assert list(slot_marks(e, s, lengths[s])) == [1] * (lengths[s] - 1) + [2]
    assert outside_writes_hold_the_sentinel(case, e) == 10 * (sum(lengths) - 69)


# ---- b. ------------------------------------------------------------------------------------------

def test_every_event_at_every_position(oracle_lib):
    case, e = dc.events_at_chunk_positions(), expected("events_at_chunk_positions")
    pairs, n = case.info["pairs"], dc.EVENT_FLOW
    assert len(pairs) == 80 == case.socks.size and e["n_flows"] == 160 and e["n_accepted"] == 80 * 367 == (e["st"] == 0).sum()
    for s, (ev, p) in enumerate(pairs):
        o, m = outs(e, s), [int(x) for x in slot_marks(e, s, n)]
        first = first_frame(e, s)
        assert first == 37 + 367 * s and o["flow"] == 2 * s + 1
        if ev == "fin":
            assert o["stop"] - first == p + 1 and m == [1] * (p + 1) + [0] * (n - p - 1) and o["n_delivered"] == p + 1
            # ... and the frame behind it carries the Seq the socket now expects
            if p + 1 < n:
                i = int(e["order"][first + p + 1])
                buf, off, _ = case.batch
                assert int.from_bytes(buf[int(off[i]) + 38 : int(off[i]) + 42].tobytes(), "big") == o["rcv_nxt"]
        elif ev in ("syn", "rst"):
            assert o["stop"] - first == p and m == [1] * p + [0] * (n - p) and o["n_dropped"] == 0
        else:
            assert o["stop"] - first == n and m == [1] * p + [2] + [1] * (n - p - 1)
            assert (o["n_delivered"], o["n_dropped"], o["bytes"]) == (n - 1, 1, 10 * (n - 1))
    # the flows without a socket are untouched
    assert int((e["delivered"] != 0).sum()) == sum(int(x) for x in e["socks_out"]["n_delivered"] + e["socks_out"]["n_dropped"])
    outside_writes_hold_the_sentinel(case, e)


# ---- c. ------------------------------------------------------------------------------------------

def test_restart_patterns(oracle_lib):
    case, e = dc.restart_patterns(), expected("restart_patterns")
    assert (e["st"] == 0).all() and e["n_flows"] == 3
    for s, name in enumerate(dc.PATTERNS):
        m = slot_marks(e, s, dc.PATTERN_FLOW)
        assert first_frame(e, s) == 200 * s and outs(e, s)["stop"] == 200 * (s + 1)
        chunks = [m[c : c + 64] for c in range(0, 200, 64)]
        assert [int((c == 2).sum()) for c in chunks] == dc.PATTERN_DROPS[name], name
        assert [int((c == 1).sum()) for c in chunks] == dc.PATTERN_ADMITTED[name], name
    m = slot_marks(e, 2, 200)
    assert list(np.flatnonzero(m == 2)) == [63, 64, 127, 128, 129]
    assert list(slot_marks(e, 1, 6)) == [1, 2, 1, 2, 1, 2] and outs(e, 0)["n_dropped"] == 200 and outs(e, 0)["bytes"] == 0
    outside_writes_hold_the_sentinel(case, e)


# ---- d. and e. -----------------------------------------------------------------------------------

def splits_of(case, e):
    out = []
    for sk, o in zip(case.socks, e["socks_out"]):
        if int(o["n_delivered"]) == 1:
            out.append((int(o["bytes"]), min(int(o["bytes"]), int(sk["ring_size"]) - int(sk["ring_wpos"]))))
    return out


def test_small_wrap_splits(oracle_lib):
    case, e = dc.wrap_splits_small(), expected("wrap_splits_small")
    assert case.socks.size == 860 and (e["delivered"] == 1).all() and (e["socks_out"]["n_delivered"] == 1).all()
    assert collections.Counter(splits_of(case, e)) == collections.Counter(case.info["splits"])
    assert {(n, f) for n, f in case.info["splits"]} == {(n, f) for n in range(1, 41) for f in range(1, n + 1)}
    assert {int(x) for x in (case.socks["ring_off"] + case.socks["ring_wpos"]) % 16} == set(range(16))
    buf, off, ln = case.batch
    assert {int(x) for x in (off + np.uint64(54)) % np.uint64(16)} == set(range(16))
    sizes = collections.defaultdict(set)
    for sk, o in zip(case.socks, e["socks_out"]):
        sizes[int(o["bytes"])].add(int(sk["ring_size"]))
    assert all(sizes[n] == {n, n + 1, 97, 4099} for n in range(3, 41))  # (lengths 1 and 2 have 2 and 3 placements)
    assert sizes[1] == {1, 2} and sizes[2] == {2, 97, 4099}  # (a ring of one byte among them)
    lo = np.sort(case.socks["ring_off"].astype(np.int64))
    end = np.sort((case.socks["ring_off"] + case.socks["ring_size"]).astype(np.int64))
    assert set((lo[1:] - end[:-1]).tolist()) == {0, 1}
    assert outside_writes_hold_the_sentinel(case, e) == sum(n for n, _ in dc.SMALL_SPLITS)


def test_large_wrap_splits(oracle_lib):
    case, e = dc.wrap_splits_large(), expected("wrap_splits_large")
    assert case.socks.size == 227 and (e["st"] == 0).all() and len(case.info["splits"]) == 224
    assert (e["socks_out"]["n_delivered"][:224] == 1).all()
    got = collections.Counter(splits_of(case, e)[:224])
    want = collections.Counter((n, n if f == 0 else f) for n in dc.LARGE_LENGTHS for f in dc.large_firsts(n) for _ in range(4))
    assert got == want == collections.Counter(case.info["splits"]) and sum(want.values()) == 224
    assert {int(x) % 16 for x in case.socks["ring_off"][:224]} == set(dc.RING_RESIDUES)
    # the jumbo flow: 40 admitted, 24 dropped, the ring wrapped once
    j, o = case.info["jumbo_sock"], outs(e, case.info["jumbo_sock"])
    assert list(slot_marks(e, j, 64)) == [1] * 40 + [2] * 24 and o["bytes"] == 40 * dc.JUMBO and o["ring_free"] == 100
    assert o["rcv_nxt"] == 20 * dc.JUMBO and o["stop"] - first_frame(e, j) == 64 and 64 * dc.JUMBO > 4190000
    # the jumbo FIN: above a window of its length, inside a window one larger
    assert [outs(e, s)["n_delivered"] for s in (225, 226)] == [0, 1] and [outs(e, s)["n_dropped"] for s in (225, 226)] == [1, 0]
    assert outs(e, 226)["rcv_nxt"] == (int(case.socks["rcv_nxt"][226]) + dc.JUMBO + 1) % M32
    outside_writes_hold_the_sentinel(case, e)


# ---- f. ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fcs", [False, True])
def test_header_geometries(oracle_lib, fcs):
    case = dc.header_case(fcs, 5)
    e = dc.reference(case)
    assert list(e["st"]) == [0] * 122 and list(e["delivered"]) == [1] * 122 and e["n_flows"] == 1
    buf, off, ln = case.batch
    geo = [(int(buf[int(o) + 14]) & 15, int(buf[int(o) + 14 + 4 * (int(buf[int(o) + 14]) & 15) + 12]) >> 4) for o in off]
    assert geo[:121] == [(i, d) for i in range(5, 16) for d in range(5, 16)] and geo[121] == (15, 15)
    assert outs(e, 0) == dict(rcv_nxt=(M32 - 3000 + 7381 + 1) % M32, ring_wpos=(7381 - 500 + 7381) % 7421, ring_free=40,
                              bytes=7381, n_delivered=122, n_dropped=0, flow=0, stop=122)
    # the same result at every lead: the GPU test computes it once
    other = dc.reference(dc.header_case(fcs, 11))
    assert other["socks_out"].tobytes() == e["socks_out"].tobytes() and np.array_equal(other["rings"], e["rings"])
    assert np.array_equal(other["dig"], e["dig"]) and other["runs"].tobytes() == e["runs"].tobytes()


# ---- g. ------------------------------------------------------------------------------------------

def test_near_miss_keys(oracle_lib):
    case, e = dc.near_miss_keys(), expected("near_miss_keys")
    assert e["n_flows"] == 16 and list(e["st"][[27, 28, 30]]) == [13, 13, 13] and int((e["st"] != 0).sum()) == 3
    assert [outs(e, s)["flow"] for s in range(3)] == [15, 14, ref.NONE]
    assert outs(e, 2) == dict(rcv_nxt=100, ring_wpos=5, ring_free=32, bytes=0, n_delivered=0, n_dropped=0, flow=ref.NONE,
                              stop=ref.NONE)
    assert outs(e, 0)["bytes"] == 63 and outs(e, 1)["bytes"] == 63 and outs(e, 1)["n_delivered"] == 2
    assert int(e["order"][first_frame(e, 1)]) == 29  # the damaged-head flow starts with its second frame
    assert list(np.flatnonzero(e["delivered"])) == [29, 31, 32, 33, 34]
    # each of the 13 near flows differs from the socket's key in exactly one bit; the UDP flow in the protocol alone
    buf, off, ln = case.batch
    key = bytes(case.socks["key"][0])
    bits = []
    for f in range(14):
        i = int(e["order"][int(e["flows"]["first_frame"][f])])
        k = fref.flow_key(buf[int(off[i]) : int(off[i]) + int(ln[i])].tobytes())
        diff = [(at, a ^ b) for at, (a, b) in enumerate(zip(k, key)) if a != b]
        assert len(diff) == 1 and bin(diff[0][1]).count("1") == (1 if f < 13 else 4)  # (6 ^ 17 has four bits)
        bits.append(diff[0])
    assert [at for at, _ in bits] == [*range(1, 13), 12, 0] and len(set(bits)) == 14
    outside_writes_hold_the_sentinel(case, e)


# ---- h. ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["one flow", "1000 flows", "every frame its own flow"])
def test_big_batches(oracle_lib, shape):
    from test_gpu_flows import BIG

    case, e = dc.big_batches(shape), expected("big_batches", shape)
    so = e["socks_out"]
    assert BIG > 65536 and e["n_accepted"] == BIG and (e["st"] == 0).all()
    if shape == "one flow":
        assert outs(e, 0) == dict(rcv_nxt=(int(case.socks["rcv_nxt"][0]) + 10 * BIG) % M32, ring_wpos=(699990 + 10 * BIG) % 700001,
                                  ring_free=700001 - 10 * BIG, bytes=10 * BIG, n_delivered=BIG, n_dropped=0, flow=0, stop=BIG)
        assert (e["delivered"] == 1).all()
    elif shape == "1000 flows":
        flow_of = case.info["flow_of"]
        count = np.bincount(flow_of, minlength=1000)[flow_of[:1000]]  # flow f opens with frame f
        assert sorted(flow_of[:1000].tolist()) == list(range(1000))
        assert list(so["flow"]) == list(range(999, -1, -1)) and np.array_equal(so["n_delivered"][::-1], count)
        assert int(so["bytes"].sum()) == 10 * BIG and (e["delivered"] == 1).all() and (so["ring_free"] == 3).all()
    else:
        assert case.socks.size == 65536 and np.array_equal(so["flow"], np.arange(65536)) and (so["bytes"] == 10).all()
        assert np.array_equal(so["stop"], np.arange(1, 65537)) and e["n_flows"] == BIG
        assert np.array_equal(e["delivered"], (np.arange(BIG) < 65536).astype(np.uint8))
        assert np.array_equal(so["ring_wpos"], (np.arange(65536) % 16 + 10) % 16)
    outside_writes_hold_the_sentinel(case, e)


# ---- the reference against closed forms ----------------------------------------------------------

def in_order_closed_form(sk, lens):
    """An all-in-order flow of payloads `lens` into a ring with `free` bytes: the frames are admitted
    while they fit, a frame that does not fit is dropped and so is every later one (its Seq is ahead)."""
    free, taken, marks, stuck = int(sk["ring_free"]), 0, [], False
    for n in lens:
        ok = not stuck and n <= free - taken
        stuck, taken = stuck or not ok, taken + (n if ok else 0)
        marks.append(1 if ok else 2)
    return dict(bytes=taken, rcv_nxt=(int(sk["rcv_nxt"]) + taken) % M32, ring_free=free - taken,
                ring_wpos=(int(sk["ring_wpos"]) + taken) % int(sk["ring_size"]), marks=marks)


def test_walk_agrees_with_the_closed_form(oracle_lib):
    from test_gpu_flows import BIG

    a, ea = dc.flow_ends_at_every_lane(), expected("flow_ends_at_every_lane")
    todo = [(a.socks[s], [10] * n, ea, s) for s, n in enumerate(a.info["lengths"])]
    todo.append((dc.big_batches("one flow").socks[0], [10] * BIG, expected("big_batches", "one flow"), 0))
    big = dc.wrap_splits_large()
    todo.append((big.socks[big.info["jumbo_sock"]], [dc.JUMBO] * 64, expected("wrap_splits_large"), big.info["jumbo_sock"]))
    for sk, lens, e, s in todo:
        want, o = in_order_closed_form(sk, lens), outs(e, s)
        assert {k: o[k] for k in ("bytes", "rcv_nxt", "ring_free", "ring_wpos")} == {k: want[k] for k in want if k != "marks"}
        assert [int(x) for x in slot_marks(e, s, len(lens))] == want["marks"]


def test_chained_calls_fill_every_ring_several_times(oracle_lib):
    rings0, calls = dc.chained_calls()
    assert len(calls) == 40 > 32 and [int(c[0][2].size) for c in calls[:4]] == [5, 300, 5, 300]
    taken = sum(c[2]["socks_out"]["bytes"][:3].astype(np.int64) for c in calls)
    assert (taken >= 3 * calls[0][1]["ring_size"]).all() and {c[1].size for c in calls} == {3, 153}
    assert all((c[2]["socks_out"]["n_dropped"] == 0).all() and (c[2]["delivered"] == 1).all() for c in calls)
    assert all((c[2]["socks_out"]["flow"][3:] == ref.NONE).all() for c in calls)
    for (_, socks, e), (_, nxt, _) in zip(calls, calls[1:]):
        so, nxt = e["socks_out"][:3], nxt[:3]
        assert np.array_equal(nxt["rcv_nxt"], so["rcv_nxt"]) and np.array_equal(nxt["ring_wpos"], so["ring_wpos"])
        assert np.array_equal(nxt["ring_free"], nxt["ring_size"])
    assert np.array_equal(calls[-1][2]["rings"][-1355:], rings0[-1355:])  # the idle sockets' rings keep the sentinel
