"""The batches of tests/close_cases.py reach what they name, shown with tests/close_ref.py alone (no GPU):
every transition and every code at every position on both sides of the chunk boundaries, several events
inside one chunk, the 64 FINs of the hostile flow, the continuations of the Established sockets, the closer
whose flow opens with a SYN to a listener, the header geometries, and the two big shapes."""
import numpy as np
import pytest

import close_cases as cases
import close_ref as ref
import flows_ref as fref
import recv_ref

M32 = ref.M32


def expected(case, lead=0):
    buf, off, ln = fref.pack(case.frames, lead=lead)
    e = ref.expected(buf, off, ln, 0, 0, np.zeros(8, np.uint8), 0, 0, case.socks, case.snd, np.zeros(case.rings_bytes, np.uint8),
                     case.listeners, case.slots, 0, np.zeros(len(case.slots) * 64, np.uint8), case.closers)
    return e, [bytes(buf[int(o) : int(o) + int(l)]) for o, l in zip(off, ln)]


def flow_codes(e, frames, key):
    """The ctl codes of the flow `key`, in delivery order."""
    for fl in e["flows"]:
        first, count = int(fl["first_frame"]), int(fl["n_frames"])
        idx = [int(e["order"][k]) for k in range(first, first + count)]
        if fref.flow_key(frames[idx[0]]) == key:
            return [int(e["ctl_code"][i]) for i in idx], first
    raise AssertionError("no such flow")


@pytest.mark.parametrize("n", [130, 258])
@pytest.mark.parametrize("which", range(len(cases.TRANSITIONS)))
def test_event_at_positions(n, which):
    case = cases.event_at_positions(n, which)
    state, event, after = cases.TRANSITIONS[which]
    e, frames = expected(case)
    assert len(case.closers) == len(case.info["positions"]) == (8 if n == 130 else 11)
    crossed = 0
    for c, out, trace, p in zip(case.closers, e["closers_out"], case.info["traces"], case.info["positions"]):
        codes, first = flow_codes(e, frames, bytes(c["key"]))
        assert len(codes) == n and trace[:p] == [(state, k) for k in codes[:p]] and not any(k in (0, 8, 9) for k in codes[:p])
        if event in ("syn", "syn_ack"):
            assert codes[p:] == [0] * (n - p) and int(out["stop"]) == first + p and int(out["state"]) == state
            continue
        assert codes[p] == (9 if event.startswith("rst") else 1) and int(out["stop"]) == first + n
        final = after if after in (0, 8) else int(out["state"])
        assert int(out["state"]) == final and (after not in (0, 8) or codes[p + 1 :] == [8] * (n - p - 1))
        assert trace[p][0] == state and (p + 1 == n or trace[p + 1][0] == after)
        # the event's flags
        want = {5: ref.ACK_OWED, 6: ref.ACK_OWED}.get(state, 0) if not event.startswith("rst") else ref.RESET
        assert int(out["flags"]) & (ref.ACK_OWED | ref.RESET) == want
        assert bool(int(out["flags"]) & ref.FIN_TAKEN) == event.startswith("fin") or after == 9
        crossed += int(c["rcv_nxt"]) > M32 - 300
    assert event.startswith("syn") or crossed >= 3  # Seq across 2^32


@pytest.mark.parametrize("n", [130, 258])
def test_codes_at_positions(n):
    case = cases.codes_at_positions(n)
    e, frames = expected(case)
    for c, (state, _, code) in zip(case.closers, cases.CODES):
        codes, _ = flow_codes(e, frames, bytes(c["key"]))
        assert [codes[p] for p in case.info["positions"]] == [code] * len(case.info["positions"]), (state, code)
    assert set(int(x) for x in e["ctl_code"]) >= {1, 4, 5, 7, 8, 10}
    assert (e["closers_out"]["rcv_nxt"][:3] > M32 - 50).all()  # Seq near 2^32


def test_several_events():
    case = cases.several_events()
    e, frames = expected(case)
    out = e["closers_out"]
    codes = [flow_codes(e, frames, bytes(c["key"]))[0] for c in case.closers]
    assert [int(x) for x in out["state"]] == [8, 8, 0, 0, 0, 6]
    assert codes[0][3] == 1 and codes[0][10] == 1 and codes[0][11:] == [8] * 59 and int(out["n_taken"][0]) == 2
    assert codes[1][:3] == [1, 1, 8]
    assert codes[2][5:7] == [1, 1] and codes[2][20] == 9 and codes[2][21:] == [8] * 49
    assert codes[3][62:66] == [1, 1, 1, 9] and int(out["flags"][3]) == ref.FIN_TAKEN | ref.RESET
    assert codes[4][63] == 1 and codes[4][64:] == [8] * 6
    first = flow_codes(e, frames, bytes(case.closers["key"][5]))[1]
    assert codes[5][8:] == [0] * 62 and int(out["stop"][5]) == first + 8 and int(out["flags"][5]) == ref.ACK_OWED


def test_hostile():
    case = cases.hostile()
    e, frames = expected(case)
    out = e["closers_out"]
    assert [int(x) for x in out["n_taken"]] == [64, 130, 5] and (out["state"] == 9).all() and (out["flags"] == ref.FIN_TAKEN).all()
    assert int(out["rcv_nxt"][0]) == (M32 - 30 + 64) % M32 == 34 and int(case.closers["rcv_wnd"][2]) == 0


def test_geometries():
    case = cases.geometries()
    e, frames = expected(case, lead=3)
    seen = {(f[14] & 15, f[14 + 4 * (f[14] & 15) + 12] >> 4) for f in frames}
    assert seen == {(a, b) for a in (5, 6, 15) for b in (5, 6, 15)} and not e["st"].any()
    assert (e["closers_out"]["state"] == 8).all() and (e["closers_out"]["n_taken"] == 2).all()


def test_established():
    case = cases.established()
    e, frames = expected(case)
    sc, so = e["socks_close"], e["socks_out"]
    by = dict(zip(case.info["names"], range(len(sc))))
    for name, p in (("fin at 63", 63), ("fin at 64", 64)):
        s = by[name]
        first = int(e["flows"][int(so["flow"][s])]["first_frame"])
        assert int(so["stop"][s]) == first + p + 1 and int(e["snd_out"]["flags"][s]) & recv_ref.FIN_SEEN
        codes = flow_codes(e, frames, bytes(case.socks["key"][s]))[0]
        assert codes[: p + 1] == [0] * (p + 1) and sorted(set(codes[p + 1 :])) == [1, 4, 5, 7]
        assert int(sc["state"][s]) == 9 and int(sc["flags"][s]) == ref.FIN_TAKEN and int(sc["stop"][s]) == first + p + 21
        assert int(sc["rcv_nxt"][s]) == (int(so["rcv_nxt"][s]) + 1) % M32
    s = by["rst passes"]
    assert [int(x) for x in sc[s]][:4] == [0, 0, 0, 0] and int(sc["flags"][s]) == ref.RESET
    assert flow_codes(e, frames, bytes(case.socks["key"][s]))[0] == [0, 0, 9, 8, 8, 8]  # TimeWait and Closed ignore a SYN too
    s = by["rst fails"]
    assert int(sc["state"][s]) == 4 and int(sc["n_rejected"][s]) == 1 and int(sc["stop"][s]) == int(so["stop"][s]) + 1
    assert flow_codes(e, frames, bytes(case.socks["key"][s]))[0] == [0, 4, 0, 0] and int(so["bytes"][s]) == 0
    s = by["rst with data"]
    assert int(sc["state"][s]) == 4 and flow_codes(e, frames, bytes(case.socks["key"][s]))[0] == [0, 7, 0]
    s = by["syn at stop"]
    assert int(sc["state"][s]) == 4 and int(sc["stop"][s]) == int(so["stop"][s]) and not any(flow_codes(e, frames, bytes(case.socks["key"][s]))[0])
    s = by["rst first"]
    assert int(sc["state"][s]) == 0 and flow_codes(e, frames, bytes(case.socks["key"][s]))[0] == [9, 8]
    s = by["no flow"]
    assert int(sc["state"][s]) == 4 and int(sc["stop"][s]) == ref.NONE and int(sc["rcv_nxt"][s]) == int(case.socks["rcv_nxt"][s])
    assert [int(x) for x in e["closers_out"]["state"]] == [8, 9]


def test_closer_and_listener():
    case = cases.closer_and_listener()
    e, frames = expected(case)
    assert int(e["listeners_out"]["n_syn"][0]) == 3 and int(e["conns"]["used"].sum()) == 3
    out = e["closers_out"]
    firsts = [flow_codes(e, frames, bytes(c["key"]))[1] for c in case.closers]
    assert [int(x) for x in out["stop"][:2]] == firsts[:2] and (out["n_taken"] == 0).all()
    assert flow_codes(e, frames, bytes(case.closers["key"][2]))[0] == [8] * 5 and int(out["stop"][2]) == firsts[2] + 5


@pytest.mark.parametrize("shape", cases.BIG_SHAPES)
def test_big(shape):
    case = cases.big(shape)
    assert len(case.frames) == cases.BIG
    e, _ = expected(case)
    out = e["closers_out"]
    if shape == "65536 closers":
        assert len(out) == 65536 and (out["state"] == 8).all() and (out["n_taken"] == 1).all() and e["n_flows"] == cases.BIG
        assert int((e["ctl_code"] == 1).sum()) == 65536
    else:
        assert len(out) == 1000 and (out["state"] == 9).all() and (out["flags"] == ref.FIN_TAKEN).all()
        assert (e["socks_close"]["state"] == 9).all() and len(e["socks_close"]) == 64
