"""The batches of tests/connect_cases.py reach what they name, shown with tests/connect_ref.py alone (no GPU):
every rule at every position on both sides of the chunk boundaries with frames behind the walk's end left
alone, two events in one chunk and across a boundary, the extremes of ISS, Seq, Window and rcv_wnd, the SYN
of a flagged opener, the header geometries with the MSS kinds, the opener whose flow opens with a SYN to a
listener, openers beside sockets, closers and listeners, the three keyed lists with a long flow each, the near
keys, and the two big shapes."""
import numpy as np
import pytest

import connect_cases as cases
import connect_ref as ref
import flows_ref as fref
import recv_ref

M32 = ref.M32


def expected(case, lead=0, reply_flags=None, mtu=0):
    buf, off, ln = fref.pack(case.frames, lead=lead)
    e = ref.expected(buf, off, ln, mtu, 0, np.zeros(8, np.uint8), 0, 0, case.socks, case.snd, np.zeros(case.rings_bytes, np.uint8),
                     case.listeners, case.slots, 0, np.zeros(len(case.slots) * 64, np.uint8), case.closers, case.openers,
                     case.reply_flags if reply_flags is None else reply_flags, np.zeros(len(case.openers) * 64, np.uint8))
    return e, [bytes(buf[int(o) : int(o) + int(l)]) for o, l in zip(off, ln)]


def flow_codes(e, frames, key):
    """The ctl codes of the flow `key`, in delivery order, its first slot and its frames' batch indices."""
    for fl in e["flows"]:
        first, count = int(fl["first_frame"]), int(fl["n_frames"])
        idx = [int(e["order"][k]) for k in range(first, first + count)]
        if fref.flow_key(frames[idx[0]]) == key:
            return [int(e["ctl_code"][i]) for i in idx], first, idx
    raise AssertionError("no such flow")


def check_traces(case, e, frames):
    """Every opener's codes are its script's trace; the frames from the walk's end on keep code 0."""
    for o, out, trace in zip(case.openers, e["openers_out"], case.info["traces"]):
        if not trace:
            continue
        codes, first, _ = flow_codes(e, frames, bytes(o["key"]))
        assert codes == [k or 0 for k in trace]
        handled = sum(k is not None for k in trace)
        assert int(out["stop"]) == first + handled
        assert int(out["n_rejected"]) == sum(k in (4, 10) for k in trace) and int(out["n_keepalive"]) == trace.count(5)


@pytest.mark.parametrize("n", [130, 258])
@pytest.mark.parametrize("which", range(len(cases.RULES)))
def test_rule_at_positions(n, which):
    case = cases.rule_at_positions(n, which)
    rule, kind, what = cases.RULES[which]
    e, frames = expected(case)
    assert len(case.openers) == len(case.info["positions"]) == (8 if n == 130 else 11)
    check_traces(case, e, frames)
    for j, (o, out, trace, p) in enumerate(zip(case.openers, e["openers_out"], case.info["traces"], case.info["positions"])):
        codes, first, idx = flow_codes(e, frames, bytes(o["key"]))
        assert len(codes) == n and set(codes[:p]) <= {4, 5, 10} and (p < 3 or set(codes[:p]) == {4, 5, 10})
        iss = int(o["iss"])
        if what in ("rst", "syn"):
            assert codes[p:] == [0] * (n - p) and int(out["stop"]) == first + p and int(out["state"]) == 3
            assert int(out["flags"]) == (ref.STOP_RST if what == "rst" else ref.STOP_SYN) and int(out["frame"]) == ref.NONE
            assert int(out["reply"]) == (ref.REPLY_SYN if int(o["flags"]) else 0)
        elif what in (1, 11):
            assert codes[p] == what and codes[p + 1 :] == [0] * (n - p - 1) and int(out["stop"]) == first + p + 1
            assert int(out["frame"]) == idx[p] and int(out["flags"]) == 0
            seq, ack, window, flags9, _ = recv_ref.fields(frames[idx[p]])
            assert int(out["snd_wnd"]) == window
            if what == 11:
                assert (int(out["state"]), int(out["reply"]), int(out["rst_seq"])) == (3, ref.REPLY_RST, ack) and ack != (iss + 1) % M32
                assert int(out["snd_una"]) == int(out["snd_nxt"]) == iss
            else:
                assert int(out["irs"]) == seq and int(out["rcv_nxt"]) == (seq + 1) % M32
                assert (int(out["state"]), int(out["reply"])) == ((4, ref.REPLY_ACK) if rule == 7 else (2, ref.REPLY_SYNACK))
                assert j % 2 == 0 or (iss == M32 - 1 and seq == M32 - 1 and int(out["rcv_nxt"]) == 0)
        else:
            # a frame that ends no walk: at p and as the flow's last frame; the SYN-ACK behind p + 2 ends the walk
            assert codes[p] == what and codes[n - 1] in (what, 0)
            taken = [k for k, c in enumerate(codes) if c == 1]
            assert (taken == [p + 2] and int(out["state"]) == 4) if p + 2 < n - 1 else (taken == [] and codes[n - 1] == what)
            if not taken:
                assert int(out["stop"]) == first + n and int(out["state"]) == 3
    # a SYN-ACK lies behind every walk that an event ended, and none of them is taken
    if what in ("rst", "syn", 11):
        assert (e["openers_out"]["state"] == 3).all() and not (e["ctl_code"] == 1).any()
        assert sum(recv_ref.fields(f)[3] == ref.SYN | ref.ACK and recv_ref.fields(f)[4] == 0 for f in frames) >= len(case.openers)


def test_two_events():
    case = cases.two_events()
    e, frames = expected(case)
    check_traces(case, e, frames)
    out = e["openers_out"]
    assert [int(x) for x in out["state"]] == [4, 2, 3, 4, 3, 3, 4]
    assert [int(x) for x in out["reply"]] == [ref.REPLY_ACK, ref.REPLY_SYNACK, ref.REPLY_RST, ref.REPLY_ACK, ref.REPLY_SYN, 0, ref.REPLY_ACK]
    assert [int(x) for x in out["flags"]] == [0, 0, 0, 0, ref.STOP_RST, ref.STOP_SYN, 0]
    assert int((e["ctl_code"] == 1).sum()) == 4 and int((e["ctl_code"] == 11).sum()) == 1


def test_extremes():
    case = cases.extremes()
    e, frames = expected(case)
    check_traces(case, e, frames)
    out, ops = e["openers_out"], case.openers
    events = out["frame"] != ref.NONE
    assert {int(x) for x in ops["iss"][events]} == {M32 - 1, 0, 1 << 31} and {int(x) for x in out["irs"][events]} == {M32 - 1, 0}
    assert {int(x) for x in out["snd_wnd"][events]} == {0, 1, 65535} and {int(x) for x in ops["rcv_wnd"][events]} == {0, 1, 65536, M32 - 1}
    assert {int(x) for x in out["state"][events]} == {2, 4}
    # the reply's Window field is the clamped rcv_wnd
    for i in np.flatnonzero(events):
        fr = bytes(e["replies"][i * 64 : i * 64 + 54])
        assert int.from_bytes(fr[48:50], "big") == min(int(ops["rcv_wnd"][i]), 65535)
    # the six data frames: refused at rcv_wnd 0 and where Last leaves the window, expected-SYN where they fit
    assert [t[0] for t in case.info["traces"][-6:]] == [4, 10, 4, 10, 4, 4]


def test_send_syn():
    case = cases.send_syn()
    e, frames = expected(case)
    check_traces(case, e, frames)
    out = e["openers_out"]
    assert [int(x) for x in out["reply"]] == case.info["replies"]
    assert int(out["stop"][0]) == ref.NONE and int(out["snd_wnd"][0]) == 1 and int(out["n_rejected"][1]) + int(out["n_keepalive"][1]) == 9
    syn = bytes(e["replies"][0:54])
    assert syn[47] == ref.SYN and int.from_bytes(syn[38:42], "big") == 100 and syn[42:46] == bytes(4)
    assert not e["replies"][5 * 64 : 6 * 64].any() and int(e["reply_status"][5]) == 0
    # with FS_FCS_APPEND the 58 bytes end in the frame's CRC
    e2, _ = expected(case, reply_flags=2)
    import zlib

    fr = bytes(e2["replies"][0:58])
    assert fr[:54] == syn and int.from_bytes(fr[54:58], "little") == zlib.crc32(syn) == int(e2["reply_out"]["crc32"][0])


def test_geometries():
    case = cases.geometries()
    e, frames = expected(case, lead=3)
    check_traces(case, e, frames)
    assert [int(x) for x in e["openers_out"]["peer_mss"]] == case.info["mss"] and {0, 0x0218, 0x2328} == set(case.info["mss"])
    assert [int(x) for x in e["openers_out"]["state"]] == [2 if j % 2 else 4 for j in range(len(case.openers))]


def test_opener_and_listener():
    case = cases.opener_and_listener()
    e, frames = expected(case)
    check_traces(case, e, frames)
    assert int(e["conns"]["used"].sum()) == 3 and (e["openers_out"]["state"] == 2).all()
    assert (e["openers_out"]["peer_mss"] == 1460).all() and (e["openers_out"]["reply"] == ref.REPLY_SYNACK).all()


def test_mixed():
    case = cases.mixed()
    e, frames = expected(case)
    check_traces(case, e, frames)
    assert [int(x) for x in e["openers_out"]["state"]] == [4, 2, 3, 3] and len(case.socks) and len(case.closers) and len(case.listeners)
    # the close call's codes are where they were, and this call's lie in the openers' flows only
    mine = e["ctl_code"] != e["close_ctl_code"]
    assert mine.any() and not e["close_ctl_code"][mine].any() and e["close_ctl_code"].any()


def test_three_lists():
    case = cases.three_lists()
    e, frames = expected(case)
    check_traces(case, e, frames)
    assert (len(case.socks), len(case.closers), len(case.openers)) == (2, 2, 2)
    assert e["n_flows"] == 8 and e["n_accepted"] == len(frames) == 211
    sizes = {fref.flow_key(frames[int(e["order"][int(fl["first_frame"])])]): int(fl["n_frames"]) for fl in e["flows"]}
    for lst in (case.socks, case.closers, case.openers):  # the first of each list walks past a chunk boundary
        assert sizes[bytes(lst["key"][0])] == 66 and sizes[bytes(lst["key"][1])] == 3
    listed = {bytes(k) for lst in (case.socks, case.closers, case.openers) for k in lst["key"]}
    assert sorted((k[0], c) for k, c in sizes.items() if k not in listed) == [(6, 2), (17, 2)]
    # every walk gets behind slot 64 of its flow: the FIN of socket 0 and its CloseWait ACK, closer 0's FIN | ACK, opener 0's SYN-ACK
    assert int(e["socks_out"]["n_delivered"][0]) == 23 and [int(x) for x in e["socks_close"]["state"]] == [9, 0]
    assert int(e["socks_close"]["n_taken"][0]) == 1
    assert [int(x) for x in e["closers_out"]["state"]] == [8, 9] and [int(x) for x in e["openers_out"]["state"]] == [4, 2]
    assert not e["conns"]["used"].any()


def test_near_keys():
    case = cases.near_keys()
    e, frames = expected(case)
    assert e["n_flows"] == 13 and [int(x) for x in np.flatnonzero(e["ctl_code"])] == [0, 1]
    assert int(e["openers_out"]["state"][0]) == 4 and int(e["openers_out"]["n_rejected"][0]) == 1


@pytest.mark.parametrize("shape", cases.BIG_SHAPES)
def test_big(shape):
    case = cases.big(shape)
    assert len(case.frames) == cases.BIG
    keys = {bytes(k) for k in case.openers["key"]}
    assert len(keys) == len(case.openers) == (65536 if shape == "65536 openers" else 1000)
    assert sum(fref.flow_key(f) in keys for f in case.frames) == len(keys)
