"""The handshake of tests/handshake.py against the models alone (tests/segment_ref.py, tests/send_ref.py,
tests/accept_ref.py): no GPU, no library call. It shows that the driver reaches what it names."""
import numpy as np

import accept_ref as aref
import handshake as hs
import recv_ref as rref


def test_the_handshake_against_the_models():
    r = hs.run(hs.Model())
    hs.check_end(r)
    e1, e2 = r["e1"], r["e2"]
    # the first call: five SYNs, five slots, no socket; every SYN carries the client's window
    assert e1["n_flows"] == hs.N_FIRST and [int(x) for x in e1["listeners_out"][0]] == [5, 5, 0, 0]
    assert [int(x) for x in e1["conns"]["snd_wnd"][:5]] == [c.rcv_wnd for c in r["first"]]
    # the second call's batch: five client frames (one pure ACK, four with data), two duplicated and two fresh SYNs
    kinds = [rref.fields(f)[3:] for f in r["batch"]]
    assert [k for k in kinds if k[0] == rref.SYN] == [(rref.SYN, 0)] * 4 and kinds[0] == (rref.ACK, 0)
    assert all(k[0] == rref.ACK | rref.PSH and k[1] > 0 for k in kinds[1:5])
    assert [int(c) for c in e2["code"][:5]] == [rref.TAKEN] * 5 and not e2["code"][5:].any()
    assert int((e2["accept_of"] == aref.NONE).sum()) == len(e2["accept_of"]) - 2
    assert (e2["snd_out"]["flags"][1:5] & rref.ACK_OWED).all() and not int(e2["snd_out"]["flags"][0])
    assert np.array_equal(e2["conns"]["used"], [0, 0, 0, 0, 0, 1, 1, 0])
