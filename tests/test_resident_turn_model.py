"""The conversation of tests/conversation.py with resident endpoints (tests/resident_turn.py) and the model
back end alone, no GPU: with persistent TX tables, the hand-off on every send and the write-back, it
terminates and passes through what the host-socket conversation does; after every send the table equals the
host chain (asserted inside the endpoint); and the hand-off, not the host, moved the receive-side state."""
import numpy as np

import conversation as conv
import resident_turn as rt


def test_the_resident_conversation_completes_and_reaches_what_it_names():
    be = rt.ResidentModel()
    handed = {"sends": 0, "with_rx": 0, "acks": 0}
    send = be.send_resident

    def counting(table, rings, rx_out, seed):
        handed["sends"] += 1
        handed["with_rx"] += rx_out is not None
        frames, outs = send(table, rings, rx_out, seed)
        handed["acks"] += int((outs["sent"] == 1).sum())
        return frames, outs

    be.send_resident = counting
    A, B, stats = rt.run(be)
    print("rounds", stats["rounds"], "codes", stats["codes"].tolist(), "window closed", stats["window_closed"],
          "most frames in a call", stats["max_frames"], "calls", stats["calls"], handed)
    conv.check_end(A, B, stats)
    assert conv.Endpoint is not rt.ResidentEndpoint and isinstance(A, rt.ResidentEndpoint)
    assert stats["codes"][3] == stats["codes"][5] == stats["codes"][6] == 0 and stats["window_closed"]["B"] == 0
    # every send but each endpoint's first handed an RX call's records off, and bare ACKs came of it
    assert handed["sends"] == 2 * stats["rounds"] and handed["with_rx"] == handed["sends"] - 2 and handed["acks"] > 0
    # the tables persisted: their send side is the mirrors' at the end (the last receive is not handed off yet),
    # and not what they were made from
    for e in (A, B):
        for k in ("hdr", "snd_nxt", "ring_rpos", "ring_buffered"):
            assert np.array_equal(e.table[k], e.tx[k]), k
    assert (A.table["snd_nxt"] != A.iss).all()
