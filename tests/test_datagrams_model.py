"""tests/datagrams.py's exchange against tests/udp_ref.py alone (no GPU): every call's output by the header's
rules is also what the transliteration of RecvEth's UDP branch gives, nothing is lost or made up between the
calls, the server's 4-cell queue fills and drains, and every answer is its question backwards."""
import numpy as np

import datagrams as dg
import udp_ref as ref


def test_the_exchange_fills_and_drains_a_queue_and_loses_nothing():
    log = dg.run()
    assert len(log) == 2 * dg.ROUNDS
    server, client = log[0::2], log[1::2]
    for who, frames, ports, out in log:
        cells_in = log[log.index((who, frames, ports, out)) - 2][3][3] if log.index((who, frames, ports, out)) >= 2 else None
        if cells_in is None:
            cells_in = np.full(out[3].size, 0xEE if who == "server" else 0xDD, dtype=np.uint8)
        other = ref.recv_eth_model(frames, ports, cells_in)  # the second statement, on the same input
        assert other[0].tobytes() == out[0].tobytes() and all(np.array_equal(x, y) for x, y in zip(other[1:], out[1:]))
        o = out[0]
        assert (o["n_matched"] == o["n_admitted"] + np.array([(out[2][out[1] == p] == ref.FULL).sum() for p in range(len(ports))])).all()
        assert (out[1] == ref.NONE).sum() == sum(1 for f in frames if f[23] == 6 or f[36:38] == (4444).to_bytes(2, "big"))
    # the server's port 67: six questions a round into four cells of which two come back in the first rounds
    admitted = [int(out[0]["n_admitted"][0]) for _, _, _, out in server]
    full = [int((out[2][out[1] == 0] == ref.FULL).sum()) for _, _, _, out in server]
    assert admitted == [4, 2, 2, 2, 4, 4] and full == [2, 4, 4, 4, 2, 2]
    assert [int(p["free"][0]) for _, _, p, _ in server] == [4, 2, 2, 2, 4, 4] and [int(p["wcell"][0]) for _, _, p, _ in server] == [0, 0, 2, 0, 2, 2]
    # port 53 (the wildcard) takes the broadcast question too, and truncation happens where the room is 16
    assert all(int(out[0]["n_admitted"][1]) == 3 for _, _, _, out in server)
    from seqs_amd import split_dgrams

    cut = [sum(int(h["stored"]) < int(h["len"]) for h, _ in split_dgrams(out[3], p, out[0])[0]) for _, _, p, out in server]
    assert cut == [int(out[0]["n_truncated"][0]) for _, _, _, out in server] and sum(cut) > 0  # (the 17-byte question, where it is admitted)
    # every answer: the length the question had, then the question's stored bytes backwards, to the port that asked
    for (_, sframes, sports, sout), (_, cframes, cports, cout), rnd in zip(server, client, range(dg.ROUNDS)):
        asked = [d for q in split_dgrams(sout[3], sports, sout[0]) for d in q]
        answers = [d for q in split_dgrams(cout[3], cports, cout[0]) for d in q]
        read = min(admitted[rnd], 2) if rnd < 3 else admitted[rnd]  # port 67's handler reads two cells a round at first
        assert len(answers) == read + 3 and int(cout[0]["n_admitted"].sum()) == len(answers)
        want = sorted(int(h["len"]).to_bytes(2, "big") + data[::-1] for h, data in asked[:read] + asked[-3:])
        assert sorted(data for _, data in answers) == want
        assert all(bytes(h["src_ip"]) == ref.ip4(dg.SERVER_IP) and int(h["src_port"]) in (67, 53) for h, _ in answers)
    # the client's queues never fill: every call's state is the next call's input
    for (_, _, p0, out), (_, _, p1, _) in zip(client, client[1:]):
        assert list(p1["wcell"]) == list(out[0]["wcell"]) and list(p1["free"]) == list(p0["n_cells"])
