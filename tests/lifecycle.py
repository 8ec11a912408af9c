"""Six connections from their SYN to their last ACK, every call's output becoming the next call's input:
the handshake of tests/handshake.py (its clients, its SYNs from fs_segment_batch, the slots of a
listener), data both ways (fs_send_rings_batch on both sides, the RX rings of the server), and then one
ending per connection, every batch through ONE RX call, fs_close_flows_batch:

  0 passive      the peer's FIN (CloseWait), our data still flowing and acknowledged there, our FIN
                 (LastAck by state_after_send), the peer's last ACK: Closed
  1 active       our FIN (FinWait1 by state_after_send), the peer's ACK (FinWait2), the peer's FIN: TimeWait
  2 shortcut     our FIN, the peer's FIN | ACK that acknowledges it: FinWait1 -> TimeWait
  3 simultaneous our FIN, the peer's FIN that has not seen it: Closing; our ACK (TimeWait by
                 state_after_send); the peer's late ACK is ignored there
  4 RST          in Established
  5 RST          in CloseWait

The peers are tests/handshake.py's clients, which check every frame they get (in order, the right Ack). The
host loop between the calls is the binding's: socks_from_accept, tx_sock_from, closers_from and
state_after_send. The driver is written once; a back end makes the calls. Model (here) is
tests/segment_ref.py, tests/send_ref.py and tests/close_ref.py; tests/test_gpu_lifecycle.py has the device's,
which compares every call with the model's for the same inputs."""
import numpy as np

import accept_cases as acases
import accept_ref as aref
import close_ref as cref
import conversation as conv
import deliver_ref as dref
import flows_ref as fref
import handshake as hs
import recv_cases as rcases
import recv_ref as rref

M32 = 1 << 32
FIN, SYN, RST, ACK = rref.FIN, rref.SYN, rref.RST, rref.ACK
ENDINGS = ("passive", "active", "shortcut", "simultaneous", "rst established", "rst close-wait")
N = len(ENDINGS)
RX_RING, TX_RING = 256, 512


def model_close(frames, socks, snd, rings, listeners, slots, closers, seed):
    """((buf, off, ln), noise, the synacks prefill, close_ref.expected's dict)."""
    batch = fref.pack(frames, lead=seed % 4, seed=seed)
    room = int(batch[2].sum())
    noise = np.random.default_rng(77 + seed).integers(0, 256, 3 + room + conv.TAIL, dtype=np.uint8)
    syn0 = np.random.default_rng(900 + seed).integers(0, 256, len(slots) * aref.STRIDE, dtype=np.uint8)
    return batch, noise, syn0, cref.expected(*batch, 0, 0, noise, 3, room, socks, snd, rings, listeners, slots, 0, syn0, closers)


class Model(hs.Model):
    def close(self, frames, socks, snd, rings, listeners, slots, closers, seed):
        _, _, _, e = model_close(frames, socks, snd, rings, listeners, slots, closers, seed)
        rings[:] = e["rings"]
        return e


class Peer(hs.Client):
    """A client that also takes the server's FIN and writes its own closing frames."""

    fin_seen = False

    def take(self, fr):
        seq, ack, window, flags9, length = rref.fields(fr)
        assert seq == self.rcv_nxt and flags9 & ACK and ack == self.snd_nxt, "the server's frame is not in order"
        assert not flags9 & (SYN | RST)
        a, b = fref.payload_range(fr)
        self.got += fr[a:b]
        self.rcv_nxt = (self.rcv_nxt + length + (1 if flags9 & FIN else 0)) % M32
        self.fin_seen = self.fin_seen or bool(flags9 & FIN)

    def frame(self, flags9, ack=None):
        """A segment without data at snd.NXT; a FIN takes a sequence number."""
        h = bytearray(self.hdr)
        h[0:6] = self.server_mac
        fr = rcases.frame(bytes(h), self.snd_nxt, self.rcv_nxt if ack is None else ack, flags9, self.rcv_wnd)
        if flags9 & FIN:
            self.snd_nxt = (self.snd_nxt + 1) % M32
        return fr


def closer_row(sock, snd_una, snd_wnd, snd_nxt, state):
    return (bytes(sock["key"]), state, int(sock["rcv_nxt"]), int(sock["rcv_wnd"]), snd_una, snd_nxt, snd_wnd)


def run(be, seed=8600):
    """The six lifecycles with the back end `be`. Returns a dict of what check_end and the tests read."""
    import send_ref
    from seqs_amd import closers_from, socks_from_accept, state_after_send, tx_sock_from
    from seqs_amd.framesum import TX_ACK, TX_FIN, TX_SOCK_DTYPE

    rng = np.random.default_rng(seed)
    peers = [Peer(rng, k, rng.integers(0, 256, 0 if k == 0 else 40 + 30 * k, dtype=np.uint8).tobytes()) for k in range(N)]
    slots = aref.slots_of(*[(M32 - 2 + 1000 * k, RX_RING, 0x300 + k) for k in range(N)])
    listeners = aref.listeners_of((acases.local(80), acases.MAC, 0, N))
    no_slots = aref.listeners_of((acases.local(80), acases.MAC, N, 0))
    none = cref.closers_of()
    rx_rings = be.rings(rng.integers(0, 256, N * RX_RING + 3, dtype=np.uint8))
    state = [cref.ESTABLISHED] * N
    log = []

    # ---- the handshake and data both ways
    syns = be.segment([p.syn_spec() for p in peers], seed)
    e1 = be.close(syns, dref.socks_of(), rref.snd_of(), rx_rings, listeners, slots, none, seed + 1)
    for p, s in zip(peers, [int(x) for x in e1["accept_of"][:N]]):
        p.take_synack(bytes(e1["synacks"][s * 64 : s * 64 + 54]))
    tx = np.ascontiguousarray(send_ref.socks_of([p.tx_sock(1 + k * (TX_RING + 1)) for k, p in enumerate(peers)]), dtype=TX_SOCK_DTYPE)
    c_rings = be.rings(rng.integers(0, 256, N * (TX_RING + 1) + 2, dtype=np.uint8))
    for k, p in enumerate(peers):
        if p.data:
            be.put(c_rings, int(tx["ring_off"][k]) + 7, p.data)
    frames, outs = be.send(tx, c_rings, seed + 2)
    for p, o in zip(peers, outs):
        p.snd_nxt = int(o["snd_nxt"])
    idx, socks, snd, stx = socks_from_accept(e1["conns"], slots, listeners, 1 + np.arange(N) * RX_RING, RX_RING)
    assert list(idx) == list(range(N))
    e2 = be.close(list(frames), socks, snd, rx_rings, no_slots, slots, none, seed + 3)
    log.append(("data", e2))
    assert (e2["socks_close"]["state"] == cref.ESTABLISHED).all() and not e2["ctl_code"].any()
    received = [be.get(rx_rings, int(socks["ring_off"][k]), len(p.data)) for k, p in enumerate(peers)]
    for name in ("rcv_nxt", "ring_wpos"):
        socks[name] = e2["socks_out"][name]  # (the application has read the rings: ring_free stays the ring's size)
    una, wnd = e2["snd_out"]["snd_una"].copy(), e2["snd_out"]["snd_wnd"].copy()

    # ---- the server's answer; connections 1, 2 and 3 close behind it (Send: Established -> FinWait1)
    answers = [bytes([65 + k]) * (10 + k) for k in range(N)]
    stx["ring_off"], stx["ring_size"] = 1 + np.arange(N) * (TX_RING + 1), TX_RING
    stx["ring_buffered"] = [len(a) for a in answers]
    s_rings = be.rings(rng.integers(0, 256, N * (TX_RING + 1) + 2, dtype=np.uint8))
    for k, a in enumerate(answers):
        be.put(s_rings, int(stx["ring_off"][k]), a)
    stx = tx_sock_from(e2["socks_out"], stx, snd_out=e2["snd_out"])
    stx["rcv_wnd"] = RX_RING
    stx["flags"][1:4] |= TX_FIN

    def server_send(rows, seed):
        """One ring send of the server's rows; the records, the states and the peers follow."""
        sub = np.ascontiguousarray(stx[rows])
        back, outs = be.send(sub, s_rings, seed)
        for r, o in zip(rows, outs):
            for name in ("snd_nxt", "ring_rpos", "ring_buffered"):
                stx[name][r] = o[name]
            stx["hdr"][r, 18], stx["hdr"][r, 19] = int(o["ip_id"]) >> 8, int(o["ip_id"]) & 0xFF
            stx["flags"][r] = 0
            state[r] = state_after_send(state[r], int(o["sent"]))
        for fr in back:
            (owner,) = [p for p in peers if fref.flow_key(fr) == fref.flow_key(conv.mirrored(bytes(p.hdr)))]
            owner.take(fr)
        return outs

    server_send(list(range(N)), seed + 4)
    assert state == [4, 5, 5, 5, 4, 4] and [p.fin_seen for p in peers] == [False, True, True, True, False, False]

    # ---- round A: one batch, one call
    p = peers
    batch = fref.finish([p[0].frame(FIN | ACK), p[1].frame(ACK), p[2].frame(FIN | ACK),
                         p[3].frame(FIN | ACK, ack=(p[3].rcv_nxt - 1) % M32), p[4].frame(RST), p[5].frame(FIN | ACK)])
    est = [0, 4, 5]
    socks["snd_nxt"] = stx["snd_nxt"]
    closers = cref.closers_of(*[closer_row(socks[k], int(una[k]), int(wnd[k]), int(stx["snd_nxt"][k]), state[k]) for k in (1, 2, 3)])
    e3 = be.close(batch, socks[est], rref.snd_of(*[(int(una[k]), int(wnd[k])) for k in est]), rx_rings, no_slots, slots, closers,
                  seed + 5)
    log.append(("round A", e3))
    for k, o in zip((1, 2, 3), e3["closers_out"]):
        state[k] = int(o["state"])
    for k, o in zip(est, e3["socks_close"]):
        state[k] = int(o["state"])
    assert state == [9, 6, 8, 7, 0, 9], state
    # the host loop: who left Established is listed as a closer from now on
    left, new = closers_from(socks[est], e3["socks_close"])
    assert [est[i] for i in left] == [0, 4, 5]
    rec = {k: r for k, r in zip((1, 2, 3), closers)}
    for k, o in zip((1, 2, 3), e3["closers_out"]):
        for name in ("state", "rcv_nxt", "snd_una", "snd_wnd"):
            rec[k][name] = o[name]
    rec.update({est[i]: r for i, r in zip(left, new)})
    owed_a = {k: int(o["flags"]) for k, o in zip((1, 2, 3), e3["closers_out"])}

    # ---- our ACKs: connection 0 still streams in CloseWait, 3 leaves Closing by its ACK (Send), 5 owes one
    late = b"late data behind the peer's FIN"
    be.put(s_rings, int(stx["ring_off"][0]) + int(stx["ring_rpos"][0]), late)
    stx["ring_buffered"][0] = len(late)
    for k in (0, 3, 5):
        stx["rcv_nxt"][k], stx["snd_una"][k], stx["snd_wnd"][k] = rec[k]["rcv_nxt"], rec[k]["snd_una"], rec[k]["snd_wnd"]
        stx["flags"][k] = TX_ACK
    server_send([0, 3, 5], seed + 6)
    assert state == [9, 6, 8, 8, 0, 9] and p[0].got == answers[0] + late

    # ---- round B
    batch = fref.finish([p[0].frame(ACK), p[1].frame(FIN | ACK), p[3].frame(ACK), p[5].frame(RST)])
    order = (0, 1, 3, 5)
    for k in order:
        rec[k]["state"], rec[k]["snd_nxt"] = state[k], stx["snd_nxt"][k]
    e4 = be.close(batch, dref.socks_of(), rref.snd_of(), rx_rings, no_slots, slots, np.array([rec[k] for k in order]), seed + 7)
    log.append(("round B", e4))
    for k, o in zip(order, e4["closers_out"]):
        state[k] = int(o["state"])
        for name in ("state", "rcv_nxt", "snd_una", "snd_wnd"):
            rec[k][name] = o[name]
    assert state == [9, 8, 8, 8, 0, 0], state

    # ---- our FIN on connection 0 (Send: CloseWait -> LastAck), our last ACK on 1
    for k, fl in ((0, TX_FIN), (1, TX_ACK)):
        stx["rcv_nxt"][k], stx["snd_una"][k], stx["snd_wnd"][k] = rec[k]["rcv_nxt"], rec[k]["snd_una"], rec[k]["snd_wnd"]
        stx["flags"][k] = fl
    server_send([0, 1], seed + 8)
    assert state == [10, 8, 8, 8, 0, 0] and p[0].fin_seen

    # ---- round C: the last ACK
    rec[0]["state"], rec[0]["snd_nxt"] = state[0], stx["snd_nxt"][0]
    e5 = be.close(fref.finish([p[0].frame(ACK)]), dref.socks_of(), rref.snd_of(), rx_rings, no_slots, slots, np.array([rec[0]]),
                  seed + 9)
    log.append(("round C", e5))
    state[0] = int(e5["closers_out"]["state"][0])
    return dict(peers=peers, state=state, log=log, e1=e1, e2=e2, e3=e3, e4=e4, e5=e5, received=received, answers=answers, late=late,
                owed_a=owed_a, stx=stx, be=be)


def check_end(r):
    p, e3, e4, e5 = r["peers"], r["e3"], r["e4"], r["e5"]
    assert r["state"] == [0, 8, 8, 8, 0, 0]
    # the handshake and the data both ways
    assert [int(x) for x in r["e1"]["accept_of"][:N]] == list(range(N)) and r["received"] == [q.data for q in p]
    assert (r["e2"]["snd_out"]["n_taken"] == 1).all()
    for k, q in enumerate(p):
        assert q.got == r["answers"][k] + (r["late"] if k == 0 else b"")
    # round A: the FINs the receive call admitted (0 and 5), the RST it stopped at (4), the three closers
    assert [int(x) for x in e3["socks_close"]["state"]] == [9, 0, 9] and int(e3["socks_close"]["flags"][1]) == cref.RESET
    assert (e3["snd_out"]["flags"][[0, 2]] & rref.FIN_SEEN).all() and not int(e3["snd_out"]["flags"][1]) & rref.FIN_SEEN
    assert [int(x) for x in e3["closers_out"]["state"]] == [6, 8, 7]
    assert r["owed_a"] == {1: cref.ACK_OWED, 2: cref.ACK_OWED | cref.FIN_TAKEN, 3: cref.ACK_OWED | cref.FIN_TAKEN}
    assert sorted(int(c) for c in e3["ctl_code"]) == [0, 0, 1, 1, 1, 9]  # the two admitted FINs are the receive call's
    # round B: the ACK of the late data in CloseWait, FinWait2's FIN, TimeWait's ignored ACK, the RST in CloseWait
    out = e4["closers_out"]
    assert [int(x) for x in out["state"]] == [9, 8, 8, 0] and [int(x) for x in out["flags"]] == [0, 3, 0, cref.RESET]
    assert int(out["snd_una"][0]) == (int(r["stx"]["snd_nxt"][0]) - 1) % M32  # everything but our FIN, which comes later
    assert sorted(int(c) for c in e4["ctl_code"]) == [1, 1, 8, 9]
    # round C: LastAck's ACK
    assert [int(x) for x in e5["closers_out"][0]][:6] == [0, 0, 0, 0, 1, 0] and list(e5["ctl_code"]) == [1]
    # Seq crosses 2^32 on the way (client 0's iss, slot 0's iss)
    assert p[0].iss == M32 - 1
