"""The three-way handshake end to end, every call's output becoming the next call's input: the clients'
SYNs (fs_segment_batch from templates with SYN set), the accept call (fs_accept_flows_batch), a client
model that takes the SYN-ACKs (rcvSynSent, control.go:175-201, and Recv, control_user.go:204-217,
transliterated), the clients' ACK and first data (fs_send_rings_batch), a link that duplicates some SYNs,
a second accept call with the new connections listed through socks_from_accept and fresh SYNs beside
them, and the server's answer (tx_sock_from, fs_send_rings_batch) back at the client model. The driver is
written once; a back end makes the calls. Model (here) is tests/segment_ref.py, tests/send_ref.py and
tests/accept_ref.py; tests/test_gpu_handshake.py has the device's, which compares every call with the
model's for the same inputs."""
import numpy as np

import accept_cases as cases
import accept_ref as aref
import conversation as conv
import deliver_ref as dref
import flows_ref as fref
import recv_ref as rref
import segment_ref as sref

M32 = 1 << 32
SYN, ACK = rref.SYN, rref.ACK
N_FIRST, N_FRESH, N_SLOTS = 5, 2, 8
RX_RING, TX_RING = 256, 512
DUPLICATED = (1, 3)  # the clients whose SYN the link delivers a second time


def model_segment(specs, seed):
    noise = np.random.default_rng(seed).integers(0, 256, 64 * len(specs) + conv.TAIL, dtype=np.uint8)
    return (noise, *sref.expected(specs, np.zeros(1, dtype=np.uint8), 0, 0, 1, noise))


def model_accept(frames, socks, snd, rings, listeners, slots, seed):
    """((buf, off, ln), noise, the synacks prefill, accept_ref.expected's dict)."""
    batch = fref.pack(frames, lead=seed % 4, seed=seed)
    room = int(batch[2].sum())
    noise = np.random.default_rng(77 + seed).integers(0, 256, 3 + room + conv.TAIL, dtype=np.uint8)
    syn0 = np.random.default_rng(900 + seed).integers(0, 256, len(slots) * aref.STRIDE, dtype=np.uint8)
    return batch, noise, syn0, aref.expected(*batch, 0, 0, noise, 3, room, socks, snd, rings, listeners, slots, 0, syn0)


class Model(conv.Model):
    def segment(self, specs, seed):
        _, buf, off, ln, _, st = model_segment(specs, seed)
        assert (st == 0).all()
        return conv.frames_of_buffer(buf, off, ln)

    def accept(self, frames, socks, snd, rings, listeners, slots, seed):
        _, _, _, e = model_accept(frames, socks, snd, rings, listeners, slots, seed)
        rings[:] = e["rings"]
        return e


class Client:
    """A ControlBlock that has sent its SYN (StateSynSent: snd.UNA = iss, snd.NXT = iss + 1)."""

    def __init__(self, rng, k, data):
        self.hdr = bytearray(cases.header(rng, 0x5000 + k))
        self.iss, self.rcv_wnd, self.data = int(rng.integers(0, M32)) if k else M32 - 1, 1000 + k, data
        self.snd_una, self.snd_nxt, self.snd_wnd = self.iss, (self.iss + 1) % M32, 0
        self.rcv_nxt, self.state, self.got = 0, "SynSent", b""

    def syn_spec(self):
        h = bytearray(self.hdr)
        h[38:42], h[42:46], h[47] = self.iss.to_bytes(4, "big"), bytes(4), SYN
        h[48:50] = self.rcv_wnd.to_bytes(2, "big")
        return (bytes(h), 0, 0, 0)

    def take_synack(self, fr):
        """rcvSynSent, then Recv's update."""
        assert fref.flow_key(fr) == fref.flow_key(conv.mirrored(bytes(self.hdr))), "the SYN-ACK is another connection's"
        seq, ack, window, flags9, length = rref.fields(fr)
        hasSyn, hasAck = bool(flags9 & SYN), bool(flags9 & ACK)
        assert hasSyn, "errExpectedSYN"
        assert not (hasAck and ack != (self.snd_una + 1) % M32), "errBadSegack"
        assert hasAck and self.state == "SynSent"
        self.state = "Established"
        self.rcv_nxt = seq                       # resetRcv(rcv.WND, seg.SEQ)
        self.snd_wnd, self.snd_una = window, ack  # control_user.go:212-215
        self.rcv_nxt = (self.rcv_nxt + length + 1) % M32
        self.server_mac = bytes(fr[6:12])

    def tx_sock(self, ring_off):
        """The TX record of the ACK (and the first data) that answers the SYN-ACK."""
        from seqs_amd.framesum import TX_ACK, TX_PSH
        import send_ref

        h = bytearray(self.hdr)
        h[0:6] = self.server_mac
        return send_ref.sock(bytes(h), 1460, ring_off, TX_RING, 7, len(self.data), snd_una=self.snd_una, snd_nxt=self.snd_nxt,
                             snd_wnd=self.snd_wnd, rcv_nxt=self.rcv_nxt, rcv_wnd=self.rcv_wnd, flags=TX_ACK | TX_PSH)

    def take(self, fr):
        """An Established connection's in-order test (validateIncomingSegment's errRequireSequential)."""
        seq, ack, window, flags9, length = rref.fields(fr)
        assert seq == self.rcv_nxt and flags9 & ACK and ack == self.snd_nxt, "the server's answer is not in order"
        a, b = fref.payload_range(fr)
        self.got += fr[a:b]
        self.rcv_nxt = (self.rcv_nxt + length) % M32


def run(be, seed=8300):
    """The handshake with the back end `be`. Returns a dict of what the checks below read."""
    import send_ref
    from seqs_amd import socks_from_accept, tx_sock_from
    from seqs_amd.framesum import TX_SOCK_DTYPE

    rng = np.random.default_rng(seed)
    clients = [Client(rng, k, rng.integers(0, 256, 0 if k == 0 else 40 + 30 * k, dtype=np.uint8).tobytes())
               for k in range(N_FIRST + N_FRESH)]
    first, fresh = clients[:N_FIRST], clients[N_FIRST:]
    slots = aref.slots_of(*[(M32 - 2 + 1000 * k, RX_RING, 0x300 + k) for k in range(N_SLOTS)])
    listeners = aref.listeners_of((cases.local(80), cases.MAC, 0, N_SLOTS))
    rx_rings = be.rings(rng.integers(0, 256, N_SLOTS * RX_RING + 3, dtype=np.uint8))
    # 1, 2: the SYNs, the first accept call
    syns = be.segment([c.syn_spec() for c in first], seed)
    e1 = be.accept(syns, dref.socks_of(), rref.snd_of(), rx_rings, listeners, slots, seed + 1)
    # 3: the SYN-ACKs at the clients
    for c, s in zip(first, [int(x) for x in e1["accept_of"][:N_FIRST]]):
        c.take_synack(bytes(e1["synacks"][s * 64 : s * 64 + 54]))
    # 4: their ACK (client 0: a pure one) and first data
    tx = np.ascontiguousarray(send_ref.socks_of([c.tx_sock(1 + k * (TX_RING + 1)) for k, c in enumerate(first)]), dtype=TX_SOCK_DTYPE)
    c_rings = be.rings(rng.integers(0, 256, N_FIRST * (TX_RING + 1) + 2, dtype=np.uint8))
    for k, c in enumerate(first):
        if c.data:
            be.put(c_rings, int(tx["ring_off"][k]) + 7, c.data)  # (ring_rpos 7; nothing wraps)
    frames, outs = be.send(tx, c_rings, seed + 2)
    for c, o in zip(first, outs):
        c.snd_nxt = int(o["snd_nxt"])
    # 5: the link: the clients' frames, a second copy of some SYNs behind them, fresh SYNs among them
    fresh_syns = be.segment([c.syn_spec() for c in fresh], seed + 3)
    batch = list(frames) + [syns[DUPLICATED[0]], fresh_syns[0], syns[DUPLICATED[1]], fresh_syns[1]]
    # 6: the second accept call: the half-open connections listed, the listener with its free slots
    idx, socks, snd, stx = socks_from_accept(e1["conns"], slots, listeners, 1 + np.arange(N_SLOTS) * RX_RING, RX_RING)
    left = aref.listeners_of((cases.local(80), cases.MAC, len(idx), N_SLOTS - len(idx)))
    e2 = be.accept(batch, socks, snd, rx_rings, left, slots, seed + 4)
    # 7: the server's answer
    answers = [bytes([65 + k]) * (10 + k) for k in range(len(idx))]
    stx["ring_off"], stx["ring_size"] = 1 + np.arange(len(idx)) * (TX_RING + 1), TX_RING
    stx["ring_buffered"] = [len(a) for a in answers]
    s_rings = be.rings(rng.integers(0, 256, len(idx) * (TX_RING + 1) + 2, dtype=np.uint8))
    for k, a in enumerate(answers):
        be.put(s_rings, int(stx["ring_off"][k]), a)
    stx = tx_sock_from(e2["socks_out"], stx, snd_out=e2["snd_out"])
    back, _ = be.send(stx, s_rings, seed + 5)
    for fr in back:
        owner = [c for c in first if fref.flow_key(fr) == fref.flow_key(conv.mirrored(bytes(c.hdr)))]
        owner[0].take(fr)
    return dict(first=first, fresh=fresh, slots=slots, idx=idx, socks=socks, e1=e1, e2=e2, rx_rings=rx_rings, answers=answers,
                batch=batch, be=be)


def check_end(r):
    first, e1, e2, slots = r["first"], r["e1"], r["e2"], r["slots"]
    assert [int(x) for x in e1["accept_of"][:N_FIRST]] == list(range(N_FIRST)) == list(r["idx"])
    for k, c in enumerate(first):
        iss = int(slots["iss"][k])
        assert c.state == "Established" and c.snd_una == (c.iss + 1) % M32 and c.rcv_nxt == (iss + 1 + len(r["answers"][k])) % M32
        # the handshake's third ACK was taken, and the data is in the connection's ring
        assert int(e2["snd_out"]["snd_una"][k]) == (iss + 1) % M32 and int(e2["snd_out"]["n_taken"][k]) == 1
        so = e2["socks_out"][k]
        assert int(so["bytes"]) == len(c.data) and int(so["rcv_nxt"]) == (c.iss + 1 + len(c.data)) % M32
        at = int(r["socks"]["ring_off"][k])
        assert r["be"].get(r["rx_rings"], at, len(c.data)) == c.data
        assert c.got == r["answers"][k], "the server's answer did not arrive"
    # no duplicate SYN took a slot: a duplicated client's flow is its data frame and then the SYN, at which
    # the walk stops (the other flows end at their one frame); the listener sees the two fresh SYNs only
    for k in range(N_FIRST):
        fl = e2["flows"][int(e2["socks_out"]["flow"][k])]
        assert int(fl["n_frames"]) == (2 if k in DUPLICATED else 1)
        assert int(e2["socks_out"]["stop"][k]) == int(fl["first_frame"]) + 1
    assert [int(x) for x in e2["listeners_out"][0]] == [N_FRESH, N_FRESH, 0, 0]
    fresh_of = [int(x) for x in e2["accept_of"][: e2["n_flows"]] if int(x) != aref.NONE]
    assert fresh_of == [N_FIRST, N_FIRST + 1] and [int(s) for s in np.flatnonzero(e2["conns"]["used"])] == fresh_of
    for c, s in zip(r["fresh"], fresh_of):
        c.take_synack(bytes(e2["synacks"][s * 64 : s * 64 + 54]))
        assert c.state == "Established" and c.rcv_nxt == (int(slots["iss"][s]) + 1) % M32
    assert first[0].iss == M32 - 1 and int(e1["conns"]["rcv_nxt"][0]) == 0  # Seq crosses 2^32 in the handshake itself
