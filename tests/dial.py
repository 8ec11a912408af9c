"""The three-way handshake with the library on BOTH ends of the link, every call's output becoming the next
call's input: the clients' SYNs come from a connect call without a batch (fs_connect_flows_batch, n == 0,
FS_CN_SEND_SYN); the server's accept call (fs_accept_flows_batch) takes them; its SYN-ACKs, two of them
duplicated by the link, go into the clients' connect call, which answers each with the handshake's ACK; the
clients are listed through socks_from_connect, and their ACK replies and first data (fs_send_rings_batch) go
back into the server's call, where the connections are listed through socks_from_accept.

Beside the clients one pair of openers dials each other, and their SYNs cross: each comes back SynRcvd with
a SYN-ACK that the other side's digest accepts. Completing that open is host work: a listed socket's walk
stops at a SYN (the delivery's `stop`), so the crossing SYN-ACKs are taken by rcvSynRcvd on the host.

The driver is written once; a back end makes the calls. Model (here) is tests/connect_ref.py,
tests/accept_ref.py and tests/send_ref.py; tests/test_gpu_dial.py has the device's, which compares every
call's whole output with the model's for the same inputs."""
import numpy as np

import accept_cases as cases
import accept_ref as aref
import close_ref as clref
import connect_ref as cref
import conversation as conv
import deliver_ref as dref
import flows_ref as fref
import handshake as hs
import recv_ref as rref

M32 = 1 << 32
N_CLIENTS, N_SLOTS = 5, 8
RX_RING, TX_RING = 256, 512
DUPLICATED = (1, 3)  # the clients whose SYN-ACK the link delivers a second time
PAIR_MACS = (bytes([2, 0, 0, 0, 7, 1]), bytes([2, 0, 0, 0, 7, 2]))


def model_connect(frames, openers, seed):
    """((buf, off, ln) or None without a batch, noise, the replies prefill, connect_ref's dict)."""
    rep0 = np.random.default_rng(1100 + seed).integers(0, 256, len(openers) * cref.STRIDE + 5, dtype=np.uint8)
    if not frames:
        return None, None, rep0, cref.contract([], dict(), openers, 0, 0, rep0, np.zeros(0, np.uint8))
    batch = fref.pack(frames, lead=seed % 4, seed=seed)
    room = int(batch[2].sum())
    noise = np.random.default_rng(77 + seed).integers(0, 256, 3 + room + conv.TAIL, dtype=np.uint8)
    e = cref.expected(*batch, 0, 0, noise, 3, room, dref.socks_of(), rref.snd_of(), np.zeros(64, np.uint8), aref.listeners_of(),
                      aref.slots_of(), 0, np.zeros(0, np.uint8), clref.closers_of(), openers, 0, rep0)
    return batch, noise, rep0, e


class Model(hs.Model):
    def connect(self, frames, openers, seed):
        return model_connect(frames, openers, seed)[3]


def replies_of(e):
    """{opener: its 54-byte reply} of a connect call's dict."""
    return {int(i): bytes(e["replies"][i * 64 : i * 64 + 54]) for i in np.flatnonzero(e["openers_out"]["reply"])}


def run(be, seed=8400):
    """The handshake with the back end `be`. Returns a dict of what check_end reads."""
    from seqs_amd import socks_from_accept, socks_from_connect
    from seqs_amd.framesum import CN_SEND_SYN, TX_ACK, TX_PSH

    rng = np.random.default_rng(seed)
    data = [rng.integers(0, 256, 0 if k == 0 else 40 + 30 * k, dtype=np.uint8).tobytes() for k in range(N_CLIENTS)]
    hdrs = [cases.header(rng, 0x5000 + k) for k in range(N_CLIENTS)]  # a client's frames to the server
    rows = [(fref.flow_key(conv.mirrored(h)), CN_SEND_SYN, h[6:12], cases.MAC, M32 - 1 if k == 0 else int(rng.integers(0, M32)),
             1000 + k, 0x700 + k) for k, h in enumerate(hdrs)]
    # the pair that dials each other: each one's key is the key of the other's frames
    pa = cases.header(rng, 0x5100, port=0x5101)
    pa = pa[:0] + PAIR_MACS[1] + PAIR_MACS[0] + pa[12:]  # A's frames: to B's MAC from A's
    rows.append((fref.flow_key(conv.mirrored(pa)), CN_SEND_SYN, PAIR_MACS[0], PAIR_MACS[1], 111111, 900, 0x801))
    rows.append((fref.flow_key(pa), CN_SEND_SYN, PAIR_MACS[1], PAIR_MACS[0], M32 - 5, 800, 0x802))
    openers = cref.openers_of(*rows)
    slots = aref.slots_of(*[(M32 - 2 + 1000 * k, RX_RING, 0x300 + k) for k in range(N_SLOTS)])
    listeners = aref.listeners_of((cases.local(80), cases.MAC, 0, N_SLOTS))
    rx_rings = be.rings(rng.integers(0, 256, N_SLOTS * RX_RING + 3, dtype=np.uint8))
    # 1: the first SYNs, from a connect call without a batch
    c1 = be.connect([], openers, seed)
    syns = replies_of(c1)
    # 2: the server takes the clients' SYNs
    e1 = be.accept([syns[k] for k in range(N_CLIENTS)], dref.socks_of(), rref.snd_of(), rx_rings, listeners, slots, seed + 1)
    # 3: the SYN-ACKs at the clients, two of them twice; the pair's SYNs cross on the same link
    slot_of = [int(x) for x in e1["accept_of"][:N_CLIENTS]]
    synacks = [bytes(e1["synacks"][s * 64 : s * 64 + 54]) for s in slot_of]
    link = synacks + [synacks[k] for k in DUPLICATED] + [syns[N_CLIENTS], syns[N_CLIENTS + 1]]
    waiting = openers.copy()
    waiting["flags"] = 0  # (the 3-second timer has not fired)
    c2 = be.connect(link, waiting, seed + 2)
    acks = replies_of(c2)
    # 4: the clients are listed; their ACK replies and first data go to the server
    idx, c_socks, c_snd, tx = socks_from_connect(openers, c2["openers_out"], 1 + np.arange(len(openers)) * RX_RING, RX_RING)
    mine = np.flatnonzero(idx < N_CLIENTS)
    tx = tx[mine]
    tx["ring_off"], tx["ring_size"], tx["ring_rpos"] = 1 + np.arange(N_CLIENTS) * (TX_RING + 1), TX_RING, 7
    tx["ring_buffered"], tx["flags"] = [len(d) for d in data], TX_ACK | TX_PSH
    c_rings = be.rings(rng.integers(0, 256, N_CLIENTS * (TX_RING + 1) + 2, dtype=np.uint8))
    for k, d in enumerate(data):
        if d:
            be.put(c_rings, int(tx["ring_off"][k]) + 7, d)  # (ring_rpos 7; nothing wraps)
    frames, outs = be.send(tx, c_rings, seed + 3)
    batch = [acks[k] for k in range(N_CLIENTS)] + list(frames)
    s_idx, socks, snd, _ = socks_from_accept(e1["conns"], slots, listeners, 1 + np.arange(N_SLOTS) * RX_RING, RX_RING)
    left = aref.listeners_of((cases.local(80), cases.MAC, len(s_idx), N_SLOTS - len(s_idx)))
    e2 = be.accept(batch, socks, snd, rx_rings, left, slots, seed + 4)
    return dict(openers=openers, data=data, slots=slots, c1=c1, e1=e1, c2=c2, e2=e2, slot_of=slot_of, socks=socks, c_socks=c_socks,
                c_snd=c_snd, idx=idx, outs=outs, rx_rings=rx_rings, be=be, synacks=synacks)


def check_end(r):
    openers, slots, c1, c2, e1, e2 = r["openers"], r["slots"], r["c1"], r["c2"], r["e1"], r["e2"]
    n = len(openers)
    # 1: every opener is still in SynSent and owes its SYN; nothing else came back
    assert (c1["openers_out"]["state"] == 3).all() and (c1["openers_out"]["reply"] == cref.REPLY_SYN).all()
    assert (c1["openers_out"]["stop"] == cref.NONE).all() and not c1["reply_status"].any()
    # 2: each client's SYN took a slot, in order
    assert r["slot_of"] == list(range(N_CLIENTS)) and int(e1["conns"]["used"].sum()) == N_CLIENTS
    # 3: the clients are Established on the server's numbers, a duplicate lies untouched behind `stop`
    out = c2["openers_out"]
    assert [int(x) for x in out["state"]] == [4] * N_CLIENTS + [2, 2] and list(r["idx"]) == list(range(n))
    for k in range(N_CLIENTS):
        iss, s_iss = int(openers["iss"][k]), int(slots["iss"][k])
        assert (int(out["irs"][k]), int(out["rcv_nxt"][k])) == (s_iss % M32, (s_iss + 1) % M32)
        assert (int(out["snd_una"][k]), int(out["snd_nxt"][k])) == ((iss + 1) % M32,) * 2 and int(out["snd_wnd"][k]) == RX_RING
        assert int(out["reply"][k]) == cref.REPLY_ACK and int(e1["conns"]["rcv_nxt"][k]) == (iss + 1) % M32
        ack = bytes(c2["replies"][k * 64 : k * 64 + 54])
        assert int.from_bytes(ack[38:42], "big") == (iss + 1) % M32 and int.from_bytes(ack[42:46], "big") == (s_iss + 1) % M32
    assert int(openers["iss"][0]) == M32 - 1 and int(out["snd_nxt"][0]) == 0  # Seq crosses 2^32 in the handshake itself
    assert int((c2["ctl_code"] == 1).sum()) == n and int((c2["ctl_code"] == 0).sum()) == len(DUPLICATED)
    # the pair whose SYNs crossed: SynRcvd on both sides, each SYN-ACK acknowledges the other's ISS, and the
    # digest of both is clean
    a, b = N_CLIENTS, N_CLIENTS + 1
    for me, peer in ((a, b), (b, a)):
        fr = bytes(c2["replies"][me * 64 : me * 64 + 54])
        assert int(out["reply"][me]) == cref.REPLY_SYNACK and fr[47] == cref.SYN | cref.ACK and int(c2["reply_status"][me]) == 0
        assert int.from_bytes(fr[38:42], "big") == int(openers["iss"][me]) == int(out["snd_nxt"][me]) == int(out["snd_una"][me])
        assert int.from_bytes(fr[42:46], "big") == (int(openers["iss"][peer]) + 1) % M32 == int(out["rcv_nxt"][me])
        assert fref.flow_key(fr) == bytes(openers["key"][peer])  # it is a frame of the peer's flow
    # 4: at the server the handshake's third ACK was taken and the data is in the connection's ring
    for k in range(N_CLIENTS):
        s_iss, iss, d = int(slots["iss"][k]), int(openers["iss"][k]), r["data"][k]
        assert int(e2["snd_out"]["snd_una"][k]) == (s_iss + 1) % M32 and int(e2["snd_out"]["n_taken"][k]) >= 1
        so = e2["socks_out"][k]
        assert int(so["bytes"]) == len(d) and int(so["rcv_nxt"]) == (iss + 1 + len(d)) % M32
        assert r["be"].get(r["rx_rings"], int(r["socks"]["ring_off"][k]), len(d)) == d
        assert int(r["outs"]["snd_nxt"][k]) == (iss + 1 + len(d)) % M32
    assert [int(x) for x in e2["listeners_out"][0]] == [0, 0, 0, 0]
