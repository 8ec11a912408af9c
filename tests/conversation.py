"""Two endpoints that talk over three TCP connections for many rounds, every call's output becoming the
next call's input: the ring send (fs_send_rings_batch), a link that interleaves and duplicates frames,
the receive call (fs_recv_flows_batch: the in-order delivery plus the fold of ACKs and windows), the
applications' reads and writes, and tx_sock_from. The driver is written once; a back end makes the
calls. Model (here) is tests/send_ref.py and tests/recv_ref.py; tests/test_gpu_conversation.py has the
device's, which compares every call with the model's for the same inputs.

A sends a stream per connection and a FIN behind it, B a byte per connection and round (its data
segments carry the window updates: a pure ACK with an old Ack is a duplicate whose window is not
taken). B's small RX rings and its slow reader on connection 0 close A's window; no frame is lost, so
nothing is ever sent twice by an endpoint."""
import numpy as np

import deliver_ref as dref
import flows_ref as fref
import recv_ref as rref
import segment_ref as sref
import send_ref

M32 = 1 << 32
TAIL = 256  # noise behind the last built frame
ALIGN = 4


class Params:
    seed = 4100
    a_streams = (6000, 12000, 20000)
    a_mss = (100, 536, 1460)
    a_tx_ring = 8192
    a_tx_start = 8192 - 40       # the TX rings' first read position
    a_iss = (M32 - 3000, 7, None)  # (None: a random one)
    a_rx_ring = 4096
    b_stream = 400
    b_tx_ring = 512
    b_iss = (M32 - 50, None, 99)
    b_rx_rings = (600, 1500, 4096)
    dup_stride, dup_first, dup_later = 7, 3, 2  # a second copy of every seventh frame, two places later
    max_rounds = 100

    @staticmethod
    def b_quota(conn, rnd):
        """How many bytes B's application reads of a connection's RX ring behind a round's receive."""
        return ((600 if rnd % 2 == 0 else 0), 1 << 20, 1700)[conn]


# ---- the model back end --------------------------------------------------------------------------

def tx_dicts(tx):
    """A TX_SOCK_DTYPE array as the list of dicts tests/send_ref.py takes."""
    return [{k: (t[k].tobytes() if k == "hdr" else int(t[k])) for k in tx.dtype.names} for t in tx]


def model_send(tx, rings, seed):
    """(noise, then send_ref.expected's tuple) for a build of `tx` into a copy of `noise`."""
    socks = tx_dicts(tx)
    frames, _ = send_ref.frames_of(socks, rings)
    _, total = sref.layout([len(f) for f in frames], 0, ALIGN)
    noise = np.random.default_rng(seed).integers(0, 256, total + TAIL, dtype=np.uint8)
    return (noise, *send_ref.expected(socks, rings, 0, 0, ALIGN, noise))


def frames_of_buffer(buf, off, ln):
    return [buf[int(o) : int(o) + int(n)].tobytes() for o, n in zip(off, ln)]


def model_recv(frames, socks, snd, rings, seed):
    """((buf, off, ln), noise, recv_ref.expected's dict) for a receive of the frames into noise[3 : 3 + room]."""
    batch = fref.pack(frames, lead=seed % 4, seed=seed)
    room = int(batch[2].sum())
    noise = np.random.default_rng(77 + seed).integers(0, 256, 3 + room + TAIL, dtype=np.uint8)
    return batch, noise, rref.expected(*batch, 0, 0, noise, 3, room, socks, snd, rings)


class Model:
    """The calls as tests/send_ref.py and tests/recv_ref.py restate them; rings are numpy arrays."""

    def rings(self, initial):
        return initial.copy()

    def put(self, rings, at, data):
        rings[at : at + len(data)] = np.frombuffer(data, dtype=np.uint8)

    def get(self, rings, at, n):
        return rings[at : at + n].tobytes()

    def send(self, tx, rings, seed):
        _, buf, off, ln, _, st, outs = model_send(tx, rings, seed)
        assert (st == 0).all()
        return frames_of_buffer(buf, off, ln), outs

    def recv(self, frames, socks, snd, rings, seed):
        _, _, e = model_recv(frames, socks, snd, rings, seed)
        rings[:] = e["rings"]
        return e["snd_out"], e["socks_out"], e["code"], e["st"]


# ---- the endpoints -------------------------------------------------------------------------------

def mirrored(hdr):
    """The header of the other direction: MACs, addresses and ports swapped."""
    h = bytearray(hdr)
    h[0:6], h[6:12] = hdr[6:12], hdr[0:6]
    h[26:30], h[30:34] = hdr[30:34], hdr[26:30]
    h[34:36], h[36:38] = hdr[36:38], hdr[34:36]
    return bytes(h)


class Endpoint:
    """One side's three connections: the TX records, the RX records, both rings buffers and the applications."""

    def __init__(self, be, rng, name, hdrs, peer_hdrs, iss, irs, mss, max_frames, tx_ring, tx_start, rx_rings, rx_start,
                 peer_rx_rings, streams, sends_fin, quota):
        from seqs_amd.framesum import TX_SOCK_DTYPE

        self.name, self.be, self.streams, self.sends_fin, self.quota = name, be, streams, sends_fin, quota
        n = len(hdrs)
        tx, at = [], 1
        for c in range(n):
            tx.append(send_ref.sock(hdrs[c], mss[c], at, tx_ring, tx_start % tx_ring, 0, snd_una=iss[c], snd_nxt=iss[c],
                                    snd_wnd=peer_rx_rings[c], rcv_nxt=irs[c], rcv_wnd=rx_rings[c], max_frames=max_frames))
            at += tx_ring + 1
        self.tx = np.ascontiguousarray(send_ref.socks_of(tx), dtype=TX_SOCK_DTYPE)
        self.tx_rings = be.rings(rng.integers(0, 256, at + 1, dtype=np.uint8))
        rx, at = [], 2
        for c in range(n):
            rx.append(dref.sock(dref.key_of_header(peer_hdrs[c]), irs[c], at, rx_rings[c], rcv_wnd=rx_rings[c], snd_nxt=iss[c],
                                ring_wpos=rx_start(rx_rings[c])))
            at += rx_rings[c] + 1
        self.rx = dref.socks_of(*rx)
        self.rx_rings = be.rings(rng.integers(0, 256, at + 2, dtype=np.uint8))
        self.iss = list(iss)
        self.written, self.received, self.fin_done = [0] * n, [bytearray() for _ in range(n)], [False] * n
        self.tx_wrapped, self.rx_wrapped = [False] * n, [False] * n

    def ring_ranges(self, off, size, pos, count):
        """The at most two linear ranges of `count` ring bytes from `pos` on."""
        first = min(count, size - pos)
        return [(off + pos, first)] + ([(off, count - first)] if count > first else [])

    def write(self):
        """Step 1: every application writes what fits into its TX ring behind the unacknowledged bytes."""
        from seqs_amd.framesum import TX_FIN

        for c, t in enumerate(self.tx):
            left = len(self.streams[c]) - self.written[c]
            if left == 0:
                continue
            in_flight = (int(t["snd_nxt"]) - int(t["snd_una"])) % M32
            size, buffered = int(t["ring_size"]), int(t["ring_buffered"])
            count = min(left, size - in_flight - buffered)
            data, at = self.streams[c][self.written[c] : self.written[c] + count], 0
            for lo, k in self.ring_ranges(int(t["ring_off"]), size, (int(t["ring_rpos"]) + buffered) % size, count):
                self.be.put(self.tx_rings, lo, data[at : at + k])
                at += k
            self.written[c] += count
            self.tx["ring_buffered"][c] = buffered + count
            if self.sends_fin and self.written[c] == len(self.streams[c]):
                self.tx["flags"][c] |= TX_FIN

    def send(self, seed, stats):
        """Step 2: one ring send; returns the frames per socket."""
        from seqs_amd.framesum import TX_ACK, TX_FIN

        before = self.tx.copy()
        frames, outs = self.be.send(self.tx, self.tx_rings, seed)
        lists = []
        for c, o in enumerate(outs):
            in_flight = (int(before["snd_nxt"][c]) - int(before["snd_una"][c])) % M32
            if int(before["ring_buffered"][c]) > 0 and int(o["bytes"]) == 0 and int(before["snd_wnd"][c]) <= in_flight:
                stats["window_closed"][self.name] += 1
            if int(before["ring_rpos"][c]) + int(o["bytes"]) >= int(before["ring_size"][c]):
                self.tx_wrapped[c] = True
            for k in ("snd_nxt", "ring_rpos", "ring_buffered"):
                self.tx[k][c] = o[k]
            self.tx["hdr"][c, 18], self.tx["hdr"][c, 19] = int(o["ip_id"]) >> 8, int(o["ip_id"]) & 0xFF
            if int(o["sent"]) == TX_FIN:
                self.fin_done[c] = True
                self.tx["flags"][c] &= ~np.uint32(TX_FIN)
                stats["fins_sent"] += 1
            self.tx["flags"][c] &= ~np.uint32(TX_ACK)
            first, count = int(o["first_frame"]), int(o["n_frames"])
            lists.append(frames[first : first + count] if count else [])
        return lists

    def receive(self, frames, rnd, seed, stats):
        """Step 4: one receive call, the applications' reads, and the next TX records."""
        from seqs_amd import tx_sock_from

        assert frames, "every round carries frames both ways"
        self.rx["snd_nxt"] = self.tx["snd_nxt"]
        snd = rref.snd_of(*[(int(t["snd_una"]), int(t["snd_wnd"])) for t in self.tx])
        snd_out, socks_out, code, st = self.be.recv(frames, self.rx, snd, self.rx_rings, seed)
        assert (np.asarray(st) == 0).all(), "the link damages nothing"
        stats["codes"] += np.bincount(code, minlength=7)
        stats["max_frames"] = max(stats["max_frames"], len(frames))
        so = np.array(socks_out, copy=True)
        for c in range(len(self.tx)):
            size, wpos = int(self.rx["ring_size"][c]), int(so["ring_wpos"][c])
            if int(self.rx["ring_wpos"][c]) + int(so["bytes"][c]) >= size:
                self.rx_wrapped[c] = True
            used = size - int(so["ring_free"][c])
            count = min(self.quota(c, rnd), used)
            for lo, k in self.ring_ranges(int(self.rx["ring_off"][c]), size, (wpos - used) % size, count):
                self.received[c] += self.be.get(self.rx_rings, lo, k)
            so["ring_free"][c] += count
            stats["fins_seen"] += 1 if int(snd_out["flags"][c]) & rref.FIN_SEEN else 0
        for k in ("rcv_nxt", "ring_wpos", "ring_free"):
            self.rx[k] = so[k]
        self.rx["rcv_wnd"] = np.minimum(so["ring_free"], 65535)
        self.tx = tx_sock_from(so, self.tx, snd_out=snd_out)


class Link:
    """Step 3: the per-socket frame lists interleaved, and a second copy of every `stride`-th frame of a
    direction (counted over the whole conversation) `later` places behind the first. No frame is lost."""

    def __init__(self, p):
        self.p, self.count = p, 0

    def carry(self, lists):
        merged = [lists[g][k] for g, k in fref.interleave(lists)]
        out, due = [], []
        for i, f in enumerate(merged):
            out.append(f)
            if self.count % self.p.dup_stride == self.p.dup_first:
                due.append((min(i + self.p.dup_later, len(merged) - 1), f))
            self.count += 1
            out += [g for at, g in due if at == i]
        return out


def run(be, p=Params):
    """The conversation with the back end `be`. Returns (A, B, stats): stats['rounds'] is None when it
    was not done within p.max_rounds."""
    rng = np.random.default_rng(p.seed)
    n = len(p.a_streams)
    a_hdrs = [fref.flow_header(rng, 0x4100 + c) for c in range(n)]
    b_hdrs = [mirrored(h) for h in a_hdrs]
    a_iss = [int(rng.integers(0, M32)) if s is None else s for s in p.a_iss]
    b_iss = [int(rng.integers(0, M32)) if s is None else s for s in p.b_iss]
    a_streams = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in p.a_streams]
    b_streams = [rng.integers(0, 256, p.b_stream, dtype=np.uint8).tobytes() for _ in range(n)]
    A = Endpoint(be, rng, "A", a_hdrs, b_hdrs, a_iss, b_iss, p.a_mss, 0, p.a_tx_ring, p.a_tx_start, [p.a_rx_ring] * n,
                 lambda size: size - 6, p.b_rx_rings, a_streams, True, lambda c, rnd: 1 << 20)
    B = Endpoint(be, rng, "B", b_hdrs, a_hdrs, b_iss, a_iss, [1] * n, 1, p.b_tx_ring, p.b_tx_ring - 2, p.b_rx_rings,
                 lambda size: size - 3, [p.a_rx_ring] * n, b_streams, False, p.b_quota)
    stats = dict(rounds=None, codes=np.zeros(7, dtype=np.int64), fins_sent=0, fins_seen=0, window_closed=dict(A=0, B=0),
                 max_frames=0, calls=0)
    to_b, to_a = Link(p), Link(p)
    for rnd in range(p.max_rounds):
        A.write()
        B.write()
        from_a, from_b = A.send(4 * rnd, stats), B.send(4 * rnd + 1, stats)
        at_b, at_a = to_b.carry(from_a), to_a.carry(from_b)
        B.receive(at_b, rnd, 4 * rnd + 2, stats)
        A.receive(at_a, rnd, 4 * rnd + 3, stats)
        stats["calls"] += 4
        if all(bytes(B.received[c]) == a_streams[c] for c in range(n)) and \
                all(int(t["snd_una"]) == int(t["snd_nxt"]) and int(t["ring_buffered"]) == 0 for t in A.tx):
            stats["rounds"] = rnd + 1
            break
    return A, B, stats


def check_end(A, B, stats, p=Params):
    """What a finished conversation must show (tests/test_conversation_model.py and the GPU test)."""
    n = len(p.a_streams)
    assert stats["rounds"] is not None and stats["rounds"] <= 100, "not done within 100 rounds"
    for c in range(n):
        assert bytes(B.received[c]) == A.streams[c], f"stream {c} did not arrive byte for byte"
        assert len(B.received[c]) == p.a_streams[c]
        got = bytes(A.received[c])
        assert len(got) > 0 and B.streams[c][: len(got)] == got, f"A's connection {c} did not receive a prefix"
        assert B.written[c] == p.b_stream and int(B.tx["ring_buffered"][c]) > 0, "B has run out of bytes"
        assert int(A.tx["snd_una"][c]) == int(A.tx["snd_nxt"][c]) == (A.iss[c] + p.a_streams[c] + 1) % M32
    assert stats["fins_sent"] == 3 and stats["fins_seen"] == 3 and all(A.fin_done)
    assert stats["codes"][1] > 0 and stats["codes"][2] > 0 and stats["codes"][4] > 0, stats["codes"]
    assert stats["window_closed"]["A"] >= 1
    assert int(A.tx["snd_una"][0]) < A.iss[0], "Seq of connection 0 has not crossed 2^32"
    longest = max(range(n), key=lambda c: p.a_streams[c])
    assert A.tx_wrapped[longest] and int(A.tx["ring_size"][longest]) == 8192 and all(B.rx_wrapped)
