"""tests/conversation.py's two endpoints with the TX side through the resident ring send
(fs_send_rings_resident) and persistent TX socket tables: the table of an endpoint is made once, every
send hands the latest receive call's socks_out and snd_out off on the device and writes the state back
(FS_TX_WRITEBACK), and between the calls the application only raises ring_buffered and sets FS_TX_FIN. The
host keeps a mirror of the table for its own bookkeeping (where to write into the TX ring, the statistics),
made as a stack on the host-socket call makes it (tx_sock_from, then socks_out into the records); after every
send the table must equal that mirror. One thing differs from tests/conversation.py by construction: the
window an endpoint advertises is its RX ring's room as the receive call left it, before the application's
reads of that round, since the hand-off takes ring_free from the call's own output.

The driver and the link are tests/conversation.py's; a back end makes the calls. ResidentModel (here) is
tests/send_resident_ref.py and tests/recv_ref.py; tests/test_gpu_resident_turn.py has the device's."""
import numpy as np

import conversation as conv
import recv_ref as rref
import send_ref
import send_resident_ref as model

M32 = conv.M32


def model_send_resident(table, rings, rx_out, seed):
    """(noise, frames_cap, send_resident_ref.expected's tuple) for a write-back send of the TX_SOCK_DTYPE array
    `table` with the RX records `rx_out` = (socks_out, snd_out) or None, into a copy of `noise`."""
    socks = conv.tx_dicts(table)
    so, sn = rx_out if rx_out is not None else (None, None)
    need = model.plan(socks, rings.size, 1 << 31, 1 << 62, 0, conv.ALIGN, rx_socks_out=so, rx_snd_out=sn)["totals"]
    cap = need["n_frames"] + 2
    noise = np.random.default_rng(seed).integers(0, 256, need["frames_bytes"] + conv.TAIL, dtype=np.uint8)
    return noise, cap, model.expected(socks, rings, 0, 0, conv.ALIGN, noise, cap, rx_socks_out=so, rx_snd_out=sn)


class ResidentModel(conv.Model):
    """The calls as the models restate them; tables and rings are numpy arrays."""

    def table(self, recs):
        return recs.copy()

    def edit(self, table, c, ring_buffered, set_flags):
        table["ring_buffered"][c] = ring_buffered
        table["flags"][c] |= set_flags

    def read_table(self, table):
        return table.copy()

    def send_resident(self, table, rings, rx_out, seed):
        _, _, (buf, off, ln, _, st, outs, totals, p) = model_send_resident(table, rings, rx_out, seed)
        assert (st == 0).all() and int(totals["n_deferred"]) == int(totals["n_invalid"]) == 0
        table[:] = send_ref.socks_of(p["after"])
        return conv.frames_of_buffer(buf, off, ln), outs

    def recv_resident(self, frames, socks, snd, rings, seed):
        snd_out, socks_out, code, st = self.recv(frames, socks, snd, rings, seed)
        return snd_out, socks_out, code, st, (socks_out, snd_out)


class ResidentEndpoint(conv.Endpoint):
    def __init__(self, be, *args, **kw):
        super().__init__(be, *args, **kw)
        self.table = be.table(self.tx)  # made once; from here on only the calls and edit() change it
        self.rx_out = None              # the latest receive call's (socks_out, snd_out), as the back end keeps them

    def write(self):
        before = self.tx.copy()
        super().write()
        for c in np.flatnonzero((self.tx["ring_buffered"] != before["ring_buffered"]) | (self.tx["flags"] != before["flags"])):
            self.be.edit(self.table, int(c), int(self.tx["ring_buffered"][c]), int(self.tx["flags"][c] & ~before["flags"][c]))

    def send(self, seed, stats):
        from seqs_amd.framesum import TX_ACK, TX_FIN

        before = self.tx  # the mirror: what the hand-off makes of the table
        frames, outs = self.be.send_resident(self.table, self.tx_rings, self.rx_out, seed)
        self.rx_out = None  # (handed off once: the table has it now)
        chain, lists = before.copy(), []
        for c, o in enumerate(outs):
            in_flight = (int(before["snd_nxt"][c]) - int(before["snd_una"][c])) % M32
            if int(before["ring_buffered"][c]) > 0 and int(o["bytes"]) == 0 and int(before["snd_wnd"][c]) <= in_flight:
                stats["window_closed"][self.name] += 1
            if int(before["ring_rpos"][c]) + int(o["bytes"]) >= int(before["ring_size"][c]):
                self.tx_wrapped[c] = True
            if int(o["n_frames"]):  # the host chain through socks_out, as tests/conversation.py's Endpoint.send
                for k in ("snd_nxt", "ring_rpos", "ring_buffered"):
                    chain[k][c] = o[k]
                chain["hdr"][c, 18], chain["hdr"][c, 19] = int(o["ip_id"]) >> 8, int(o["ip_id"]) & 0xFF
                chain["flags"][c] &= ~np.uint32(TX_ACK)
            if int(o["sent"]) == TX_FIN:
                self.fin_done[c] = True
                chain["flags"][c] &= ~np.uint32(TX_FIN)
                stats["fins_sent"] += 1
            first, count = int(o["first_frame"]), int(o["n_frames"])
            lists.append(frames[first : first + count] if count else [])
        after = self.be.read_table(self.table)
        assert np.array_equal(after, chain), f"the table differs from the host chain at {np.flatnonzero(after != chain)}"
        self.tx = after
        return lists

    def receive(self, frames, rnd, seed, stats):
        from seqs_amd import tx_sock_from

        assert frames, "every round carries frames both ways"
        self.rx["snd_nxt"] = self.tx["snd_nxt"]
        snd = rref.snd_of(*[(int(t["snd_una"]), int(t["snd_wnd"])) for t in self.tx])
        snd_out, socks_out, code, st, self.rx_out = self.be.recv_resident(frames, self.rx, snd, self.rx_rings, seed)
        assert (np.asarray(st) == 0).all(), "the link damages nothing"
        stats["codes"] += np.bincount(code, minlength=7)
        stats["max_frames"] = max(stats["max_frames"], len(frames))
        left = np.array(socks_out, copy=True)  # as the call left it: what the hand-off reads
        so = left.copy()
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
        self.tx = tx_sock_from(left, self.tx, snd_out=snd_out)  # the mirror of what the next send's hand-off does


def run(be, p=conv.Params):
    """tests/conversation.py's run() with resident endpoints."""
    saved = conv.Endpoint
    conv.Endpoint = ResidentEndpoint
    try:
        return conv.run(be, p)
    finally:
        conv.Endpoint = saved
