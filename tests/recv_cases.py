"""The batches of the receive call's GPU suite (tests/test_gpu_recv.py), built without a GPU so that
tests/test_recv_case_builders.py can show with tests/recv_ref.py alone that every one of them reaches
what it names. A case is an RCase: the frames (a list of bytes, checksums filled), the sockets, their
send side, the size of the rings buffer, and `info`, what the builder knows of its own layout."""
import functools

import numpy as np

import deliver_ref as dref
import flows_ref as fref
import recv_ref as ref

M32, HALF = 1 << 32, 1 << 31
ACK, PSH, FIN, SYN, RST, NS = ref.ACK, ref.PSH, ref.FIN, ref.SYN, ref.RST, ref.NS


class RCase:
    def __init__(self, frames, socks, snd, rings_bytes, **info):
        self.frames, self.socks, self.snd, self.rings_bytes, self.info = frames, socks, snd, rings_bytes, info


def frame(hdr, seq, ack, flags9, window, payload=b"", options=b"", ip_options=b""):
    """One TCP segment of the flow `hdr` with its Ack, its nine flag bits and its window set at L4."""
    f = bytearray(fref.tcp_frame(hdr, seq, payload, flags9 & 0xFF, options=options, ip_options=ip_options))
    l4 = 14 + 4 * (f[14] & 15)
    f[l4 + 8 : l4 + 12] = (ack % M32).to_bytes(4, "big")
    f[l4 + 12] |= flags9 >> 8
    f[l4 + 14 : l4 + 16] = window.to_bytes(2, "big")
    return bytes(f)


def data(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def one_socket(hdr, frames, rcv_nxt, snd_nxt, snd_una, snd_wnd=777, ring=4096, rcv_wnd=65535, ring_free=None, **info):
    socks = dref.socks_of(dref.sock(dref.key_of_header(hdr), rcv_nxt, 3, ring, rcv_wnd=rcv_wnd, snd_nxt=snd_nxt,
                                    ring_wpos=ring - 5, ring_free=ring_free))
    return RCase(fref.finish(frames), socks, ref.snd_of((snd_una, snd_wnd)), ring + 9, **info)


# ---- lane and chunk positions --------------------------------------------------------------------

POSITIONS = [0, 1, 62, 63, 64, 65, 127, 128, 255, 256, 257]
LANE_FLOWS = [(n, code, None) for n in (130, 258) for code in range(1, 7)] + [(130, 1, (63,)), (258, 1, (62, 127)), (258, 2, (64,))]


@functools.lru_cache(maxsize=None)
def lane_flow(n, code, positions=None):
    """One flow of n frames with a socket: a frame of code `code` at every slot of `positions` (POSITIONS
    below n when None) among frames of another code. The others are pure ACKs whose Ack rises by one
    (code 1, each with a window of its own), every seventh a 3-byte data segment that is admitted, so
    that snd.UNA and rcv.NXT move from lane to lane and across the chunks; for code 1 they are duplicate
    ACKs, so that the window comes from the last special slot, which may lie in an earlier chunk than
    the flow's end. rcv.NXT crosses 2^32 inside the flow."""
    rng = np.random.default_rng(6100 + 10 * n + code)
    hdr = fref.flow_header(rng, 0x6100 + code)
    positions = tuple(p for p in POSITIONS if p < n) if positions is None else positions
    snd_nxt, rcv_nxt = 0x20000, M32 - 40
    una, nxt = snd_nxt - 5000, rcv_nxt
    una0, frames = una, []
    for k in range(n):
        if k in positions:
            if code == 1:
                una += 1
                frames.append(frame(hdr, nxt, una, ACK, 2000 + k))
            elif code == 2:
                frames.append(frame(hdr, nxt, una, ACK, 9))
            elif code == 3:
                frames.append(frame(hdr, nxt, snd_nxt + 1, ACK, 9))
            elif code == 4:
                frames.append(frame(hdr, nxt + 1, una + 1, ACK, 9))
            elif code == 5:
                frames.append(frame(hdr, nxt - 1, snd_nxt, ACK, 9))
            else:
                frames.append(frame(hdr, nxt, una + 1, ACK, 9, data(rng, 5000)))  # more than the ring has room for
        elif code == 1:
            frames.append(frame(hdr, nxt, una, ACK, 7))  # a duplicate
        elif k % 7 == 3:
            una += 1
            frames.append(frame(hdr, nxt, una, ACK | PSH, 1000 + k, data(rng, 3)))
            nxt += 3
        else:
            una += 1
            frames.append(frame(hdr, nxt, una, ACK, 1000 + k))
    return one_socket(hdr, frames, rcv_nxt, snd_nxt, una0, positions=positions, code=code)


# ---- composition ---------------------------------------------------------------------------------

COMPOSITIONS = ["una goes back", "duplicate keeps the window", "no ACK flag", "half alone", "half in a full chunk",
                "acks below 2^32", "rcv.NXT crosses 2^32"]


@functools.lru_cache(maxsize=None)
def composition(name):
    """Small flows, each with what it expects: info['codes'] per frame, info['una'], info['wnd'], info['flags']."""
    rng = np.random.default_rng(6200 + COMPOSITIONS.index(name))
    hdr = fref.flow_header(rng, 0x6200 + COMPOSITIONS.index(name))
    if name == "una goes back":
        # data with an old Ack sets una backwards; pure ACKs raise it again; the same old Ack, pure, is a duplicate
        fr = [frame(hdr, 500, 900, ACK, 11, data(rng, 10)), frame(hdr, 510, 900, ACK, 12), frame(hdr, 510, 950, ACK, 13),
              frame(hdr, 510, 1000, ACK, 14), frame(hdr, 510, 1000, ACK, 15)]
        return one_socket(hdr, fr, 500, 1000, 990, codes=[1, 2, 1, 1, 2], una=1000, wnd=14, flags=ref.ACK_OWED)
    if name == "duplicate keeps the window":
        fr = [frame(hdr, 500, 990, ACK, 4321), frame(hdr, 500, 989, ACK, 4322)]
        return one_socket(hdr, fr, 500, 1000, 990, codes=[2, 2], una=990, wnd=777, flags=0)
    if name == "no ACK flag":
        fr = [frame(hdr, 500, 995, 0, 100), frame(hdr, 500, 1001, PSH, 200), frame(hdr, 500, 990, ACK, 300)]
        return one_socket(hdr, fr, 500, 1000, 990, codes=[1, 1, 2], una=990, wnd=200, flags=0)
    if name == "half alone":
        # una == snd_nxt and an Ack exactly 2^31 behind: newer by the literal rule; then Acks on both sides of it
        fr = [frame(hdr, 500, 1000 - HALF - 1, ACK, 21), frame(hdr, 500, 1000 - HALF, ACK, 22), frame(hdr, 500, 1000 - HALF, ACK, 23),
              frame(hdr, 500, 1000 - HALF + 1, ACK, 24), frame(hdr, 500, 1000, ACK, 25)]
        return one_socket(hdr, fr, 500, 1000, 1000, codes=[3, 1, 2, 1, 1], una=1000, wnd=25, flags=ref.ACK_OWED)
    if name == "half in a full chunk":
        # 64 + 6 frames: rising ACKs up to una == snd_nxt at slot 30, the point at slot 31, rising again behind it
        snd_nxt, fr, codes, una = 5, [], [], 5 - 31
        for k in range(70):
            if k < 31:
                una += 1
                fr.append(frame(hdr, 500, una, ACK, 100 + k))
                codes.append(1)
            elif k == 31:
                una = snd_nxt - HALF
                fr.append(frame(hdr, 500, una, ACK, 100 + k))
                codes.append(1)
            elif k == 40:
                fr.append(frame(hdr, 500, snd_nxt - HALF, ACK, 100 + k))  # the same Ack again, una now ahead of it
                codes.append(2)
            else:
                una += 3
                fr.append(frame(hdr, 500, una, ACK, 100 + k))
                codes.append(1)
        return one_socket(hdr, fr, 500, snd_nxt, 5 - 31, codes=codes, una=una % M32, wnd=169, flags=0)
    if name == "acks below 2^32":
        fr = [frame(hdr, 500, M32 - 3, ACK, 31), frame(hdr, 500, M32 - 1, ACK, 32), frame(hdr, 500, M32 - 2, ACK, 33),
              frame(hdr, 500, 2, ACK, 34), frame(hdr, 500, 6, ACK, 35), frame(hdr, 500, 5, ACK, 36)]
        return one_socket(hdr, fr, 500, 5, M32 - 4, codes=[1, 1, 2, 1, 3, 1], una=5, wnd=36, flags=ref.ACK_OWED)
    # rcv.NXT crosses 2^32: data up to it, a pure ACK at it, data behind it, a pure ACK at the old Seq
    fr = [frame(hdr, M32 - 10, 991, ACK, 41, data(rng, 6)), frame(hdr, M32 - 4, 992, ACK, 42, data(rng, 4)),
          frame(hdr, 0, 993, ACK, 43), frame(hdr, 0, 994, ACK, 44, data(rng, 7)), frame(hdr, 7, 995, ACK, 45),
          frame(hdr, M32 - 4, 996, ACK, 46)]
    return one_socket(hdr, fr, M32 - 10, 1000, 990, codes=[1, 1, 1, 1, 1, 4], una=995, wnd=45, flags=ref.ACK_OWED)


# ---- keepalive -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def keepalives():
    """A keepalive right after data (rcv.NXT has moved), the same frame with PSH or NS added, with
    another Ack, and the old keepalive Seq."""
    rng = np.random.default_rng(6300)
    hdr = fref.flow_header(rng, 0x6300)
    fr = [frame(hdr, 499, 1000, ACK, 51), frame(hdr, 500, 995, ACK, 52, data(rng, 20)), frame(hdr, 519, 1000, ACK, 53),
          frame(hdr, 519, 1000, ACK | PSH, 54), frame(hdr, 519, 1000, ACK | NS, 55), frame(hdr, 519, 999, ACK, 56),
          frame(hdr, 499, 1000, ACK, 57), frame(hdr, 520, 1000, ACK | NS, 58)]
    return one_socket(hdr, fr, 500, 1000, 990, codes=[5, 1, 5, 4, 4, 4, 4, 1], una=1000, wnd=58, flags=ref.ACK_OWED, n_keepalive=2)


# ---- stop ----------------------------------------------------------------------------------------

STOPS = ["syn", "rst", "fin"]


@functools.lru_cache(maxsize=None)
def stops(kind):
    """SYN or RST mid-flow, or an admitted FIN: the frames from `stop` on have code 0."""
    rng = np.random.default_rng(6400 + STOPS.index(kind))
    hdr = fref.flow_header(rng, 0x6400 + STOPS.index(kind))
    flags = {"syn": SYN, "rst": RST | ACK, "fin": FIN | ACK}[kind]
    fr = [frame(hdr, 500, 991, ACK, 61, data(rng, 5)), frame(hdr, 505, 992, ACK, 62),
          frame(hdr, 505, 993, flags, 63, data(rng, 4) if kind == "fin" else b""),
          frame(hdr, 510 if kind == "fin" else 505, 994, ACK, 64), frame(hdr, 510, 995, ACK, 65, data(rng, 3))]
    if kind == "fin":
        return one_socket(hdr, fr, 500, 1000, 990, codes=[1, 1, 1, 0, 0], una=993, wnd=63, flags=ref.ACK_OWED | ref.FIN_SEEN)
    return one_socket(hdr, fr, 500, 1000, 990, codes=[1, 1, 0, 0, 0], una=992, wnd=62, flags=ref.ACK_OWED)


# ---- header geometries ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def geometries():
    """IHL x data offset in {5, 6, 15}^2, twice: a data segment and a pure ACK per geometry, so that Ack,
    flags and window are read at L4 and not at a fixed offset."""
    rng = np.random.default_rng(6500)
    hdr = fref.flow_header(rng, 0x6500)
    fr, una, nxt = [], 990, 500
    for k, (ihl, doff) in enumerate((i, d) for i in (5, 6, 15) for d in (5, 6, 15)):
        opts = dict(options=b"\x01" * (4 * (doff - 5)), ip_options=b"\x01" * (4 * (ihl - 5)))
        fr.append(frame(hdr, nxt, una + 1, ACK | PSH, 7000 + k, data(rng, k + 1), **opts))
        nxt, una = nxt + k + 1, una + 1
        fr.append(frame(hdr, nxt, una, ACK | (NS if k % 2 else 0), 7100 + k, **opts))  # a duplicate
    fr.append(frame(hdr, nxt - 1, 1000, ACK, 7200, options=b"\x01" * 40, ip_options=b"\x01" * 40))  # a keepalive
    return one_socket(hdr, fr, 500, 1000, 990, codes=[1, 2] * 9 + [5], una=999, wnd=7008, flags=ref.ACK_OWED)


# ---- random batches ------------------------------------------------------------------------------

KINDS = ["ack", "ack", "data", "data", "dup", "old data", "unsent", "ahead", "keepalive", "no flag", "wide", "half", "unsent data"]


@functools.lru_cache(maxsize=None)
def random_flows(n_flows=64, per=40, seed=6600, with_sockets=None):
    """n_flows interleaved flows of about `per` frames with a seeded mix of all kinds; rings of 64
    bytes fill up, so that code 6 occurs. Every third flow's snd_nxt lies just above 0, so that its
    Acks straddle 2^32. `with_sockets`: how many of the flows have a socket (all when None); the
    sockets are listed in reverse flow order."""
    rng = np.random.default_rng(seed)
    flows, socks, snd = [], [], []
    for f in range(n_flows):
        hdr = fref.flow_header(rng, 0x6600 + f)
        h = bytearray(hdr)
        h[26:30] = int(f + 1).to_bytes(4, "big")  # distinct keys
        hdr = bytes(h)
        snd_nxt = 7 if f % 3 == 0 else int(rng.integers(0, M32))
        una0 = (snd_nxt - int(rng.integers(1, 400))) % M32
        rcv_nxt = M32 - 100 if f % 5 == 0 else int(rng.integers(0, M32))
        una, nxt, free, frames = una0, rcv_nxt, 64, []
        for _ in range(int(rng.integers(per - 8, per + 8))):
            kind = KINDS[int(rng.integers(0, len(KINDS)))]
            wnd, size = int(rng.integers(0, 65536)), int(rng.integers(1, 30))
            dist = (snd_nxt - una) % M32
            step = int(rng.integers(0, dist + 1))
            if kind == "ack":
                frames.append(frame(hdr, nxt, una + step, ACK, wnd))
                una = (una + step) % M32
            elif kind == "data":
                frames.append(frame(hdr, nxt, una + step, ACK | PSH, wnd, data(rng, size)))
                if size <= free:
                    una, nxt, free = (una + step) % M32, (nxt + size) % M32, free - size
            elif kind == "dup":
                frames.append(frame(hdr, nxt, una - int(rng.integers(0, 3)), ACK, wnd))
            elif kind == "old data":
                back = int(rng.integers(1, 50)) if dist + 50 < HALF else 0  # (an Ack the delivery's rule (c) passes)
                frames.append(frame(hdr, nxt, una - back, ACK, wnd, data(rng, size)))
                if size <= free:
                    una, nxt, free = (una - back) % M32, (nxt + size) % M32, free - size
            elif kind == "unsent":
                frames.append(frame(hdr, nxt, snd_nxt + int(rng.integers(1, 9)), ACK, wnd))
            elif kind == "ahead":
                frames.append(frame(hdr, nxt + int(rng.integers(1, 9)), una + step, ACK, wnd, data(rng, size) if size % 2 else b""))
            elif kind == "keepalive":
                frames.append(frame(hdr, nxt - 1, snd_nxt, ACK | (PSH if size == 7 else 0), wnd))
            elif kind == "no flag":
                frames.append(frame(hdr, nxt, int(rng.integers(0, M32)), PSH if size % 2 else 0, wnd))
            elif kind == "wide":
                frames.append(frame(hdr, nxt, una + step, ACK, wnd, bytes(301)))  # above the window of 300
            elif kind == "half":
                ack = (snd_nxt - HALF + int(rng.integers(-1, 2))) % M32
                frames.append(frame(hdr, nxt, ack, ACK, wnd))
                if ref.less_than(una, ack) and ref.less_than_eq(ack, snd_nxt):
                    una = ack
            else:
                frames.append(frame(hdr, nxt, snd_nxt + 1, ACK, wnd, data(rng, size)))
        flows.append(frames)
        socks.append(dref.sock(dref.key_of_header(hdr), rcv_nxt, 2 + 65 * f, 64, rcv_wnd=300, snd_nxt=snd_nxt, ring_wpos=f % 64))
        snd.append((una0, int(rng.integers(0, 65536))))
    frames = fref.finish([flows[g][k] for g, k in fref.interleave([range(len(x)) for x in flows])])
    keep = n_flows if with_sockets is None else with_sockets
    order = list(range(keep))[::-1]
    return RCase(frames, dref.socks_of(*[socks[i] for i in order]), ref.snd_of(*[snd[i] for i in order]), 2 + 65 * n_flows + 3)


# ---- the round trip ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def round_trip():
    """Three sockets whose TX rings hold 100 bytes past snd.UNA, none of it sent, behind a window of 0:
    socket 0's window is opened by a pure ACK, socket 1's only ACK is a duplicate with a window (not
    taken: it sends nothing), socket 2 gets data, which opens its window and owes an ACK."""
    rng = np.random.default_rng(6700)
    hdrs = [fref.flow_header(rng, 0x6700 + f) for f in range(3)]
    fr = [frame(hdrs[0], 500, 995, ACK, 60), frame(hdrs[1], 500, 990, ACK, 60), frame(hdrs[2], 500, 992, ACK | PSH, 30, data(rng, 8))]
    socks = dref.socks_of(*[dref.sock(dref.key_of_header(h), 500, 1 + 65 * f, 64, snd_nxt=1000) for f, h in enumerate(hdrs)])
    return RCase(fref.finish(fr), socks, ref.snd_of((990, 0), (990, 0), (990, 0)), 200, hdrs=hdrs)
