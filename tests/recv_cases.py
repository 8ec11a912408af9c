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


# ==== the edge suite (tests/test_gpu_recv_edges.py) ===============================================
# What the walk carries from one round of four chunks to the next, a chunk full of constants, the half
# point where the first suite has none, a payload length above 2^15, and frames that are not slots.

# ---- a. state that changes in every chunk of rounds 2 to 5 ---------------------------------------

LONG_POSITIONS = (255, 256, 257, 319, 320, 383, 384, 447, 448, 511, 512, 513, 575, 576, 767, 768, 769, 1023, 1024, 1029)
LONG_LANE_FLOWS = [(1030, code, LONG_POSITIONS) for code in range(1, 7)]


def round_and_chunk(slot):
    """(round, chunk) of a flow's slot as recv_walk walks it: rounds of 256 slots counted from 1, four
    chunks of 64 in each."""
    return slot // 256 + 1, slot % 256 // 64


# ---- b. four long flows in one workgroup ---------------------------------------------------------

FOUR_FLOWS = ((1030, 5, LONG_POSITIONS), (522, 3, None), (321, 6, None), (70, 1, None))


@functools.lru_cache(maxsize=None)
def four_long_flows():
    """Lane flows of 1030, 522, 321 and 70 frames and of four codes, interleaved, one socket each in
    flow order: the four waves of the first workgroup walk 5, 3, 2 and 1 rounds. info['mine'][g]: the
    batch indices of flow g's frames."""
    parts = [lane_flow(*spec) for spec in FOUR_FLOWS]
    where = fref.interleave([range(len(p.frames)) for p in parts])
    socks = []
    for g, p in enumerate(parts):
        s = p.socks.copy()
        s["ring_off"] = 3 + 4100 * g
        socks.append(s)
    mine = [[i for i, (h, _) in enumerate(where) if h == g] for g in range(len(parts))]
    return RCase([parts[g].frames[k] for g, k in where], dref.socks_of(*socks), np.concatenate([p.snd for p in parts]),
                 3 + 4100 * len(parts) + 2, mine=mine, parts=parts)


# ---- c. a chunk of 64 constants ------------------------------------------------------------------

DENSE = (64, 48)


@functools.lru_cache(maxsize=None)
def dense_constants(dense=64, seed=6800):
    """150 frames of one flow. Slots 0 to dense - 1: admitted 1-byte data segments with ACK (constants
    of the scan), their Acks drawn from [snd_nxt - 900, snd_nxt] in no order, so that snd.UNA jumps
    forwards and backwards from lane to lane. From slot `dense` on three pure ACKs and a data segment in
    turn, each pure ACK a few bytes on either side of the running snd.UNA (half of a chunk's newer, half
    not, the first one newer): a lane that saw another snd.UNA would give another code. With 64 the
    snd.UNA behind 64 constants is carried into the next chunk; with 48 the lanes 48 to 63 meet 48 and
    more constants below them in their own chunk. Every frame has a window of its own."""
    rng = np.random.default_rng(seed + dense)
    hdr = fref.flow_header(rng, 0x6800 + dense)
    snd_nxt, rcv_nxt = 0x3000, M32 - 30
    una0 = snd_nxt - 500
    una, nxt, frames, windows = una0, rcv_nxt, [], [int(w) for w in rng.permutation(60000)[:150] + 1]
    newer = {}
    for lo, hi in ((dense, 64), (64, 128), (128, 150)):
        pure = [k for k in range(lo, hi) if k % 4 != 3]
        flip = [bool(f) for f in rng.permutation(len(pure)) % 2 == 0]
        if pure and not flip[0]:
            first = flip.index(True)
            flip[0], flip[first] = True, False
        newer.update(zip(pure, flip))
    for k in range(150):
        if k < dense or k % 4 == 3:
            una = snd_nxt - int(rng.integers(0 if k < dense - 1 else 50, 901))
            frames.append(frame(hdr, nxt, una, ACK | PSH, windows[k], data(rng, 1)))
            nxt += 1
        elif newer[k]:
            una += int(rng.integers(1, 6))
            frames.append(frame(hdr, nxt, una, ACK, windows[k]))
        else:
            frames.append(frame(hdr, nxt, una - int(rng.integers(0, 6)), ACK, windows[k]))
    return one_socket(hdr, frames, rcv_nxt, snd_nxt, una0, windows=windows, una=una, dense=dense)


# ---- d. half points ------------------------------------------------------------------------------

HALF_SMALL = ["data at the half point", "no pure half point"]


@functools.lru_cache(maxsize=None)
def half_small(name):
    """Admitted data segments whose Ack is exactly 2^31 behind snd_nxt: rule (c) passes them, they are
    taken and leave snd.UNA at that distance. With a pure ACK at the half point among them the chunk is
    stepped; without one the scan itself meets a snd.UNA 2^31 behind. Pinned by hand."""
    rng = np.random.default_rng(6810 + HALF_SMALL.index(name))
    hdr = fref.flow_header(rng, 0x6810 + HALF_SMALL.index(name))
    fr = [frame(hdr, 500, 1000 - HALF, ACK, 11, data(rng, 4)), frame(hdr, 504, 1000, ACK, 12),
          frame(hdr, 504, 1000 - HALF, ACK, 13, data(rng, 4)), frame(hdr, 508, 1000 - HALF, ACK, 14),
          frame(hdr, 508, 1000 - HALF - 1, ACK, 15, data(rng, 4)), frame(hdr, 508, 5, ACK, 16)]
    if name == "data at the half point":
        return one_socket(hdr, fr, 500, 1000, 1000, codes=[1, 1, 1, 2, 3, 1], delivered=[1, 0, 1, 0, 2, 0],
                          snd_out=(5, 16, 4, 1, 1, 0, 0, ref.ACK_OWED))
    # frame 4 one byte inside the half (newer than a snd.UNA 2^31 behind), frame 6 at snd_nxt
    fr[3], fr[5] = frame(hdr, 508, 1000 - HALF + 1, ACK, 14), frame(hdr, 508, 1000, ACK, 16)
    return one_socket(hdr, fr, 500, 1000, 1000, codes=[1, 1, 1, 1, 3, 1], delivered=[1, 0, 1, 0, 2, 0],
                      snd_out=(1000, 16, 5, 0, 1, 0, 0, ref.ACK_OWED))


@functools.lru_cache(maxsize=None)
def half_long():
    """400 frames: rising pure ACKs bring snd.UNA to snd_nxt at slot 389; slots 384 to 399 are a chunk
    of 16 lanes in round 2. Slot 390 is the half point (taken), 393 an admitted data segment with
    Ack == snd_nxt, 395 the half point again (taken), 396 the same Ack (a duplicate)."""
    rng = np.random.default_rng(6820)
    hdr = fref.flow_header(rng, 0x6820)
    snd_nxt, nxt, fr = 7, 500, []
    una0 = snd_nxt - 390
    for k in range(390):
        fr.append(frame(hdr, nxt, una0 + k + 1, ACK, 100 + k))
    fr += [frame(hdr, nxt, snd_nxt - HALF, ACK, 490), frame(hdr, nxt, snd_nxt - HALF + 1, ACK, 491),
           frame(hdr, nxt, snd_nxt - HALF + 2, ACK, 492), frame(hdr, nxt, snd_nxt, ACK | PSH, 493, data(rng, 3)),
           frame(hdr, nxt + 3, snd_nxt, ACK, 494), frame(hdr, nxt + 3, snd_nxt - HALF, ACK, 495),
           frame(hdr, nxt + 3, snd_nxt - HALF, ACK, 496)]
    fr += [frame(hdr, nxt + 3, snd_nxt - HALF + k, ACK, 500 + k) for k in (1, 2, 3)]
    return one_socket(hdr, fr, 500, snd_nxt, una0, at={390: 1, 393: 1, 395: 1, 396: 2}, una=(snd_nxt - HALF + 3) % M32, wnd=503)


# ---- e. payloads above 2^15 ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def jumbo():
    """Five times a data segment of the longest payload RecvEth accepts, a pure ACK at the new rcv.NXT
    and a keepalive one below it: the length the rcv.NXT scan adds is above 2^15, and rcv.NXT crosses 2^32."""
    import deliver_cases as dcases

    rng = np.random.default_rng(6830)
    hdr = fref.flow_header(rng, 0x6830)
    rcv_nxt, fr = M32 - 100_000, []
    nxt = rcv_nxt
    for k in range(5):
        fr.append(frame(hdr, nxt, 901 + 2 * k, ACK, 50 + k, data(rng, dcases.JUMBO)))
        nxt += dcases.JUMBO
        fr += [frame(hdr, nxt, 902 + 2 * k, ACK, 60 + k), frame(hdr, nxt - 1, 1000, ACK, 70 + k)]
    return one_socket(hdr, fr, rcv_nxt, 1000, 900, ring=400_000, codes=[1, 1, 5] * 5, snd_out=(910, 64, 10, 0, 0, 0, 5, ref.ACK_OWED),
                      rcv_nxt_out=227_405)


# ---- f. frames of the flow that are not slots ----------------------------------------------------

NOT_SLOTS = {"damaged pure ACKs": (63, 64), "a damaged data segment": (10, 63, 64)}


def damaged_tcp(f: bytes) -> bytes:
    """The frame with one bit of its TCP checksum field flipped."""
    b = bytearray(f)
    b[14 + 4 * (b[14] & 15) + 16] ^= 0x10
    return bytes(b)


@functools.lru_cache(maxsize=None)
def not_slots(name):
    """lane_flow(130, 2) with some of its frames damaged (RecvEth drops them: they are no slots, and
    every later frame of the flow sits that many lanes lower), interleaved with UDP frames that have
    the flow's addresses and ports and with a TCP flow that has no socket. info['mine']: the batch
    indices of the socket's frames, info['foreign']: the others, info['damaged']: indices into mine."""
    base = lane_flow(130, 2)
    rng = np.random.default_rng(6840)
    mine = list(base.frames)
    for k in NOT_SLOTS[name]:
        mine[k] = damaged_tcp(mine[k])
    udp = []
    for k in range(20):
        u = bytearray(fref.udp_frame(rng, data(rng, 5 + k)))
        u[26:38] = mine[0][26:38]  # (IHL 5 in both: the addresses and the ports)
        udp.append(bytes(u))
    other = fref.segments(rng, fref.flow_header(rng, 0x6841), 77, [9] * 30)
    groups = [mine, fref.finish(udp), fref.finish(other)]
    where = fref.interleave([range(len(g)) for g in groups])
    return RCase([groups[g][k] for g, k in where], base.socks, base.snd, base.rings_bytes,
                 mine=[i for i, (g, _) in enumerate(where) if g == 0], foreign=[i for i, (g, _) in enumerate(where) if g != 0],
                 damaged=NOT_SLOTS[name], base=base)
