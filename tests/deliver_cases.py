"""The batches of the in-order delivery's edge suite (tests/test_gpu_deliver_edges.py), built without a
GPU so that tests/test_deliver_case_builders.py can show with tests/deliver_ref.py alone that every one
of them reaches what it names. A case is a Case: the batch (buf, off, ln), the sockets, the size of the
rings buffer, the RX flags, and `info`, what the builder knows of its own layout. Every ring lies inside
the rings buffer with at least one sentinel byte before the first and behind the last ring."""
import functools

import numpy as np

import deliver_ref as ref
import flows_ref as fref

ACK, FIN, PSH, SYN, RST = fref.ACK, fref.FIN, fref.PSH, ref.SYN, ref.RST
M32 = 1 << 32
JUMBO = 65481  # the longest TCP payload RecvEth accepts (tests/test_gpu_large_offsets.py)


class Case:
    def __init__(self, batch, socks, rings_bytes, flags=0, **info):
        self.batch, self.socks, self.rings_bytes, self.flags, self.info = batch, socks, rings_bytes, flags, info


def reference(case, seed=0):
    """deliver_ref.expected of the case over the buffers test_gpu_deliver.check(..., payload=False,
    seed=seed) makes: usable as that call's `e`."""
    from test_gpu_deliver import TAIL, sentinel

    noise = np.random.default_rng(77 + seed).integers(0, 256, 3 + TAIL, dtype=np.uint8)
    return ref.expected(*case.batch, 0, case.flags, noise, 3, 0, case.socks, sentinel(case.rings_bytes, seed))


# ---- uniform frames with numpy -------------------------------------------------------------------

def big_batch(flow_of, seed, patch=None):
    """One 64-byte TCP segment (10 bytes of payload) per entry of flow_of, back to back; a flow's
    segments continue each other in batch order. Built with numpy, checksums by the C oracle.
    `patch(frames, seq)`: called with the (n, 64) frame array and the Seq of every frame before the
    checksums are filled; it may rewrite flags and Seq (put_seq)."""
    from oracle import coracle

    rng = np.random.default_rng(seed)
    n, n_flows = flow_of.size, int(flow_of.max()) + 1
    hdr = rng.integers(0, 256, (n_flows, 54), dtype=np.uint8)
    ids = np.arange(n_flows, dtype=np.uint32)
    hdr[:, 12], hdr[:, 13], hdr[:, 14], hdr[:, 23], hdr[:, 46], hdr[:, 47] = 8, 0, 0x45, 6, 0x50, ACK
    hdr[:, 16], hdr[:, 17] = 0, 50
    for k in range(4):  # distinct keys: the flow's number is its source address
        hdr[:, 26 + k] = (ids >> (24 - 8 * k)) & 0xFF
    hdr[:, 34:38] = [0x10, 0x01, 0x00, 0x50]
    frames = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    frames[:, :54] = hdr[flow_of]
    by_flow = np.argsort(flow_of, kind="stable")
    start = np.searchsorted(flow_of[by_flow], np.arange(n_flows))
    rank = np.empty(n, dtype=np.int64)
    rank[by_flow] = np.arange(n) - start[flow_of[by_flow]]
    seq = (rng.integers(0, 1 << 32, n_flows, dtype=np.int64)[flow_of] + 10 * rank) % (1 << 32)
    put_seq(frames, seq)
    frames[:, 18:20] = rng.integers(0, 256, (n, 2), dtype=np.uint8)
    if patch is not None:
        patch(frames, seq)
    buf = np.concatenate([frames.reshape(-1), rng.integers(0, 256, 64, dtype=np.uint8)])
    off = np.arange(n, dtype=np.uint64) * np.uint64(64)
    ln = np.full(n, 64, dtype=np.uint32)
    coracle.fill_batch(buf, off, ln, 0, coracle.FILL_CSUM)
    return buf, off, ln


def put_seq(frames, seq):
    for k in range(4):
        frames[:, 38 + k] = ((seq % M32) >> (24 - 8 * k)) & 0xFF


def be32(cols):
    c = cols.astype(np.int64)
    return (c[:, 0] << 24) | (c[:, 1] << 16) | (c[:, 2] << 8) | c[:, 3]


def socks_at(buf, off, heads, rcv_nxt, ring_off, ring_size, ring_wpos, ring_free=None):
    """One socket per frame index in `heads` (IHL 5), its key and snd_nxt (the frame's Ack) from that
    frame; the other fields are arrays or scalars."""
    from seqs_amd.framesum import SOCK_DTYPE

    at = off[np.asarray(heads, dtype=np.int64)].astype(np.int64)
    h = buf[at[:, None] + np.arange(54)[None, :]]
    s = np.zeros(at.size, dtype=SOCK_DTYPE)
    s["key"][:, 0], s["key"][:, 1:9], s["key"][:, 9:13] = h[:, 23], h[:, 26:34], h[:, 34:38]
    s["rcv_nxt"], s["snd_nxt"], s["rcv_wnd"] = np.asarray(rcv_nxt) % M32, be32(h[:, 42:46]), 65535
    s["ring_off"], s["ring_size"], s["ring_wpos"] = ring_off, ring_size, ring_wpos
    s["ring_free"] = s["ring_size"] if ring_free is None else ring_free
    return s


def sock_of(frame: bytes, rcv_nxt, ring_off, ring_size, **kw):
    """A socket of the flow of `frame` (any IHL), whose snd_nxt is the frame's Ack."""
    l4 = 14 + 4 * (frame[14] & 15)
    kw.setdefault("snd_nxt", int.from_bytes(frame[l4 + 8 : l4 + 12], "big"))
    return ref.sock(fref.flow_key(frame), rcv_nxt, ring_off, ring_size, **kw)


def seq_of(frame: bytes) -> int:
    l4 = 14 + 4 * (frame[14] & 15)
    return int.from_bytes(frame[l4 + 4 : l4 + 8], "big")


def check_layout(socks, rings_bytes):
    """Every ring inside the buffer with sentinel on both sides of the whole, no two overlapping."""
    lo, size = socks["ring_off"].astype(np.int64), socks["ring_size"].astype(np.int64)
    by = np.argsort(lo)
    assert (size >= 1).all() and (socks["ring_wpos"] < socks["ring_size"]).all() and (socks["ring_free"] <= socks["ring_size"]).all()
    assert int(lo.min()) >= 1 and int((lo + size).max()) + 1 <= rings_bytes
    assert ((lo + size)[by][:-1] <= lo[by][1:]).all()


# ---- a. a long flow beside another flow ----------------------------------------------------------

LANE_LENGTHS = [*range(257, 191, -1), 1, 2, 64]


@functools.lru_cache(maxsize=None)
def flow_ends_at_every_lane(interleaved=False):
    """69 flows of 10-byte segments, each with a socket: lengths 257 down to 192 (the flow's fourth
    chunk ends at every lane, at 256 with the round of four chunks, at 257 one slot into the next), then
    1, 2 and 64. Contiguous, so that each flow's slots are followed by the next flow's head, or dealt
    round-robin. Every ring is short by one frame: the flow's last frame is dropped."""
    lengths = LANE_LENGTHS
    if interleaved:
        flow_of = np.array([g for g, _ in fref.interleave([range(c) for c in lengths])], dtype=np.int64)
    else:
        flow_of = np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)
    buf, off, ln = big_batch(flow_of, 310 + int(interleaved))
    heads = np.array([int(np.flatnonzero(flow_of == f)[0]) for f in range(len(lengths))])
    size = np.array([10 * (c - 1) if c > 1 else 5 for c in lengths], dtype=np.int64)
    ring_off = 3 + np.concatenate([[0], np.cumsum(size + 1)[:-1]])  # one sentinel byte between neighbours
    frames = buf[: flow_of.size * 64].reshape(-1, 64)
    socks = socks_at(buf, off, heads, be32(frames[heads, 38:42]), ring_off, size, (size * 3) // 4)
    rings_bytes = int(ring_off[-1] + size[-1]) + 9
    check_layout(socks, rings_bytes)
    return Case((buf, off, ln), socks, rings_bytes, lengths=lengths, flow_of=flow_of)


# ---- b. FIN, SYN, RST and an out-of-order frame at the chunk positions ---------------------------

EVENTS = ["fin", "fin dropped", "syn", "rst", "out of order"]
POSITIONS = [0, 1, 62, 63, 64, 65, 127, 128, 191, 192, 255, 256, 257, 319, 320, 329]
EVENT_FLOW, EVENT_LEAD = 330, 37


@functools.lru_cache(maxsize=None)
def events_at_chunk_positions():
    """One flow of 330 ten-byte segments and one socket per (event, position), each behind a 37-frame
    flow without a socket (so no walk starts at slot 0 or on a multiple of 64). The frames behind an
    admitted FIN carry Seq + 1: they would be admitted if the walk went on. Behind a dropped FIN (Seq =
    nxt + 1) and behind an out-of-order frame (Seq = nxt + 5) the flow continues at nxt."""
    pairs = [(ev, p) for ev in EVENTS for p in POSITIONS]
    per = EVENT_LEAD + EVENT_FLOW
    flow_of = np.concatenate([np.repeat([2 * j, 2 * j + 1], [EVENT_LEAD, EVENT_FLOW]) for j in range(len(pairs))]).astype(np.int64)
    heads = np.array([j * per + EVENT_LEAD for j in range(len(pairs))])
    keep = {}

    def patch(frames, seq):
        keep["seq0"] = seq[heads].copy()
        for j, (ev, p) in enumerate(pairs):
            g, end = int(heads[j]) + p, int(heads[j]) + EVENT_FLOW
            if ev == "fin":
                frames[g, 47] = ACK | FIN
                seq[g + 1 : end] += 1
            elif ev == "fin dropped":
                frames[g, 47] = ACK | FIN
                seq[g] += 1
                seq[g + 1 : end] -= 10
            elif ev == "syn":
                frames[g, 47] = SYN
            elif ev == "rst":
                frames[g, 47] = RST | ACK
            else:
                seq[g] += 5
                seq[g + 1 : end] -= 10
        put_seq(frames, seq)

    buf, off, ln = big_batch(flow_of, 320, patch)
    size = np.full(len(pairs), 10 * EVENT_FLOW + 7, dtype=np.int64)
    ring_off = 2 + np.arange(len(pairs), dtype=np.int64) * (size[0] + 1)
    socks = socks_at(buf, off, heads, keep["seq0"], ring_off, size, np.arange(len(pairs)) * 41 % size[0])
    rings_bytes = int(ring_off[-1] + size[-1]) + 5
    check_layout(socks, rings_bytes)
    return Case((buf, off, ln), socks, rings_bytes, pairs=pairs, heads=heads)


# ---- c. restart patterns -------------------------------------------------------------------------

PATTERNS = ["all duplicates", "alternating", "drops at 63 64 127 128 129"]
PATTERN_FLOW = 200
# the count of marks equal to 2, and to 1, in each chunk of 64 slots (the last chunk has 8)
PATTERN_DROPS = {"all duplicates": [64, 64, 64, 8], "alternating": [32, 32, 32, 4], "drops at 63 64 127 128 129": [1, 2, 2, 0]}
PATTERN_ADMITTED = {"all duplicates": [0, 0, 0, 0], "alternating": [32, 32, 32, 4], "drops at 63 64 127 128 129": [63, 62, 62, 8]}


def pattern_frames(rng, name, hdr, nxt):
    data = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    out = []
    for k in range(PATTERN_FLOW):
        if name == "all duplicates":
            out.append(fref.tcp_frame(hdr, nxt - 10, data(10)))
        elif name == "alternating":
            out.append(fref.tcp_frame(hdr, nxt if k % 2 == 0 else nxt - 10, data(10)))
            nxt += 10 if k % 2 == 0 else 0
        else:
            drop = k in (63, 64, 127, 128, 129)
            out.append(fref.tcp_frame(hdr, nxt + 1 if drop else nxt, data(10)))
            nxt += 0 if drop else 10
    return out


@functools.lru_cache(maxsize=None)
def restart_patterns():
    """Three flows of 200 frames, contiguous, each with a socket: every frame a duplicate of delivered
    bytes (all 64 lanes of three chunks running are dropped), in-order frames and duplicates in turn (a
    restart at every second lane), and drops at the last lane of a chunk and the first lanes of the next.
    (Pure ACKs, a ring that fills and frames above the window are test_gpu_deliver.mixed_flow's.)"""
    rng = np.random.default_rng(330)
    frames, socks, at = [], [], 1
    for j, name in enumerate(PATTERNS):
        hdr = fref.flow_header(rng, 0x3300 + j)
        nxt = int(rng.integers(0, 1 << 32))
        mine = pattern_frames(rng, name, hdr, nxt)
        size = 4001
        socks.append(sock_of(mine[0], nxt, at, size, ring_wpos=3990 - j))
        frames += mine
        at += size + j % 2
    frames = fref.finish(frames)
    socks = ref.socks_of(*socks)
    check_layout(socks, at + 3)
    return Case(fref.pack(frames, lead=1), socks, at + 3, frames=frames)


# ---- d. and e. the split at the wrap -------------------------------------------------------------

def split_key(length, first):
    """What (len, min(len, ring_size - ring_wpos)) is for a payload placed `first` bytes before the
    ring's end: first = 0 stands for ring_wpos = 0."""
    return (length, length if first == 0 else first)


SMALL_SPLITS = [(n, first) for n in range(1, 41) for first in range(n + 1)]


@functools.lru_cache(maxsize=None)
def wrap_splits_small():
    """860 sockets with one data frame each: every payload length 1..40 landing `first` = 0..len bytes
    before its ring's end, over ring sizes len, len + 1, 97 and 4,099, neighbouring rings touching or one
    sentinel byte apart (so ring_off takes every residue of 16), the frames back to back."""
    rng = np.random.default_rng(340)
    frames, socks, at = [], [], 5
    for i, (n, first) in enumerate(SMALL_SPLITS):
        size = (n, n + 1, 97, 4099)[i % 4]
        hdr = fref.flow_header(rng, 0x4000 + i)
        seq = int(rng.integers(0, 1 << 32))
        f = fref.tcp_frame(hdr, seq, rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        socks.append(sock_of(f, seq, at, size, ring_wpos=(size - first) % size))
        frames.append(f)
        at += size + (i // 3) % 2
    socks = ref.socks_of(*socks)
    check_layout(socks, at + 2)
    return Case(fref.pack(fref.finish(frames), lead=3), socks, at + 2, splits=[split_key(*s) for s in SMALL_SPLITS])


LARGE_LENGTHS = [1023, 1024, 1025, 1460, 4111, 8960, JUMBO]
RING_RESIDUES = [0, 1, 7, 12]


def large_firsts(n):
    return [1, 15, 16, 17, n - 17, n - 16, n - 1, 0]  # 0: a placement that does not wrap


@functools.lru_cache(maxsize=None)
def wrap_splits_large():
    """224 single-frame sockets: the lengths around copy_payload's 1,024-byte trip and the jumbo, each
    split at the wrap 1, 15, 16, 17 bytes from either end and not at all, at four ring_off residues of
    16. Then one flow of 64 in-order jumbo segments into a ring with room for 40 (one chunk whose scan
    sum is 4.19 MB), and a jumbo FIN against a window of its length and of its length + 1."""
    rng = np.random.default_rng(350)
    frames, socks, splits, at = [], [], [], 16
    data = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731

    def place(size, residue):
        nonlocal at
        at += 1 + (residue - (at + 1)) % 16
        lo = at
        at += size
        return lo

    for n in LARGE_LENGTHS:
        for first in large_firsts(n):
            for r in RING_RESIDUES:
                size = n + 33 + r
                seq = int(rng.integers(0, 1 << 32))
                f = fref.tcp_frame(fref.flow_header(rng, 0x5000 + len(frames)), seq, data(n))
                wpos = 7 if first == 0 else size - first
                socks.append(sock_of(f, seq, place(size, r), size, ring_wpos=wpos))
                splits.append((n, n if first == 0 else first))
                frames.append(f)
    jumbo_at = len(frames)
    hdr = fref.flow_header(rng, 0x5F00)
    seq = M32 - 20 * JUMBO  # Seq wraps inside the admitted part
    frames += fref.segments(rng, hdr, seq, [JUMBO] * 64)
    size = 40 * JUMBO + 100
    socks.append(sock_of(frames[jumbo_at], seq, place(size, 5), size, ring_wpos=size - 1000))
    for wnd in (JUMBO, JUMBO + 1):
        seq = int(rng.integers(0, 1 << 32))
        f = fref.tcp_frame(fref.flow_header(rng, 0x5F10 + wnd - JUMBO), seq, data(JUMBO), flags=ACK | FIN)
        socks.append(sock_of(f, seq, place(JUMBO + 9, 3), JUMBO + 9, ring_wpos=JUMBO - 20, rcv_wnd=wnd))
        frames.append(f)
    socks = ref.socks_of(*socks)
    check_layout(socks, at + 16)
    return Case(fref.pack(fref.finish(frames), lead=2), socks, at + 16, splits=splits, jumbo_at=jumbo_at, jumbo_sock=224)


@functools.lru_cache(maxsize=None)
def jumbo_flow():
    """(e)'s flow of 64 jumbo segments alone, for the host form: the ring starts at 4,099 of a rings
    array with caller bytes before and behind it, a second small ring (without a flow) further on."""
    big = wrap_splits_large()
    buf, off, ln = big.batch
    j = big.info["jumbo_at"]
    s = big.socks[big.info["jumbo_sock"] : big.info["jumbo_sock"] + 1].copy()
    s["ring_off"] = 4099
    other = ref.sock(bytes([6]) + bytes(range(12)), 1, 4099 + int(s["ring_size"][0]) + 333, 64)
    socks = ref.socks_of(s, other)
    lo, hi = int(off[j]), int(off[j + 63]) + int(ln[j + 63])
    return Case((buf[lo - 2 : hi + 64].copy(), off[j : j + 64] - np.uint64(lo - 2), ln[j : j + 64].copy()), socks,
                4099 + int(s["ring_size"][0]) + 333 + 64 + 500)


# ---- f. header geometries ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def header_geometries(fcs=False):
    """One flow of 121 in-order segments, one per (IHL 5..15, data offset 5..15), payloads of 1..121
    bytes, then the flow's FIN under IHL 15 and data offset 15. The frames only (with their FCS when
    `fcs`): header_case packs them at a lead."""
    rng = np.random.default_rng(360)
    hdr = fref.flow_header(rng, 0x6000)
    seq0 = M32 - 3000  # Seq wraps inside the flow
    frames, seq = [], seq0
    for k, (ihl, doff) in enumerate((i, d) for i in range(5, 16) for d in range(5, 16)):
        frames.append(fref.tcp_frame(hdr, seq, rng.integers(0, 256, k + 1, dtype=np.uint8).tobytes(), ident=k,
                                     options=b"\x01" * (4 * (doff - 5)), ip_options=b"\x01" * (4 * (ihl - 5))))
        seq += k + 1
    frames.append(fref.tcp_frame(hdr, seq, b"", flags=ACK | FIN, ident=121, options=b"\x01" * 40, ip_options=b"\x01" * 40))
    return hdr, seq0, fref.finish(frames, fcs=fcs)


def header_case(fcs, lead):
    hdr, seq0, frames = header_geometries(fcs)
    total = 121 * 122 // 2
    socks = ref.socks_of(sock_of(frames[0], seq0, 6, total + 40, ring_wpos=total - 500))
    return Case(fref.pack(frames, lead=lead), socks, total + 40 + 13, fref.RX_FCS if fcs else 0)


# ---- g. near-miss keys ---------------------------------------------------------------------------

KEY_AT = [26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37]  # the 12 key bytes of a TCP frame behind the protocol


@functools.lru_cache(maxsize=None)
def near_miss_keys():
    """Socket 0 and 13 TCP flows whose keys differ from its key in one bit (one per key byte behind the
    protocol, bits 0..7 in turn, and a second bit of the last byte), a UDP flow with its addresses and
    ports, then its own flow. Socket 1's flow has its first batch frame damaged: the flow's head is its
    second frame. Every frame of socket 2's flow is damaged."""
    rng = np.random.default_rng(370)
    base = fref.flow_header(rng, 0x7000)
    frames = []
    for j, at in enumerate(KEY_AT + [37]):
        h = bytearray(base)
        h[at] ^= 1 << (j % 8) if j < 12 else 0x80
        frames += fref.segments(rng, bytes(h), 500, [20, 20])
    u = bytearray(fref.udp_frame(rng, b"a datagram of the same addresses and ports"))
    u[26:38] = base[26:38]
    frames.append(bytes(u))
    hb, hc = fref.flow_header(rng, 0x7100), fref.flow_header(rng, 0x7200)
    b = fref.segments(rng, hb, 9000, [30, 31, 32])
    c = fref.segments(rng, hc, 100, [8, 9])
    own = fref.segments(rng, base, 500, [20, 21, 22])
    frames += [b[0], c[0], b[1], c[1], b[2]] + own
    frames = fref.finish(frames)
    n_miss = 27
    for i in (n_miss, n_miss + 1, n_miss + 3):  # b[0] and both of c
        f = bytearray(frames[i])
        f[56] ^= 0x80
        frames[i] = bytes(f)
    socks = ref.socks_of(sock_of(own[0], 500, 3, 100, ring_wpos=90), sock_of(b[1], 9030, 104, 64, ring_wpos=60),
                         sock_of(c[0], 100, 169, 32, ring_wpos=5))
    check_layout(socks, 205)
    return Case(fref.pack(frames, lead=1), socks, 205)


# ---- h. more than 65,536 frames ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def big_batches(shape):
    """65,793 ten-byte segments in the three shapes of test_gpu_flows.BIG_SHAPES: one flow into one ring
    that wraps once and takes every byte; 1,000 flows with their sockets listed in reverse flow order;
    every frame a flow of its own with 65,536 sockets (the maximum) of 16-byte rings, the last 257 flows
    without one."""
    from test_gpu_flows import BIG, BIG_SHAPES

    flow_of = BIG_SHAPES[shape]()
    if shape == "1000 flows":
        flow_of[:1000] = np.random.default_rng(7).permutation(1000)  # (every flow present)
    buf, off, ln = big_batch(flow_of, 380 + len(shape))
    frames = buf[: BIG * 64].reshape(-1, 64)
    if shape == "one flow":
        socks = socks_at(buf, off, [0], be32(frames[:1, 38:42]), 11, 700001, 699990)
        rings_bytes = 700001 + 30
    elif shape == "1000 flows":
        heads = np.arange(1000)  # the first 1,000 frames open the 1,000 flows: flow f's head is frame f
        count = np.bincount(flow_of, minlength=1000)[flow_of[:1000]]
        size = 10 * count + 3
        ring_off = 1 + np.concatenate([[0], np.cumsum(size + 1)[:-1]])
        socks = socks_at(buf, off, heads, be32(frames[heads, 38:42]), ring_off, size, size - 5)[::-1].copy()
        rings_bytes = int(ring_off[-1] + size[-1]) + 4
    else:
        heads = np.arange(65536)
        socks = socks_at(buf, off, heads, be32(frames[heads, 38:42]), 1 + 16 * heads, 16, heads % 16)
        rings_bytes = 1 + 16 * 65536 + 1
    check_layout(socks, rings_bytes)
    return Case((buf, off, ln), socks, rings_bytes, flow_of=flow_of)


# ---- 40 chained calls ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def chained_calls(n_calls=40):
    """Three flows' segments (1..60 bytes) dealt round-robin and cut into 40 consecutive batches of 5
    and 300 frames in turn. Call j's sockets are call j - 1's expected state with ring_free reset to
    the ring's size (the application has read everything). Returns (the rings buffer before call 0,
    [(batch, socks, expected) per call]), the expected dicts by deliver_ref applied in sequence."""
    from test_gpu_deliver import TAIL, sentinel

    rng = np.random.default_rng(390)
    sizes = [5 if j % 2 == 0 else 300 for j in range(n_calls)]
    total = sum(sizes)
    hdrs = [fref.flow_header(rng, 0x9000 + f) for f in range(3)]
    seq0 = [M32 - 5000, 77, int(rng.integers(0, 1 << 32))]
    per = [total // 3 + (1 if f < total % 3 else 0) for f in range(3)]
    segs = [fref.segments(rng, hdrs[f], seq0[f], [int(x) for x in rng.integers(1, 61, per[f])]) for f in range(3)]
    frames = fref.finish([segs[g][k] for g, k in fref.interleave([range(c) for c in per])])
    ring_sizes = [4096, 5000, 20011]
    at, socks = 7, []
    for f in range(3):
        socks.append(sock_of(segs[f][0], seq0[f], at, ring_sizes[f], ring_wpos=ring_sizes[f] - 3 - f))
        at += ring_sizes[f] + f
    socks = ref.socks_of(*socks)
    # 150 sockets without a flow, listed in the long calls only: the staged blocks differ in size
    idle = ref.socks_of(*[ref.sock(bytes([6, 0xEE]) + i.to_bytes(2, "big") + bytes(9), i, at + 9 * i, 8, ring_wpos=i % 8)
                          for i in range(150)])
    rings_bytes = at + 9 * 150 + 5
    check_layout(np.concatenate([socks, idle]), rings_bytes)
    rings, calls, k = sentinel(rings_bytes, 39), [], 0
    for j, c in enumerate(sizes):
        listed = np.concatenate([socks, idle]) if c == 300 else socks
        batch = fref.pack(frames[k : k + c], lead=j % 5, seed=j)
        noise = np.random.default_rng(j).integers(0, 256, 3 + TAIL, dtype=np.uint8)
        e = ref.expected(*batch, 0, 0, noise, 3, 0, listed, rings)
        calls.append((batch, listed, e))
        rings = e["rings"]
        nxt, so = socks.copy(), e["socks_out"][:3]
        nxt["rcv_nxt"], nxt["ring_wpos"], nxt["ring_free"] = so["rcv_nxt"], so["ring_wpos"], nxt["ring_size"]
        socks, k = nxt, k + c
    return sentinel(rings_bytes, 39), calls
