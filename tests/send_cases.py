"""The batches of the ring send's GPU suite (tests/test_gpu_send_rings.py), built without a GPU so
that tests/test_send_host.py can show that the reference builds valid frames for every one of them.
A case is (socks, rings): a list of send_ref.sock() dicts and the uint8 array their rings lie in."""
import numpy as np

import segment_ref as sref
import send_ref as ref

ACK, FIN, PSH = ref.TX_ACK, ref.TX_FIN, ref.TX_PSH


def hdr(rng, ident=None) -> bytes:
    return sref.tcp_header(rng, ident=ident)


def wrap_sweep_positions():
    """Case 1: every read position from 4,096 - 1,000 - 20 on, so that the wrap falls at every residue of
    a 16-byte piece, of the head piece too, on chunk boundaries, not at all, and exactly at the end."""
    return range(4096 - 1000 - 20, 4096)


def wrap_sweep(rpos: int, seed=21):
    rng = np.random.default_rng(seed)
    rings = rng.integers(0, 256, 4096 + 5, dtype=np.uint8)
    s = ref.sock(hdr(rng), 100, 5, 4096, rpos, 1000, snd_nxt=int(rng.integers(0, 1 << 32)), snd_una=0, snd_wnd=0xFFFFFFFF)
    s["snd_una"] = s["snd_nxt"]
    return [s], rings


CHUNK_LENGTHS = [*range(1, 50), *range(1023, 1042), *range(2047, 2066)]


def chunk_lengths(seed=22):
    """Case 2: single-frame sockets of every head-piece length, around the 1,024-byte lane stride and
    the two-piece loop, each once unwrapped and once with the wrap one third into the chunk."""
    rng = np.random.default_rng(seed)
    socks, at = [], 3
    for c in CHUNK_LENGTHS:
        for wrapped in (False, True):
            size = c + int(rng.integers(0, 9))
            rpos = (size - max(1, c // 3)) if wrapped else int(rng.integers(0, size - c + 1))
            socks.append(ref.sock(hdr(rng), c, at, size, rpos % size, c, rcv_nxt=int(rng.integers(0, 1 << 32))))
            at += size + int(rng.integers(0, 3))
    return socks, rng.integers(0, 256, at, dtype=np.uint8)


def tiny_rings(seed=23):
    """Case 3: full rings of 1, 2, 15, 16 and 17 bytes read from every position, cut at mss 5 and whole."""
    rng = np.random.default_rng(seed)
    socks, at = [], 0
    for size in (1, 2, 15, 16, 17):
        for rpos in range(size):
            for mss in (5, 64):
                socks.append(ref.sock(hdr(rng), mss, at, size, rpos, size))
        at += size
    return socks, rng.integers(0, 256, at, dtype=np.uint8)


def ring_at_the_end(seed=24):
    """Case 4: wrapped rings whose last byte is the last byte of `rings`."""
    rng = np.random.default_rng(seed)
    rings = rng.integers(0, 256, 1000 + 777, dtype=np.uint8)
    return [ref.sock(hdr(rng), 100, 1000, 777, 700, 500), ref.sock(hdr(rng), 1460, 1000, 777, 776, 777),
            ref.sock(hdr(rng), 33, 1777 - 16, 16, 9, 16)], rings


def window_and_flags(seed=25):
    """Case 5. mss 100, 1,000 bytes buffered, 500 in flight unless said otherwise."""
    rng = np.random.default_rng(seed)
    socks = []

    def add(buffered=1000, snd_wnd=1 << 20, flags=0, **kw):
        una = int(rng.integers(0, 1 << 32))
        kw.setdefault("snd_una", una)
        kw.setdefault("snd_nxt", (kw["snd_una"] + 500) & ref.M32)
        kw.setdefault("rcv_nxt", int(rng.integers(0, 1 << 32)))
        socks.append(ref.sock(hdr(rng), 100, 4096 * len(socks), 4096, int(rng.integers(3000, 4096)), buffered,
                              snd_wnd=snd_wnd, flags=flags, **kw))

    for room in (0, 1, 99, 100, 101, 999, 1000, 1001):
        add(snd_wnd=500 + room)
    add(snd_wnd=100)                       # in_flight > snd_wnd: a room of 0
    add(snd_wnd=100, flags=ACK)            # ... and the bare ACK that still goes out
    add(buffered=0, flags=ACK)             # FS_TX_ACK alone: one 54-byte frame
    add(flags=ACK)                         # ... changes nothing when data goes out
    add(buffered=250, flags=FIN)           # FIN on the last data segment
    add(buffered=0, flags=FIN)             # FIN on a frame of its own
    add(snd_wnd=800, flags=FIN)            # FIN held back by the window
    add(buffered=300, snd_wnd=800, flags=FIN)  # all buffered data fits the room exactly: FIN needs no room
    add(buffered=250, flags=PSH)
    add(buffered=250, flags=PSH | FIN | ACK)
    add(buffered=0, flags=PSH | ACK)       # no data segment: no PSH
    add(rcv_wnd=65535)
    add(rcv_wnd=65536)
    add(rcv_wnd=0)
    add(max_frames=1)
    add(max_frames=3, flags=FIN | PSH)     # the cap holds the FIN back, PSH marks the last segment sent
    add(snd_una=0xFFFFFE00, snd_nxt=0xFFFFFF00)            # Seq crosses 2^32 inside the socket
    add(snd_una=0xFFFFFF00, snd_nxt=0x00000010, snd_wnd=2000)  # in_flight across 2^32
    add(buffered=4, snd_una=0xFFFFFF00, snd_nxt=0xFFFFFFFC, flags=FIN)  # snd_nxt comes out as 1
    return socks, rng.integers(0, 256, 4096 * len(socks), dtype=np.uint8)


def mixed(n=300, seed=26):
    """Case 6: sockets of mixed state, a third of them, and the first and the last, with no frame."""
    rng = np.random.default_rng(seed)
    socks, at = [], 1
    for i in range(n):
        size = int(rng.choice([64, 1000, 4096, 20000]))
        mss = int(rng.choice([1, 17, 536, 1446, 1460]))
        quiet = i == 0 or (n - 1 - i) % 3 == 0
        buffered = 0 if quiet and i % 2 else int(rng.integers(1, size + 1))
        if mss <= 17:
            buffered = min(buffered, 40 * mss)
        una = int(rng.integers(0, 1 << 32))
        in_flight = int(rng.integers(0, 3000))
        wnd = in_flight - int(rng.integers(0, 2)) * min(in_flight, 7) if quiet else in_flight + int(rng.integers(1, 30000))
        flags = 0 if quiet else int(rng.choice([0, ACK, FIN, PSH, FIN | PSH]))
        socks.append(ref.sock(hdr(rng), mss, at, size, int(rng.integers(0, size)), buffered, snd_una=una,
                              snd_nxt=(una + in_flight) & ref.M32, snd_wnd=wnd, rcv_nxt=int(rng.integers(0, 1 << 32)),
                              rcv_wnd=int(rng.integers(0, 100000)), max_frames=int(rng.choice([0, 1, 2, 40])), flags=flags))
        at += size - int(rng.integers(0, 2)) * min(size, 9)  # (rings may overlap: they are only read)
    rings = rng.integers(0, 256, max(s["ring_off"] + s["ring_size"] for s in socks), dtype=np.uint8)
    assert ref.rule(socks[0])["S"] == 0 and ref.rule(socks[-1])["S"] == 0
    assert sum(ref.rule(s)["S"] == 0 for s in socks) == n // 3 + 1
    return socks, rings


def long_socket(seed=27):
    """Case 6: one socket of 4,096 frames, wrapped, its Seq crossing 2^32 and its IDs a long prand16 chain."""
    rng = np.random.default_rng(seed)
    size = 4096 * 16
    return [ref.sock(hdr(rng, ident=1), 16, 7, size, size - 5000, size, snd_una=0xFFFFF000, snd_nxt=0xFFFFF000,
                     flags=FIN | PSH)], rng.integers(0, 256, size + 7, dtype=np.uint8)


def rejected_frames(seed=28):
    """Case 7 (with an mtu of 1,514): frames above the MTU and a zero port beside frames that pass."""
    rng = np.random.default_rng(seed)
    zero = bytearray(hdr(rng))
    zero[36:38] = b"\0\0"
    socks = [ref.sock(hdr(rng), 1460, 0, 8192, 7000, 4000), ref.sock(hdr(rng), 3000, 100, 8192, 8000, 7000),
             ref.sock(bytes(zero), 40, 50, 300, 250, 100), ref.sock(hdr(rng), 1461, 3, 8000, 0, 1461)]
    return socks, rng.integers(0, 256, 8292, dtype=np.uint8)


def both_entry_point_cases():
    """The batches built through fs_send_rings_batch and, linearised, through fs_segment_batch: every
    head-piece length 1 to 49, the 1,024-byte lane stride and the two-piece loop, each unwrapped and
    wrapped; and ten frames of 100 bytes that end 20 bytes before the ring's end, wrap inside a whole
    piece of the last frame, and wrap inside the first frame's 4-byte head piece."""
    return [chunk_lengths(), *(wrap_sweep(r) for r in (3076, 3111, 4095))]


def oracle_cases():
    """Every case whose frames all pass RecvEth (case 7's are judged in the GPU test)."""
    yield from (wrap_sweep(r) for r in (3076, 3096, 3111, 3996, 4095))
    yield from (chunk_lengths(), tiny_rings(), ring_at_the_end(), window_and_flags(), mixed(), long_socket())
