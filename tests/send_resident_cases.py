"""The batches of the resident ring send's GPU suite (tests/test_gpu_send_resident.py), built without a GPU
so that tests/test_send_resident_model.py can show that each reaches what it names. A case is (socks, rings)
as in tests/send_cases.py, plus what the case adds (capacities, RX records, the index)."""
import numpy as np

import send_cases as cases
import send_ref as ref
import send_resident_ref as rref

ACK, FIN, PSH = ref.TX_ACK, ref.TX_FIN, ref.TX_PSH

BOUNDARY_SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
IDLE_POSITIONS = (0, 1, 62, 63, 64, 65, 255, 256, 257)
STRIDE_FRAMES = (1, 63, 64, 65, 128, 129, 4096)


def small(rng, i, idle=False, flags=0, **kw):
    """A socket of one or two frames (mss 40, up to 70 bytes) in its own 128-byte ring; idle: nothing buffered."""
    buffered = 0 if idle else int(rng.integers(1, 71))
    return ref.sock(cases.hdr(rng), 40, 128 * i, 128, int(rng.integers(0, 128)), buffered,
                    snd_nxt=int(rng.integers(0, 1 << 32)), snd_una=0, snd_wnd=0, rcv_nxt=int(rng.integers(0, 1 << 32)),
                    flags=flags, **kw)


def finish(rng, socks):
    for s in socks:  # nothing in flight, an open window
        if s["snd_wnd"] == 0:
            s["snd_una"], s["snd_wnd"] = s["snd_nxt"], 1 << 20
    return socks, ref.filled_rings(rng, socks)


def boundary(n, idle="positions", seed=41):
    """Case 2a: n small sockets; `idle`: "positions" (IDLE_POSITIONS and the last), "alternate" or "all"."""
    rng = np.random.default_rng(seed + n)
    quiet = {"positions": lambda i: i in IDLE_POSITIONS or i == n - 1, "alternate": lambda i: i % 2 == 0,
             "all": lambda i: True}[idle]
    return finish(rng, [small(rng, i, idle=quiet(i)) for i in range(n)])


def id_strides(seed=42):
    """Case 2b: sockets of 1, 63, 64, 65, 128, 129 and 4,096 frames (mss 2), each beside a one-frame socket."""
    rng = np.random.default_rng(seed)
    socks, at = [], 3
    for S in STRIDE_FRAMES:
        size = 2 * S + 6
        socks.append(ref.sock(cases.hdr(rng), 2, at, size, int(rng.integers(0, size)), 2 * S - 1, snd_una=9, snd_nxt=9))
        at += size
        socks.append(ref.sock(cases.hdr(rng), 50, at, 64, 60, 30, snd_una=1, snd_nxt=1, flags=PSH))
        at += 64
    return socks, np.random.default_rng(seed).integers(0, 256, at, dtype=np.uint8)


def many_acks(n=65536, seed=43):
    """Case 2c: n sockets of one bare ACK each, as the TX_SOCK_DTYPE array itself (one shared one-byte ring)."""
    from seqs_amd.framesum import TX_SOCK_DTYPE

    rng = np.random.default_rng(seed)
    recs = np.zeros(n, dtype=TX_SOCK_DTYPE)
    recs["hdr"] = np.frombuffer(cases.hdr(rng), dtype=np.uint8)
    recs["hdr"][:, 18], recs["hdr"][:, 19] = np.arange(n) >> 8, np.arange(n) & 0xFF
    recs["mss"], recs["ring_size"], recs["snd_wnd"], recs["flags"] = 1460, 1, 65535, ACK
    recs["snd_nxt"] = recs["snd_una"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    recs["rcv_nxt"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return recs, np.zeros(1, dtype=np.uint8)


def capacity(seed=44):
    """Case 3: twelve sockets of 1 to 4 frames, the 4th and the 9th idle, an idle one last too."""
    rng = np.random.default_rng(seed)
    socks = []
    for i in range(12):
        idle = i in (3, 8, 11)
        s = ref.sock(cases.hdr(rng), 100, 512 * i, 512, int(rng.integers(0, 512)), 0 if idle else int(rng.integers(1, 400)),
                     snd_una=7 * i, snd_nxt=7 * i, flags=(ACK if i == 5 else 0) | (FIN if i == 10 else 0))
        socks.append(s)
    return socks, ref.filled_rings(rng, socks)


def frame_ends(socks, flags=0, align=1):
    """Per socket (F_i, B_i): the inclusive sums of step 4 (every socket of `socks` valid)."""
    F = B = 0
    ends = []
    for s in socks:
        r = ref.rule(s)
        if r["S"]:
            F, B = F + r["S"], B + rref.sock_bytes(s, r, flags, align)
        ends.append((F, B))
    return ends


def invalid_sockets():
    """Case 4: {FS_TX_BAD_* reason: the edit that makes a valid socket fail it} (the RX index apart)."""
    def hdr_edit(at, value):
        def edit(s):
            h = bytearray(s["hdr"])
            h[at] = value
            s["hdr"] = bytes(h)
        return edit

    return {
        rref.BAD_ETHERTYPE: hdr_edit(13, 0x06), rref.BAD_IHL: hdr_edit(14, 0x46), rref.BAD_PROTO: hdr_edit(23, 17),
        rref.BAD_DATA_OFFSET: hdr_edit(46, 0x60), rref.BAD_MSS: lambda s: s.update(mss=0),
        rref.BAD_SOCK_FLAGS: lambda s: s.update(flags=8), rref.BAD_MAX_FRAMES: lambda s: s.update(max_frames=4097),
        rref.BAD_RING_SIZE: lambda s: s.update(ring_size=0), rref.BAD_RING_POS: lambda s: s.update(ring_rpos=s["ring_size"]),
        rref.BAD_BUFFERED: lambda s: s.update(ring_buffered=s["ring_size"] + 1),
        # (rings_bytes of the call is the rings' size less one ring: the last ring lies outside it, inside the tensor)
        rref.BAD_RING_RANGE: lambda s: s.update(ring_off=128 * INVALID_N),
    }


INVALID_N = 9


def with_invalid(reason, at, seed=45):
    """Nine small sockets (socket 5 idle), the one at `at` failing `reason`; the rings have a tenth ring's room
    that the call's rings_bytes (128 * 9) leaves out. Returns (socks, rings, rings_bytes)."""
    rng = np.random.default_rng(seed)
    socks = [small(rng, i, idle=i == 5, flags=ACK if i == 2 else 0) for i in range(INVALID_N)]
    socks, _ = finish(rng, socks)
    invalid_sockets()[reason](socks[at])
    return socks, rng.integers(0, 256, 128 * (INVALID_N + 1), dtype=np.uint8), 128 * INVALID_N


def rx_records(n, seed=46):
    """Case 5: RX records built in numpy for n sockets (n >= 8): ring_free above 65,535, rcv_nxt across 2^32,
    a snd_una that opens room, ACK owed with and without data. Returns (socks, rings, rx_socks_out, rx_snd_out)."""
    from seqs_amd.framesum import SND_OUT_DTYPE, SOCK_OUT_DTYPE

    rng = np.random.default_rng(seed)
    socks = [small(rng, i, idle=i % 4 == 1) for i in range(n)]
    for s in socks:  # 60 bytes in flight against a window of 60: no room until the RX record opens it
        s["snd_una"], s["snd_wnd"] = (s["snd_nxt"] - 60) & ref.M32, 60
    so, sn = np.zeros(n, dtype=SOCK_OUT_DTYPE), np.zeros(n, dtype=SND_OUT_DTYPE)
    so["rcv_nxt"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    so["ring_free"] = rng.integers(0, 65536, n)
    so["ring_free"][0], so["rcv_nxt"][0] = 70000, 0xFFFFFFFF
    so["ring_free"][2], so["rcv_nxt"][2] = 65536, 3
    sn["snd_una"] = [(s["snd_nxt"] - 60) & ref.M32 for s in socks]
    sn["snd_wnd"] = 60
    sn["snd_una"][::2] = [s["snd_nxt"] for s in socks[::2]]       # every other socket's bytes are acknowledged
    sn["snd_wnd"][4] = 65535
    sn["flags"] = rng.integers(0, 4, n)                           # ACK owed on about half, FIN seen on half
    sn["flags"][1], sn["flags"][3], sn["flags"][5] = 1, 0, 1       # owed on an idle socket: a bare ACK; idle stays idle
    sn["flags"][0] |= 1                                            # owed on a socket with data
    return socks, ref.filled_rings(rng, socks), so, sn


def indices(n, n_rx, kind, seed=47):
    """rx_index of n entries into n_rx records: "identity", "permuted", "holes" (NO_RX entries) or "range"
    (entries >= n_rx among valid ones)."""
    rng = np.random.default_rng(seed)
    idx = np.arange(n, dtype=np.uint32) % n_rx
    if kind != "identity":
        idx = rng.permutation(n_rx).astype(np.uint32)[:n] if n <= n_rx else rng.integers(0, n_rx, n).astype(np.uint32)
    if kind == "holes":
        idx[[0, n // 2, n - 1]] = rref.NO_RX
    if kind == "range":
        idx[[1, n // 2]] = n_rx, 0xFFFFFFFE
        idx[n - 1] = n_rx - 1
    return idx


def writeback_turns(seed=48):
    """Case 6: a table for three turns: (socks, rings, per turn the application's edits {index: fields},
    per turn (frames_cap, RX records or None)). Socket 1 closes in turn 0 (one FIN, never a second); socket 2
    owes an ACK in turn 0 (cleared after); socket 6 owes one and is deferred in turn 1 (it keeps it for turn 2);
    socket 4 sends about 200 one-byte frames over the turns (the ID chain)."""
    rng = np.random.default_rng(seed)
    socks = [small(rng, i) for i in range(8)]
    socks, _ = finish(rng, socks)
    socks[1]["flags"] = FIN
    socks[2].update(ring_buffered=0, flags=ACK)
    socks[4].update(mss=1, ring_buffered=100, max_frames=70)
    socks[6].update(ring_buffered=0)
    rings = ref.filled_rings(rng, socks)
    edits = [{}, {6: dict(flags=ACK), 0: dict(ring_buffered=33), 4: dict(ring_buffered=128)}, {1: dict(ring_buffered=5)}]
    caps = [1000, None, 1000]  # (turn 1's cap is set by the test: one frame short of socket 6's)
    return socks, rings, edits, caps


def dicts_of(recs):
    """A TX_SOCK_DTYPE array as send_ref.sock() dicts."""
    return [dict(hdr=r["hdr"].tobytes(), **{k: int(r[k]) for k in recs.dtype.names if k != "hdr"}) for r in recs]
