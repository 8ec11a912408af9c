"""The batches of the accept call's GPU suite (tests/test_gpu_accept.py), built without a GPU so that
tests/test_accept_case_builders.py can show with tests/accept_ref.py alone that every one of them reaches
what it names. A case is an ACase: the frames (a list of bytes, checksums filled), the sockets and their
send side, the size of the rings buffer, the listeners and the slots, and `info`, what the builder knows
of its own layout."""
import functools
import itertools

import numpy as np

import accept_ref as ref
import deliver_ref as dref
import flows_ref as fref
import recv_cases as rcases
import recv_ref

M32 = 1 << 32
ACK, PSH, FIN, SYN, RST, URG, ECE, CWR, NS = (recv_ref.ACK, recv_ref.PSH, recv_ref.FIN, recv_ref.SYN, recv_ref.RST,
                                              recv_ref.URG, recv_ref.ECE, recv_ref.CWR, recv_ref.NS)
LOCAL_IP, MAC = bytes([10, 0, 0, 1]), bytes([2, 0, 0, 0, 0, 1])
MSS_1460 = bytes([2, 4, 0x05, 0xB4])


class ACase:
    def __init__(self, frames, listeners, slots, socks=None, snd=None, rings_bytes=64, **info):
        self.frames, self.listeners, self.slots = frames, listeners, slots
        self.socks = dref.socks_of() if socks is None else socks
        self.snd = recv_ref.snd_of() if snd is None else snd
        self.rings_bytes, self.info = rings_bytes, info


def local(port, ip=LOCAL_IP):
    return bytes(ip) + int(port).to_bytes(2, "big")


def header(rng, sport, port=80, ip=LOCAL_IP):
    """A flow's random header whose destination is (ip, port)."""
    h = bytearray(fref.flow_header(rng, sport))
    h[30:34], h[36:38] = ip, int(port).to_bytes(2, "big")
    return bytes(h)


def syn(hdr, seq=1000, window=4096, flags9=SYN, ack=0, payload=b"", options=b"", ip_options=b""):
    return rcases.frame(hdr, seq, ack, flags9, window, payload, options, ip_options)


def udp_to(rng, port=80, ip=LOCAL_IP):
    f = bytearray(fref.udp_frame(rng, rcases.data(rng, 9)))
    f[30:34], f[36:38] = ip, int(port).to_bytes(2, "big")
    return bytes(f)


def default_slots(n, rcv_wnd=8192):
    return ref.slots_of(*[(0x1000 * (k + 1) + k, rcv_wnd, (0x100 + 7 * k) & 0xFFFF) for k in range(n)])


# ---- one listener, candidates across wave and scan-block boundaries ---------------------------------

LANE_CANDIDATES = (0, 1, 62, 63, 64, 65, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def lanes(n_slots=len(LANE_CANDIDATES)):
    """300 one-frame flows; those of LANE_CANDIDATES are SYNs to the one listener. The others, in turn:
    pure ACKs and data to the listener's address and port, UDP to them, SYNs to a port nobody listens on."""
    rng = np.random.default_rng(7100)
    frames = []
    for f in range(300):
        hdr = header(rng, 0x2000 + f)
        if f in LANE_CANDIDATES:
            frames.append(syn(hdr, seq=M32 - 3 + f, window=100 + f, options=MSS_1460 if f % 2 else b""))
        elif f % 4 == 0:
            frames.append(rcases.frame(hdr, 5, 6, ACK, 77))
        elif f % 4 == 1:
            frames.append(rcases.frame(hdr, 5, 6, ACK | PSH, 77, rcases.data(rng, 3 + f % 5)))
        elif f % 4 == 2:
            frames.append(udp_to(rng))
        else:
            frames.append(syn(header(rng, 0x2000 + f, port=81)))
    listeners = ref.listeners_of((local(80), MAC, 0, n_slots))
    return ACase(fref.finish(frames), listeners, default_slots(n_slots), candidates=LANE_CANDIDATES)


# ---- three listeners whose candidates interleave ----------------------------------------------------

@functools.lru_cache(maxsize=None)
def three_listeners():
    """SYNs to ports 80, 443 and (another address) 80 in turn, 7 + 5 + 3 of them; the listeners are listed
    in another order than their first SYNs arrive, their slot ranges in yet another, with a gap between
    them, and the second has fewer slots than candidates."""
    rng = np.random.default_rng(7200)
    other = bytes([10, 0, 0, 2])
    targets = [(80, LOCAL_IP)] * 7 + [(443, LOCAL_IP)] * 5 + [(80, other)] * 3
    order = [t for trio in itertools.zip_longest(targets[:7], targets[7:12], targets[12:]) for t in trio if t is not None]
    frames = [syn(header(rng, 0x3000 + k, port=p, ip=ip), seq=77 * k, window=k) for k, (p, ip) in enumerate(order)]
    listeners = ref.listeners_of((local(80, other), bytes([2, 0, 0, 0, 0, 3]), 12, 3),
                                 (local(80), MAC, 4, 7),
                                 (local(443), bytes([2, 0, 0, 0, 0, 2]), 0, 3))
    return ACase(fref.finish(frames), listeners, default_slots(16), n_syn=[3, 7, 5], n_accepted=[3, 7, 3])


# ---- flows that look like candidates and are none ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def near_misses():
    """Flow 0: a first SYN with a listed socket (a half-open connection's retransmitted SYN). Flow 1: a
    pure ACK, then a SYN (the SYN is its second frame). A SYN whose TCP checksum is wrong: not accepted, no
    flow. Flow 2: a plain candidate, which takes slot 0."""
    rng = np.random.default_rng(7300)
    h0, h1, h2, h3 = (header(rng, 0x4000 + k) for k in range(4))
    frames = fref.finish([syn(h0, seq=500), rcases.frame(h1, 9, 9, ACK, 5), syn(h1, seq=9), syn(h2, seq=1), syn(h3, seq=2)])
    bad = bytearray(frames[3])
    bad[50] ^= 0x40
    frames[3] = bytes(bad)
    socks = dref.socks_of(dref.sock(dref.key_of_header(h0), 501, 3, 32, snd_nxt=0x7001))
    return ACase(frames, ref.listeners_of((local(80), MAC, 0, 2)), default_slots(2), socks, recv_ref.snd_of((0x7000, 500)), 40,
                 accept_of=[ref.NONE, ref.NONE, 0])


OTHER_FLAGS = (FIN, RST, PSH, ACK, URG, ECE, CWR, NS)
GRID_GOOD = [(seq, window, rcv_wnd) for seq in (7, M32 - 1) for window in (0, 1, 65535)
             for rcv_wnd in (0, 65535, 65536, M32 - 1)]


@functools.lru_cache(maxsize=None)
def grid():
    """One-frame flows to one listener: a SYN with each of the eight other flag bits, one with Ack 1, one
    with a byte of payload (none a candidate), then GRID_GOOD's SYNs, each of which takes the slot with
    its rcv_wnd."""
    rng = np.random.default_rng(7400)
    frames = [syn(header(rng, 0x5000 + k), flags9=SYN | bit) for k, bit in enumerate(OTHER_FLAGS)]
    frames.append(syn(header(rng, 0x5010), ack=1))
    frames.append(syn(header(rng, 0x5011), payload=b"x"))
    misses = len(frames)
    frames += [syn(header(rng, 0x5100 + k), seq=seq, window=window) for k, (seq, window, _) in enumerate(GRID_GOOD)]
    slots = ref.slots_of(*[(M32 - 1 - k, rcv_wnd, k) for k, (_, _, rcv_wnd) in enumerate(GRID_GOOD)])
    return ACase(fref.finish(frames), ref.listeners_of((local(80), MAC, 0, len(GRID_GOOD))), slots, misses=misses)


# ---- header geometries and the MSS option -----------------------------------------------------------

def options_of(kind, words):
    """`words` * 4 bytes of TCP options with the MSS option `kind`: first, behind NOPs, absent, malformed."""
    room = 4 * words
    if room == 0:
        return b""
    if kind == "first":
        o = bytes([2, 4, 0x02, 0x18]) + bytes([1]) * (room - 4)
    elif kind == "behind NOPs":
        o = bytes([1]) * (room - 4) + bytes([2, 4, 0x23, 0x28])
    elif kind == "absent":
        o = bytes([3, 3, 7, 1]) + bytes([1]) * (room - 4)  # a window scale, then NOPs
    else:
        o = bytes([1]) * (room - 3) + bytes([2, 4, 0x05])  # the option runs past the header's end
    return o


MSS_KINDS = {"first": 0x0218, "behind NOPs": 0x2328, "absent": 0, "malformed": 0}


@functools.lru_cache(maxsize=None)
def geometries():
    """SYNs with IHL and data offset in {5, 6, 15}, crossed with the four MSS kinds (no options at data
    offset 5): every one a candidate."""
    rng = np.random.default_rng(7500)
    frames, want = [], []
    for k, (ihl, doff, kind) in enumerate(itertools.product((5, 6, 15), (5, 6, 15), MSS_KINDS)):
        ip_opts = bytes([1]) * (4 * (ihl - 5))
        frames.append(syn(header(rng, 0x6000 + k), seq=k, options=options_of(kind, doff - 5), ip_options=ip_opts))
        want.append(MSS_KINDS[kind] if doff > 5 else 0)
    return ACase(fref.finish(frames), ref.listeners_of((local(80), MAC, 0, len(frames))), default_slots(len(frames)), mss=want)


# ---- scale -------------------------------------------------------------------------------------------

BIG = 65793
BIG_SHAPES = ("one listener", "1000 listeners", "among established frames")


def _many_syns(ports):
    """BIG one-frame SYN flows, flow k to ports[k % len(ports)], as one array of finished frames: the
    header of flow 0 with the source port and address, the destination port and the Seq varied, both
    checksums by the C oracle."""
    rng = np.random.default_rng(7600)
    base = np.frombuffer(syn(header(rng, 1), options=MSS_1460), dtype=np.uint8)
    rows = np.tile(base, (BIG, 1))
    k = np.arange(BIG, dtype=np.uint64)
    sport = k % 60000 + 1  # (never 0: RecvEth drops a zero port)
    rows[:, 28], rows[:, 29] = k // 60000, 1 + (k % 250)
    rows[:, 34], rows[:, 35] = sport >> 8, sport & 0xFF
    port = np.asarray(ports, dtype=np.uint32)[k % len(ports)]
    rows[:, 36], rows[:, 37] = port >> 8, port & 0xFF
    rows[:, 38:42] = (k * 2654435761 % M32).astype(">u4").view(np.uint8).reshape(BIG, 4)
    return fref.finish([r.tobytes() for r in rows])


@functools.lru_cache(maxsize=None)
def big(shape):
    assert shape in BIG_SHAPES
    if shape == "one listener":
        return ACase(_many_syns([80]), ref.listeners_of((local(80), MAC, 0, 65536)), default_slots(65536), n_full=BIG - 65536)
    if shape == "1000 listeners":
        ports = list(range(1000, 2000))
        per = 65  # 65,793 SYNs over 1000 ports: 65 or 66 each; the first 793 ports are one slot short
        listeners = ref.listeners_of(*[(local(p), MAC, per * k, per) for k, p in enumerate(ports)])
        return ACase(_many_syns(ports), listeners, default_slots(per * 1000), n_full=793)
    # 64 sockets' flows of 1024 pure ACKs each, the SYN flows between their frames
    rng = np.random.default_rng(7700)
    syns = _many_syns([80])
    hdrs = [header(rng, 0x7000 + s, port=8080) for s in range(64)]
    est = [[rcases.frame(hdrs[s], 100, 200 + j, ACK, 50) for j in range(1024)] for s in range(64)]
    est = [fref.finish(flow) for flow in est]
    frames, si = [], iter(syns)
    for j in range(1024):
        for s in range(64):
            frames.append(est[s][j])
            frames.append(next(si))
    frames += list(si)
    socks = dref.socks_of(*[dref.sock(dref.key_of_header(h), 100, 8 * s, 8, snd_nxt=5000) for s, h in enumerate(hdrs)])
    snd = recv_ref.snd_of(*[(150, 9)] * 64)
    return ACase(frames, ref.listeners_of((local(80), MAC, 0, 65536)), default_slots(65536), socks, snd, 8 * 64, n_full=BIG - 65536)
