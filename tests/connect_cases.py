"""The batches of the connect call's GPU suite (tests/test_gpu_connect.py), built without a GPU so that
tests/test_connect_case_builders.py can show with tests/connect_ref.py alone that every one of them reaches
what it names. A case is an NCase: a close case (the frames, the sockets and their send side, the rings'
size, the listeners, the slots and the closers) plus the openers, the reply flags and `info`, what the
builder knows of its own layout.

An opener's flow is written by script(): the frame named at a slot, elsewhere a filler that ends no walk
(codes 4, 5 and 10), with its trace: the code of every frame the walk handles, None from its end on."""
import functools
import itertools

import numpy as np

import accept_cases as acases
import accept_ref
import close_cases as ccases
import close_ref
import connect_ref as ref
import deliver_ref as dref
import flows_ref as fref
import recv_cases as rcases
import recv_ref

M32 = 1 << 32
ACK, PSH, FIN, SYN, RST = recv_ref.ACK, recv_ref.PSH, recv_ref.FIN, recv_ref.SYN, recv_ref.RST
POSITIONS = ccases.POSITIONS


class NCase(ccases.CCase):
    def __init__(self, frames, openers, closers=None, reply_flags=0, **kw):
        super().__init__(frames, close_ref.closers_of() if closers is None else closers, **kw)
        self.openers, self.reply_flags = openers, reply_flags


# ---- one frame by name -------------------------------------------------------------------------------------

def make(hdr, kind, iss, j=0, seq=None, window=None, options=b"", ip_options=b""):
    """The frame named `kind` for an opener whose ISS is `iss`. Window and (where the name leaves it free)
    Seq and Ack vary with j."""
    nxt, wnd = (iss + 1) % M32, (37 * j + 11) % 65536 if window is None else window
    irs = (0x9000 + 77 * j) % M32 if seq is None else seq
    f = {
        "keepalive": (M32 - 1, nxt, ACK, b""),                        # rule 1: code 5
        "rejected": (1 + j % 3, nxt, ACK, b""),                       # rule 2: code 4 (:308)
        "rejected_data": (M32 - 1, nxt, ACK | PSH, b"d" * (1 + j % 9)),   # rule 2: code 4 (:302)
        "rejected_rst": (5, 0, RST, b""),                             # rule 2 comes before rule 3
        "rst": (0, 0, RST, b""),                                      # rule 3
        "rst_ack": (0, nxt, RST | ACK, b""),
        "rst_syn": (irs, nxt, RST | SYN | ACK, b""),                  # rule 3 comes before rule 4
        "syn_data": (irs, nxt, SYN | ACK, b"early"),                  # rule 4
        "syn_fin": (irs, nxt, SYN | ACK | FIN, b""),
        "syn_psh": (irs, 0, SYN | PSH, b""),
        "bad_ack": (0, (nxt + 1 + j % 5) % M32, ACK, b""),            # rule 5: code 11 (unsent)
        "bad_ack_old": (0, iss, ACK, b""),                            # rule 5 (old)
        "bad_ack_half": (0, (nxt + (1 << 31)) % M32, ACK | PSH, b""),  # rule 5, 2^31 away
        "bad_synack": (irs, iss, SYN | ACK, b""),                     # rule 5 with SYN set
        "expected": (0, nxt, ACK, b""),                               # rule 6: code 10
        "expected_bare": (0, 0, PSH if j % 2 else 0, b""),
        "expected_fin": (0, nxt, FIN | ACK, b""),
        "synack": (irs, nxt, SYN | ACK, b""),                         # rule 7
        "syn": (irs, (j * 3) % M32, SYN, b""),                        # rule 8 (the Ack field is not read)
    }[kind]
    return rcases.frame(hdr, f[0], f[1], f[2], wnd, f[3], options, ip_options)


FILLERS = ("rejected", "keepalive", "expected", "rejected_data", "expected_bare", "expected_fin", "rejected_rst")
EVENTS = ("rst", "rst_ack", "rst_syn", "syn_data", "syn_fin", "syn_psh", "bad_ack", "bad_ack_old", "bad_ack_half", "bad_synack",
          "synack", "syn")
LOCAL_MAC, REMOTE_MAC = bytes([2, 0, 0, 0, 0, 0x21]), bytes([2, 0, 0, 0, 0, 0x42])


def opener_row(hdr, iss, rcv_wnd=8192, flags=0, ip_id=None):
    key = dref.key_of_header(hdr)
    return (key, flags, LOCAL_MAC, REMOTE_MAC, iss, rcv_wnd, (key[9] << 8 | key[10]) ^ 0x5A5A if ip_id is None else ip_id)


def script(hdr, iss, n, at=None, rcv_wnd=8192, flags=0, only=None, options=b"", ip_options=b"", **more):
    """n frames of one opener's flow and the opener's row: at slot p of `at` (a dict) the frame named at[p],
    elsewhere a filler (`only`: that filler alone). Returns (frames, row, trace) with trace[k] the code of
    frame k, None from the walk's end on."""
    at = at or {}
    frames, trace, ended = [], [], False
    for k in range(n):
        kind = at.get(k) or only or FILLERS[(k * 5 + k // len(FILLERS)) % len(FILLERS)]
        fr = make(hdr, kind, iss % M32, k, options=options, ip_options=ip_options, **more)
        frames.append(fr)
        code = None if ended else ref.code_of(iss % M32, rcv_wnd, recv_ref.fields(fr))
        if code in (ref.ENDS_RST, ref.ENDS_SYN):
            code, ended = None, True
        trace.append(code)
        ended = ended or code in (ref.TAKEN, ref.BAD_ACK)
    return frames, opener_row(hdr, iss, rcv_wnd, flags), trace


def interleaved(groups):
    return [groups[g][k] for g, k in fref.interleave(groups)]


def openers_case(flows, **info):
    """A case of openers' flows [(frames, row, trace)], their frames interleaved."""
    frames = fref.finish(interleaved([f for f, _, _ in flows]))
    return NCase(frames, ref.openers_of(*[r for _, r, _ in flows]), traces=[t for _, _, t in flows], **info)


# ---- every rule at every side of a chunk boundary ------------------------------------------------------------

# (the rule, the frame at the position, what the walk makes of it: a code, or how it ends)
RULES = [(1, "keepalive", 5), (2, "rejected", 4), (2, "rejected_data", 4), (3, "rst", "rst"), (3, "rst_syn", "rst"),
         (4, "syn_data", "syn"), (4, "syn_fin", "syn"), (5, "bad_ack", 11), (5, "bad_synack", 11), (5, "bad_ack_half", 11),
         (6, "expected", 10), (7, "synack", 1), (8, "syn", 1)]


def positions_of(n):
    return [p for p in POSITIONS if p < n]


@functools.lru_cache(maxsize=None)
def rule_at_positions(n, which):
    """One flow of n frames per position p: RULES[which]'s frame at slot p (and, for a frame that ends no
    walk, as the flow's last frame too), fillers in front of it, and behind it fillers and a SYN-ACK, which
    no walk that has ended may take. ISS and the peer's Seq of every other flow are 2^32 - 1."""
    _, kind, _ = RULES[which]
    rng = np.random.default_rng(9100 + which)
    flows = []
    for j, p in enumerate(positions_of(n)):
        iss = M32 - 1 if j % 2 else 70000 + j
        at = {n - 1: kind if kind in FILLERS else "synack", p: kind}
        if p + 2 < n - 1:
            at[p + 2] = "synack"
        flows.append(script(acases.header(rng, 0x2000 + j, port=40000 + j), iss, n, at, flags=j % 2,
                            seq=M32 - 1 if j % 2 else None))
    return openers_case(flows, kind=kind, positions=positions_of(n))


def two_events():
    """Two events in one chunk, and in lanes 63 / 0 across a chunk boundary: only the first may count."""
    rng = np.random.default_rng(9300)
    h = [acases.header(rng, 0x2200 + j, port=41000 + j) for j in range(7)]
    flows = [
        script(h[0], 1000, 70, {10: "synack", 20: "syn"}),
        script(h[1], M32 - 2, 70, {0: "syn", 1: "synack"}),
        script(h[2], 2000, 130, {63: "bad_ack", 64: "synack"}),
        script(h[3], 3000, 130, {63: "synack", 64: "bad_ack"}),
        script(h[4], 4000, 130, {64: "rst", 65: "synack"}, flags=1),
        script(h[5], 5000, 70, {5: "syn_data", 6: "synack"}),
        script(h[6], 6000, 130, {127: "synack", 128: "rst"}),
    ]
    return openers_case(flows)


def extremes():
    """ISS 2^32 - 1 and the peer's Seq 2^32 - 1; Windows 0, 1 and 65535; rcv_wnd 0, 1 and up to 2^32 - 1
    (the reply's Window is clamped); data that rule 2 passes and refuses by rcv_wnd."""
    rng = np.random.default_rng(9350)
    flows = []
    for j, (iss, seq, window, rcv_wnd, kind) in enumerate(itertools.product((M32 - 1, 0, 1 << 31), (M32 - 1, 0), (0, 1, 65535),
                                                                            (0, 1, 65536, M32 - 1), ("synack", "syn"))):
        if (j * 7) % 5 > 1:  # a fifth of the product, every value of every column among it
            continue
        h = acases.header(rng, 0x2800 + j, port=42000 + j)
        flows.append(script(h, iss, 3, {1: kind}, rcv_wnd=rcv_wnd, seq=seq, window=window))
    # SYN clear with data under small windows: code 4 at rcv_wnd 0 (:299) and where Last leaves the window
    # (:305), code 10 where it fits
    for j, (rcv_wnd, size) in enumerate(((0, 1), (1, 1), (1, 2), (5, 5), (5, 6), (4, 4))):
        h = acases.header(rng, 0x2900 + j, port=43000 + j)
        fr = rcases.frame(h, 0, 7778, ACK | (FIN if j == 5 else 0), 9, b"z" * size)
        flows.append(([fr], opener_row(h, 7777, rcv_wnd), [ref.code_of(7777, rcv_wnd, recv_ref.fields(fr))]))
    return openers_case(flows)


def send_syn():
    """FS_CN_SEND_SYN: without a flow, with a flow of rejected frames only, beside a SYN-ACK (the ACK wins),
    beside a bad Ack (the RST wins), behind an RST (the SYN goes out), and not flagged at all."""
    rng = np.random.default_rng(9360)
    h = [acases.header(rng, 0x2A00 + j, port=44000 + j) for j in range(6)]
    flows = [([], opener_row(h[0], 100, flags=1), []), script(h[1], 200, 9, flags=1), script(h[2], 300, 5, {2: "synack"}, flags=1),
             script(h[3], 400, 5, {0: "bad_ack"}, flags=1), script(h[4], 500, 5, {3: "rst"}, flags=1), script(h[5], 600, 9)]
    return openers_case(flows, replies=[ref.REPLY_SYN, ref.REPLY_SYN, ref.REPLY_ACK, ref.REPLY_RST, ref.REPLY_SYN, ref.REPLY_NONE])


@functools.lru_cache(maxsize=None)
def geometries():
    """IHL x data offset in {5, 6, 15}, crossed with the four MSS kinds, on the SYN-ACK (even flows) or the
    SYN (odd flows) and on the fillers in front of it."""
    rng = np.random.default_rng(9500)
    flows, want = [], []
    for j, (ihl, doff, kind) in enumerate(itertools.product((5, 6, 15), (5, 6, 15), acases.MSS_KINDS)):
        opts, ip_opts = acases.options_of(kind, doff - 5), bytes([1]) * (4 * (ihl - 5))
        flows.append(script(acases.header(rng, 0x2400 + j, port=45000 + j), 900 + j, 4, {2: "syn" if j % 2 else "synack"},
                            options=opts, ip_options=ip_opts))
        want.append(acases.MSS_KINDS[kind] if doff > 5 else 0)
    return openers_case(flows, mss=want)


def opener_and_listener():
    """Openers whose flow's first frame is a lone SYN to a listener's address: the accept stage takes it as
    it would without the list (a slot, a SYN-ACK), and the opener's walk takes it under rule 8."""
    rng = np.random.default_rng(9700)
    flows = []
    for j in range(3):
        h = acases.header(rng, 0x2700 + j)  # (to port 80, the listener's)
        syn = acases.syn(h, seq=333 + j, options=acases.MSS_1460)
        rest, row, _ = script(h, 50 + j, 4)
        flows.append(([syn] + rest, row, [1, None, None, None, None]))
    case = openers_case(flows)
    case.listeners = accept_ref.listeners_of((acases.local(80), acases.MAC, 0, 4))
    case.slots = acases.default_slots(4)
    return case


def mixed():
    """Openers beside sockets, closers and listeners in one batch: close_cases.established() and
    closer_and_listener() with openers' flows among their frames."""
    rng = np.random.default_rng(9750)
    est, cal = ccases.established(), ccases.closer_and_listener()
    flows = [script(acases.header(rng, 0x2B00 + j, port=46000 + j), 10 + j, 70, {p: ev})
             for j, (p, ev) in enumerate(((5, "synack"), (64, "syn"), (30, "bad_ack"), (69, "rst")))]
    mine = fref.finish(interleaved([f for f, _, _ in flows]))
    frames = interleaved([list(est.frames), list(cal.frames), mine])
    closers = np.concatenate([est.closers, cal.closers])
    return NCase(frames, ref.openers_of(*[r for _, r, _ in flows]), closers=closers, listeners=cal.listeners, slots=cal.slots,
                 socks=est.socks, snd=est.snd, rings_bytes=est.rings_bytes, traces=[t for _, _, t in flows])


def three_lists():
    """All three keyed lists in one batch: 2 listed sockets, 2 closers and 2 openers, whose six TCP flows are
    interleaved with one TCP flow and one UDP flow that match nothing, and a listener with two slots that no
    frame reaches (its SYN-ACK arrays must come back as they went in). The first socket's, the first closer's
    and the first opener's flow have 66 slots each, so each of their walks crosses a chunk boundary (three
    flows of more than 64 slots: 211 frames in all); the events lie behind it, in slots 64 and 65."""
    rng = np.random.default_rng(9780)
    snd_nxt, una = 7000, 6990
    sh = [acases.header(rng, 0x2D00 + j, port=8080) for j in range(2)]
    nxt = [M32 - 150, 500]
    # socket 0: data and pure ACKs up to a FIN in slot 64, a pure ACK in CloseWait behind it; socket 1: an RST that passes
    long_flow, seq = [], nxt[0]
    for k in range(64):
        pay = rcases.data(rng, 1 + k % 7) if k % 3 == 0 else b""
        long_flow.append(rcases.frame(sh[0], seq, una + 1 + k % 5, ACK | (PSH if pay else 0), 300 + k, pay))
        seq = (seq + len(pay)) % M32
    long_flow.append(rcases.frame(sh[0], seq, una + 3, FIN | ACK, 999))
    long_flow.append(ccases.make(sh[0], "ack", close_ref.Ctl(9, (seq + 1) % M32, 0, 0), snd_nxt, 1))
    short_flow = [rcases.frame(sh[1], nxt[1], una + 1, ACK, 300), rcases.frame(sh[1], nxt[1], 0, RST, 0),
                  rcases.frame(sh[1], nxt[1], una + 2, ACK, 301)]
    socks = dref.socks_of(*[dref.sock(dref.key_of_header(h), x, 256 * j, 256, snd_nxt=snd_nxt) for j, (h, x) in enumerate(zip(sh, nxt))])
    cf = [ccases.script(acases.header(rng, 0x2D10), 5, M32 - 3, 41, 50, 66, {3: "ack", 65: "fin_ack_nxt"}),
          ccases.script(acases.header(rng, 0x2D11), 9, 900, 41, 50, 3, {1: "fin"})]
    of = [script(acases.header(rng, 0x2D20, port=46100), 77, 66, {64: "synack"}),
          script(acases.header(rng, 0x2D21, port=46101), M32 - 1, 3, {1: "syn"}, flags=1)]
    stray = fref.flow_header(rng, 0x2D30)
    stray_tcp = [fref.tcp_frame(stray, 10, b"nobody's"), fref.tcp_frame(stray, 18, b"either")]
    udp = fref.udp_frame(rng, b"datagram 1")
    stray_udp = [udp, udp[:42] + b"datagram 2"]
    frames = fref.finish(interleaved([long_flow, cf[0][0], of[0][0], short_flow, cf[1][0], of[1][0], stray_tcp, stray_udp]))
    return NCase(frames, ref.openers_of(*[r for _, r, _ in of]), closers=close_ref.closers_of(*[r for _, r, _ in cf]), socks=socks,
                 snd=recv_ref.snd_of(*[(una, 444)] * 2), rings_bytes=512, traces=[t for _, _, t in of],
                 listeners=accept_ref.listeners_of((acases.local(81), acases.MAC, 0, 2)), slots=acases.default_slots(2))


def near_keys():
    """Opener 0 and 12 flows whose keys differ from its key in one bit (one per key byte behind the protocol),
    each a SYN-ACK that would open it: none is the opener's."""
    rng = np.random.default_rng(9800)
    h = acases.header(rng, 0x2C00, port=47000)
    frames = [make(h, "expected", 4242), make(h, "synack", 4242, 1)]
    for b, at in enumerate(range(26, 38)):
        other = bytearray(h)
        other[at] ^= 1 << (b % 8)
        frames.append(make(bytes(other), "synack", 4242, 2 + b))
    return NCase(fref.finish(frames), ref.openers_of(opener_row(h, 4242)))


# ---- scale ----------------------------------------------------------------------------------------------------

BIG = acases.BIG
BIG_OPENERS = 65536
PER = ccases.PER
BIG_ISS = 4999


def _one_frame_synacks(n, sport0=1):
    """n one-frame flows, each a SYN-ACK with Seq 77 + k and Ack BIG_ISS + 1 (every 16th: Ack BIG_ISS + 2, a
    bad one), as finished frames."""
    rng = np.random.default_rng(9850)
    base = np.frombuffer(rcases.frame(acases.header(rng, 1, port=9999), 77, BIG_ISS + 1, SYN | ACK, 1234), dtype=np.uint8)
    rows = np.tile(base, (n, 1))
    k = np.arange(n, dtype=np.uint64)
    sport = k % 60000 + sport0
    rows[:, 28], rows[:, 29] = k // 60000, 1 + (k % 250)
    rows[:, 34], rows[:, 35] = sport >> 8, sport & 0xFF
    rows[:, 38:42] = ((k + 77) % M32).astype(">u4").view(np.uint8).reshape(n, 4)
    rows[15::16, 45] += 1
    return fref.finish([r.tobytes() for r in rows])


def _openers_for(frames, flags=0):
    from seqs_amd.framesum import OPENER_DTYPE

    a = np.zeros(len(frames), dtype=OPENER_DTYPE)
    for i, fr in enumerate(frames):
        a["key"][i] = np.frombuffer(fref.flow_key(fr), dtype=np.uint8)
    a["flags"], a["iss"], a["rcv_wnd"] = flags, BIG_ISS, 8192
    a["local_mac"], a["remote_mac"] = np.frombuffer(LOCAL_MAC, dtype=np.uint8), np.frombuffer(REMOTE_MAC, dtype=np.uint8)
    a["ip_id"] = np.arange(len(frames)) & 0xFFFF
    return a


@functools.lru_cache(maxsize=None)
def big(shape):
    """65,793 frames: 65,536 openers with one SYN-ACK each (the 257 other flows have no opener), or 1,000
    openers (and 25 flows without one) beside 64 established sockets of 1,011 pure ACKs and a FIN each."""
    flows = _one_frame_synacks(BIG)
    if shape == "65536 openers":
        return NCase(flows, _openers_for(flows[:BIG_OPENERS]))
    assert shape == "1000 openers, 64 sockets"
    rng = np.random.default_rng(9900)
    hdrs = [acases.header(rng, 0x7000 + s, port=8080) for s in range(64)]
    est = [fref.finish([rcases.frame(hdrs[s], 100, 200 + j, ACK, 50) for j in range(PER - 1)] +
                       [rcases.frame(hdrs[s], 100, 1500, FIN | ACK, 50)]) for s in range(64)]
    rest = flows[: BIG - 64 * PER]
    frames, ri = [], iter(rest)
    for j in range(PER):
        for s in range(64):
            frames.append(est[s][j])
            nxt = next(ri, None)
            if nxt is not None:
                frames.append(nxt)
    frames += list(ri)
    socks = dref.socks_of(*[dref.sock(dref.key_of_header(h), 100, 8 * s, 8, snd_nxt=5000) for s, h in enumerate(hdrs)])
    return NCase(frames, _openers_for(rest[:1000], flags=1), socks=socks, snd=recv_ref.snd_of(*[(150, 9)] * 64), rings_bytes=8 * 64)


BIG_SHAPES = ("65536 openers", "1000 openers, 64 sockets")
