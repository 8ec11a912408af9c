"""The batches of the close call's GPU suite (tests/test_gpu_close.py), built without a GPU so that
tests/test_close_case_builders.py can show with tests/close_ref.py alone that every one of them reaches what
it names. A case is a CCase: an accept case (the frames, the sockets and their send side, the rings' size,
the listeners and the slots) plus the closers and `info`, what the builder knows of its own layout.

A closer's flow is written by script(): frame by frame it follows the connection with close_ref's rule, so
that the frames it makes are the ones their names say under the state they meet -- a filler that is no
event in that state, or the event asked for at that slot."""
import functools

import numpy as np

import accept_cases as acases
import accept_ref
import close_ref as ref
import deliver_ref as dref
import flows_ref as fref
import recv_cases as rcases
import recv_ref

M32 = 1 << 32
ACK, PSH, FIN, SYN, RST = recv_ref.ACK, recv_ref.PSH, recv_ref.FIN, recv_ref.SYN, recv_ref.RST
POSITIONS = [0, 1, 62, 63, 64, 65, 127, 128, 255, 256, 257]
NAMES = {5: "FinWait1", 6: "FinWait2", 7: "Closing", 8: "TimeWait", 9: "CloseWait", 10: "LastAck"}


class CCase(acases.ACase):
    def __init__(self, frames, closers, listeners=None, slots=None, socks=None, snd=None, rings_bytes=64, **info):
        super().__init__(frames, accept_ref.listeners_of() if listeners is None else listeners,
                         accept_ref.slots_of() if slots is None else slots, socks, snd, rings_bytes, **info)
        self.closers = closers


# ---- one frame by name -------------------------------------------------------------------------------------

def make(hdr, kind, c, snd_nxt, j=0, options=b"", ip_options=b""):
    """The frame named `kind` for a connection whose rcv.NXT is c.nxt. Window and (where the name leaves it
    free) Ack vary with j."""
    nxt, wnd = c.nxt, (37 * j + 11) % 65536
    old = (snd_nxt - 1 - j % 5) % M32
    f = {
        "ack": (nxt, old, ACK, b""),                       # code 1 with ACK (in FinWait2: code 10)
        "ack_nxt": (nxt, snd_nxt, ACK, b""),
        "bare": (nxt, old, PSH if j % 2 else 0, b""),      # no ACK, no FIN: code 1 without una (FinWait1: code 10)
        "wrong_seq": ((nxt + 1 + j % 3) % M32, old, ACK, b""),                  # code 4
        "behind": ((nxt - 1) % M32, old, ACK, b""),                             # code 4 (not a keepalive: Ack != snd_nxt)
        "keepalive": ((nxt - 1) % M32, snd_nxt, ACK, b""),                      # code 5
        "data": (nxt, old, ACK | PSH, b"d" * (1 + j % 9)),                      # code 7
        "fin_ack_nxt": (nxt, snd_nxt, FIN | ACK, b""),
        "fin_ack_old": (nxt, old, FIN | ACK, b""),
        "fin": (nxt, old, FIN, b""),
        "rst": (nxt, old, RST, b""),
        "rst_ack": (nxt, old, RST | ACK, b""),
        "rst_wrong": ((nxt + 2) % M32, old, RST, b""),                          # code 4
        "syn": (nxt, 0, SYN, b""),                                              # rule 2
        "syn_ack": (nxt, old, SYN | ACK, b""),
    }[kind]
    return rcases.frame(hdr, f[0], f[1], f[2], wnd, f[3], options, ip_options)


# what is no event under a state, by the codes the fillers get there
FILLERS = {
    ref.FIN_WAIT_1: ("wrong_seq", "keepalive", "data", "bare", "behind"),        # 4, 5, 7, 10, 4
    ref.FIN_WAIT_2: ("ack", "wrong_seq", "keepalive", "data", "bare"),           # 10, 4, 5, 7, 10
    ref.CLOSING: ("bare", "wrong_seq", "keepalive", "data"),                     # 1, 4, 5, 7
    ref.CLOSE_WAIT: ("ack", "ack", "wrong_seq", "ack_nxt", "keepalive", "data", "bare"),  # 1, 1, 4, 1, 5, 7, 1
    ref.LAST_ACK: ("bare", "wrong_seq", "keepalive", "data"),
    ref.TIME_WAIT: ("ack", "fin_ack_nxt", "data", "rst", "syn", "wrong_seq"),    # all 8
    ref.CLOSED: ("ack", "fin_ack_nxt", "data", "rst", "syn", "wrong_seq"),
}


def script(hdr, state, nxt, una, snd_nxt, n, at=None, rcv_wnd=8192, snd_wnd=500, only=None, options=b"", ip_options=b""):
    """n frames of one closer's flow and the closer's record: at slot p of `at` (a dict) the frame named
    at[p], elsewhere a filler of the state the connection is in there (`only`: that filler alone). Returns
    (frames, record, trace) with trace[k] = (state before, code) of frame k, None behind the walk's end."""
    at = at or {}
    c = ref.Ctl(state, nxt % M32, una % M32, snd_wnd)
    frames, trace, ended = [], [], False
    for k in range(n):
        menu = FILLERS[c.state]
        kind = at.get(k) or only or menu[(k * 7 + k // len(menu)) % len(menu)]
        fr = make(hdr, kind, c, snd_nxt % M32, k, options, ip_options)
        frames.append(fr)
        if ended:
            trace.append(None)
            continue
        code = ref.code_of(c.state, c.nxt, snd_nxt % M32, rcv_wnd, recv_ref.fields(fr))
        if code == ref.ENDS:
            ended = True
            trace.append(None)
            continue
        trace.append((c.state, code))
        ref.step(c, code, snd_nxt % M32, recv_ref.fields(fr))
    record = (dref.key_of_header(hdr), state, nxt, rcv_wnd, una, snd_nxt, snd_wnd)
    return frames, record, trace


def interleaved(groups):
    return [groups[g][k] for g, k in fref.interleave(groups)]


def closers_case(flows, **info):
    """A case of closers' flows [(frames, record, trace)], their frames interleaved."""
    frames = fref.finish(interleaved([f for f, _, _ in flows]))
    return CCase(frames, ref.closers_of(*[r for _, r, _ in flows]), traces=[t for _, _, t in flows], **info)


# ---- events and codes at every side of a chunk boundary ------------------------------------------------------

# (state, the event, the state behind it)
TRANSITIONS = [(5, "fin_ack_nxt", 8), (5, "fin", 7), (5, "fin_ack_old", 7), (5, "ack", 6), (6, "fin_ack_nxt", 8), (6, "fin_ack_old", 8),
               (7, "ack", 8), (9, "fin", 9), (10, "ack", 0), (9, "rst", 0), (5, "rst_ack", 0), (9, "syn", 9)]
# (state, the filler forced at the positions, its code)
CODES = [(9, "ack", 1), (9, "wrong_seq", 4), (9, "keepalive", 5), (9, "data", 7), (6, "ack", 10), (5, "bare", 10), (8, "ack", 8),
         (10, "bare", 1), (7, "bare", 1), (9, "rst_wrong", 4)]


def positions_of(n):
    return [p for p in POSITIONS if p < n]


@functools.lru_cache(maxsize=None)
def event_at_positions(n, which):
    """One flow of n frames per position p: TRANSITIONS[which]'s event at slot p, fillers around it. The
    sequence numbers of every other flow cross 2^32 inside the flow."""
    state, event, after = TRANSITIONS[which]
    rng = np.random.default_rng(9100 + which)
    flows = []
    for j, p in enumerate(positions_of(n)):
        nxt = M32 - 1 if j % 2 else 70000 + j
        snd_nxt = M32 - 1 if j % 2 == 0 else 1
        flows.append(script(acases.header(rng, 0x2000 + j), state, nxt, snd_nxt - 9, snd_nxt, n, {p: event}))
    return closers_case(flows, state=state, event=event, after=after, positions=positions_of(n))


@functools.lru_cache(maxsize=None)
def codes_at_positions(n):
    """One flow of n frames per entry of CODES: the frame of that code at every position of POSITIONS."""
    rng = np.random.default_rng(9200 + n)
    flows = [script(acases.header(rng, 0x2100 + j), state, M32 - 40 + j, 5, 14, n, {p: kind for p in positions_of(n)})
             for j, (state, kind, _) in enumerate(CODES)]
    return closers_case(flows, positions=positions_of(n))


def several_events():
    """Two and three events inside one chunk, and events in consecutive lanes."""
    rng = np.random.default_rng(9300)
    h = [acases.header(rng, 0x2200 + j) for j in range(6)]
    flows = [
        script(h[0], 5, 1000, 41, 50, 70, {3: "ack", 10: "fin_ack_nxt"}),            # FinWait1 -> FinWait2 -> TimeWait, 8 behind
        script(h[1], 5, M32 - 2, 41, 50, 70, {0: "fin", 1: "ack"}),                    # FinWait1 -> Closing -> TimeWait
        script(h[2], 9, 2000, 41, 50, 70, {5: "fin", 6: "fin", 20: "rst"}),            # three events, the last an RST
        script(h[3], 9, 3000, 41, 50, 130, {62: "fin", 63: "fin", 64: "fin", 65: "rst"}),  # over the chunk boundary
        script(h[4], 10, 4000, 41, 50, 70, {63: "ack"}),                               # LastAck -> Closed in the last lane
        script(h[5], 5, 5000, 41, 50, 70, {7: "ack", 8: "syn", 9: "fin_ack_nxt"}),     # a SYN ends the walk in FinWait2
    ]
    return closers_case(flows)


def hostile():
    """CloseWait flows of FINs at consecutive Seqs: 64 in one chunk (the 64-pass bound), 130 over three, and
    one at rcv_wnd 0 (the bare FIN passes: zeroWindowOK)."""
    rng = np.random.default_rng(9400)
    flows = [script(acases.header(rng, 0x2300), 9, M32 - 30, 41, 50, 64, only="fin"),
             script(acases.header(rng, 0x2301), 9, 600, 41, 50, 130, only="fin"),
             script(acases.header(rng, 0x2302), 9, 700, 41, 50, 5, only="fin", rcv_wnd=0)]
    return closers_case(flows)


def geometries():
    """IHL x data offset in {5, 6, 15}: the same short script behind every pair of option lengths."""
    rng = np.random.default_rng(9500)
    flows = []
    for j, (ihl, doff) in enumerate((a, b) for a in (5, 6, 15) for b in (5, 6, 15)):
        opts, ip_opts = bytes([1]) * (4 * (doff - 5)), bytes([1]) * (4 * (ihl - 5))
        flows.append(script(acases.header(rng, 0x2400 + j), 5, 900 + j, 41, 50, 9, {2: "ack", 6: "fin_ack_nxt"}, options=opts,
                            ip_options=ip_opts))
    return closers_case(flows)


# ---- Established sockets: where the receive call's walk ended ------------------------------------------------

def established():
    """Listed sockets whose flows end in a FIN (at slot 63 and at slot 64, pure ACKs behind it), in an RST
    that passes, in an RST that fails with data behind it, in a SYN, in an RST as the flow's first frame;
    one socket without a flow; and two closers beside them."""
    rng = np.random.default_rng(9600)
    names = ("fin at 63", "fin at 64", "rst passes", "rst fails", "syn at stop", "rst first", "no flow", "rst with data")
    hdrs = [acases.header(rng, 0x2500 + j, port=8080) for j in range(len(names))]
    snd_nxt, una = 7000, 6990
    flows, socks, nxts = [], [], []
    for j, (name, h) in enumerate(zip(names, hdrs)):
        nxt = M32 - 200 if j % 2 else 100 + j
        fl, seq = [], nxt
        def pure(k, s=None):
            return rcases.frame(h, seq if s is None else s, una + 1 + k % 5, ACK, 300 + k)
        if name.startswith("fin at"):
            p = int(name[-2:])
            for k in range(p):  # data and pure ACKs in front of the FIN
                if k % 3 == 0:
                    pay = rcases.data(rng, 1 + k % 7)
                    fl.append(rcases.frame(h, seq, una + 1, ACK | PSH, 300 + k, pay))
                    seq = (seq + len(pay)) % M32
                else:
                    fl.append(pure(k))
            fl.append(rcases.frame(h, seq, una + 3, FIN | ACK, 999))
            seq = (seq + 1) % M32
            c = ref.Ctl(9, seq, 0, 0)
            for k in range(20):  # CloseWait: pure ACKs, a wrong Seq, a keepalive, a second FIN, data
                kind = {5: "wrong_seq", 9: "keepalive", 12: "fin", 15: "data"}.get(k, "ack")
                fl.append(make(h, kind, c, snd_nxt, k))
                if kind == "fin":
                    c.nxt = (c.nxt + 1) % M32
        elif name == "rst passes":
            fl += [pure(0), pure(1), rcases.frame(h, seq, 0, RST, 0), pure(3), rcases.frame(h, seq, una, SYN, 5), pure(5)]
        elif name == "rst fails":
            pay = rcases.data(rng, 6)
            fl += [pure(0), rcases.frame(h, seq + 1, 0, RST, 0), rcases.frame(h, seq, una + 1, ACK, 5, pay), pure(3, seq + 6)]
        elif name == "rst with data":
            fl += [pure(0), rcases.frame(h, seq, 0, RST, 0, b"why"), pure(2)]
        elif name == "syn at stop":
            fl += [pure(0), rcases.frame(h, seq, una, SYN | ACK, 5), rcases.frame(h, seq, 0, RST, 0)]
        elif name == "rst first":
            fl += [rcases.frame(h, seq, 0, RST | ACK, 0), pure(1)]
        flows.append(fl)
        nxts.append(nxt)
        socks.append(dref.sock(dref.key_of_header(h), nxt, 256 * j, 256, snd_nxt=snd_nxt))
    cf = [script(acases.header(rng, 0x2600 + j), st, 50 + j, 41, 50, 30, {11: ev}) for j, (st, ev) in enumerate(((5, "fin_ack_nxt"), (9, "fin")))]
    frames = fref.finish(interleaved([f for f in flows if f] + [f for f, _, _ in cf]))
    return CCase(frames, ref.closers_of(*[r for _, r, _ in cf]), socks=dref.socks_of(*socks),
                 snd=recv_ref.snd_of(*[(una, 444)] * len(names)), rings_bytes=256 * len(names), names=names)


# ---- a closer and a listener -----------------------------------------------------------------------------------

def closer_and_listener():
    """Closers whose flow's first frame is a lone SYN to a listener: the accept stage takes it as it would
    without the list; the walk ends at slot 0, except in TimeWait, where rule 1 comes first."""
    rng = np.random.default_rng(9700)
    flows = []
    for j, state in enumerate((5, 9, 8)):
        h = acases.header(rng, 0x2700 + j)
        syn = acases.syn(h, seq=333 + j)
        rest, record, _ = script(h, state, 50, 41, 50, 4)
        flows.append(([syn] + rest, record, None))
    case = closers_case(flows)
    case.listeners = accept_ref.listeners_of((acases.local(80), acases.MAC, 0, 4))
    case.slots = acases.default_slots(4)
    return case


# ---- scale ----------------------------------------------------------------------------------------------------

BIG = acases.BIG
BIG_CLOSERS = 65536
PER = 1012  # frames of an established socket's flow in the second shape: 64 x 1,012 + 1,025 = 65,793


def _one_frame_flows(n, sport0=1):
    """n one-frame flows, each a FIN | ACK with Seq 77 + k and Ack 5000, as finished frames, and their keys."""
    rng = np.random.default_rng(9800)
    base = np.frombuffer(rcases.frame(acases.header(rng, 1), 77, 5000, FIN | ACK, 1234), dtype=np.uint8)
    rows = np.tile(base, (n, 1))
    k = np.arange(n, dtype=np.uint64)
    sport = k % 60000 + sport0
    rows[:, 28], rows[:, 29] = k // 60000, 1 + (k % 250)
    rows[:, 34], rows[:, 35] = sport >> 8, sport & 0xFF
    rows[:, 38:42] = ((k + 77) % M32).astype(">u4").view(np.uint8).reshape(n, 4)
    frames = fref.finish([r.tobytes() for r in rows])
    return frames


def _closers_for(frames, state, snd_nxt=5000):
    from seqs_amd.framesum import CLOSER_DTYPE

    a = np.zeros(len(frames), dtype=CLOSER_DTYPE)
    for i, fr in enumerate(frames):
        a["key"][i] = np.frombuffer(fref.flow_key(fr), dtype=np.uint8)
        a["rcv_nxt"][i] = recv_ref.fields(fr)[0]
    a["state"], a["rcv_wnd"], a["snd_una"], a["snd_nxt"], a["snd_wnd"] = state, 8192, snd_nxt - 1, snd_nxt, 100
    return a


@functools.lru_cache(maxsize=None)
def big(shape):
    """65,793 frames: 65,536 closers in FinWait1 with one FIN | ACK each (the 257 other flows have no closer),
    or 1,000 closers in CloseWait (and 25 flows without one) beside 64 established sockets of 1,011 pure ACKs
    and a FIN each."""
    flows = _one_frame_flows(BIG)
    if shape == "65536 closers":
        return CCase(flows, _closers_for(flows[:BIG_CLOSERS], 5), n_time_wait=BIG_CLOSERS)
    assert shape == "1000 closers, 64 sockets"
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
    return CCase(frames, _closers_for(rest[:1000], 9), socks=socks, snd=recv_ref.snd_of(*[(150, 9)] * 64), rings_bytes=8 * 64,
                 n_close_wait=64)


BIG_SHAPES = ("65536 closers", "1000 closers, 64 sockets")
