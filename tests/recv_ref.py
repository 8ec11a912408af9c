"""The expected output of the receive call (fs_recv_flows_batch), restated twice with code the kernels
do not share.

contract(): the rules of include/framesum_recv.h, sequentially in Python integers, on top of the
`delivered` marks and the `stop` of tests/deliver_ref.py's walk. expected() is deliver_ref.expected's
dict plus snd_out and code.

GoBlock: a literal transliteration of the reference's ControlBlock for StateEstablished, branch for
branch, in the manner of tests/test_go_gate_order.py: validateIncomingSegment (control.go:281-351), Recv
(control_user.go:164-224), rcvEstablished (control.go:217-232), IncomingIsKeepalive
(control_user.go:260-264), with LessThan / LessThanEq / InRange / InWindow / Add (valuesize.go:27-50)
and Segment.LEN / Last (seqs.go:19-32). It knows nothing of rings or codes; go_walk() names what it
did to each segment with the contract's code numbers."""
import numpy as np

import deliver_ref
import flows_ref

M32 = 1 << 32
FIN, SYN, RST, PSH, ACK, URG, ECE, CWR, NS = (1 << k for k in range(9))  # eth/headers.go:174
ACK_OWED, FIN_SEEN = 1, 2
NONE = deliver_ref.NONE
TAKEN, DUPLICATE, UNSENT, REJECTED, KEEPALIVE, RING_FULL = 1, 2, 3, 4, 5, 6


def snd_of(*pairs):
    """A SND_DTYPE array of (snd_una, snd_wnd) pairs."""
    from seqs_amd.framesum import SND_DTYPE

    a = np.zeros(len(pairs), dtype=SND_DTYPE)
    for i, (una, wnd) in enumerate(pairs):
        a[i] = (una % M32, wnd)
    return a


def fields(fr: bytes):
    """(Seq, Ack, Window, the nine flag bits, payload length) of an accepted TCP frame."""
    l4 = 14 + (fr[14] & 15) * 4
    a, b = flows_ref.payload_range(fr)
    return (int.from_bytes(fr[l4 + 4 : l4 + 8], "big"), int.from_bytes(fr[l4 + 8 : l4 + 12], "big"),
            int.from_bytes(fr[l4 + 14 : l4 + 16], "big"), ((fr[l4 + 12] & 1) << 8) | fr[l4 + 13], b - a)


# ---- 1. the contract ---------------------------------------------------------------------------------

def less_than(v, w):
    return (v - w) % M32 >= 1 << 31


def less_than_eq(v, w):
    return v == w or less_than(v, w)


def code_of(una, nxt_k, snd_nxt, rcv_wnd, seq, ack, flags9, length, admitted):
    fin = 1 if flags9 & FIN else 0
    if length == 0 and not fin:
        if seq == (nxt_k - 1) % M32 and flags9 == ACK and ack == snd_nxt:
            return KEEPALIVE
        if seq != nxt_k:
            return REJECTED
        if flags9 & ACK and not less_than(una, ack):
            return DUPLICATE
        if flags9 & ACK and not less_than_eq(ack, snd_nxt):
            return UNSENT
        return TAKEN
    if admitted:
        return TAKEN
    if seq != nxt_k or length + fin > rcv_wnd:
        return REJECTED
    if flags9 & ACK and not less_than_eq(ack, snd_nxt):
        return UNSENT
    return RING_FULL


def contract(segs, admitted, una, wnd, rcv_nxt, snd_nxt, rcv_wnd):
    """The walk over one socket's segments before `stop`: segs = [(seq, ack, window, flags9, len)],
    admitted[k] = the delivery admitted segment k. Returns (codes, una, wnd, flags)."""
    nxt, codes, flags = rcv_nxt, [], 0
    for (seq, ack, window, flags9, length), adm in zip(segs, admitted):
        c = code_of(una, nxt, snd_nxt, rcv_wnd, seq, ack, flags9, length, adm)
        considered = length != 0 or flags9 & FIN
        if c == TAKEN:
            wnd = window
            if flags9 & ACK:
                una = ack
        if c == UNSENT or (c == TAKEN and considered):
            flags |= ACK_OWED
        if adm:
            nxt = (nxt + length + (1 if flags9 & FIN else 0)) % M32
            if flags9 & FIN:
                flags |= FIN_SEEN
        codes.append(c)
    return codes, una, wnd, flags


def walk(frames, socks, snd, e):
    """(snd_out, code) for the batch's frames (a list of bytes) and the delivery part `e`
    (deliver_ref.expected's dict)."""
    from seqs_amd.framesum import SND_OUT_DTYPE

    out = np.zeros(len(socks), dtype=SND_OUT_DTYPE)
    code = np.zeros(len(frames), dtype=np.uint8)
    order = e["order"]
    for s, (sk, sn, so) in enumerate(zip(socks, snd, e["socks_out"])):
        una, wnd, flags, codes = int(sn["snd_una"]), int(sn["snd_wnd"]), 0, []
        if int(so["flow"]) != NONE:
            first = int(e["flows"][int(so["flow"])]["first_frame"])
            idx = [int(order[k]) for k in range(first, int(so["stop"]))]
            codes, una, wnd, flags = contract([fields(frames[i]) for i in idx], [e["delivered"][i] == 1 for i in idx], una, wnd,
                                              int(sk["rcv_nxt"]), int(sk["snd_nxt"]), int(sk["rcv_wnd"]))
            code[idx] = codes
        out[s] = (una, wnd, codes.count(TAKEN), codes.count(DUPLICATE), codes.count(UNSENT),
                  codes.count(REJECTED) + codes.count(RING_FULL), codes.count(KEEPALIVE), flags)
    return out, code


def expected(buf, offsets, lengths, mtu, flags, noise, plead, cap, socks, snd, rings):
    """deliver_ref.expected's dict plus snd_out and code."""
    e = deliver_ref.expected(buf, offsets, lengths, mtu, flags, noise, plead, cap, socks, rings)
    raw = buf.tobytes()
    room = 4 if flags & flows_ref.RX_FCS else 0
    frames = [raw[int(o) : int(o) + max(0, int(l) - room)] for o, l in zip(offsets, lengths)]
    e["snd_out"], e["code"] = walk(frames, socks, snd, e)
    return e


# ---- 2. the reference, transliterated ----------------------------------------------------------------

def go_less_than(v, w):       # valuesize.go:27
    d = (v - w) % M32
    return (d - M32 if d >= 1 << 31 else d) < 0   # int32(v-w) < 0


def go_less_than_eq(v, w):    # valuesize.go:32
    return v == w or go_less_than(v, w)


def go_in_range(v, a, b):     # valuesize.go:37
    return (v - a) % M32 < (b - a) % M32


def go_add(v, s):             # valuesize.go:48
    return (v + s) % M32


def go_in_window(v, first, size):  # valuesize.go:43
    return go_in_range(v, first, go_add(first, size))


class Segment:
    def __init__(self, seq, ack, wnd, flags, datalen):
        self.SEQ, self.ACK, self.WND, self.Flags, self.DATALEN = seq, ack, wnd, flags, datalen

    def LEN(self):            # seqs.go:19
        add = (self.Flags >> 0) & 1
        add += (self.Flags >> 1) & 1
        return self.DATALEN + add

    def Last(self):           # seqs.go:26
        seglen = self.LEN()
        if seglen == 0:
            return self.SEQ
        return (go_add(self.SEQ, seglen) - 1) % M32


class GoBlock:
    """ControlBlock in StateEstablished: snd.UNA / NXT / WND, rcv.NXT / WND, pending[0]."""

    def __init__(self, una, snd_nxt, snd_wnd, rcv_nxt, rcv_wnd):
        self.snd_UNA, self.snd_NXT, self.snd_WND, self.rcv_NXT, self.rcv_WND = una, snd_nxt, snd_wnd, rcv_nxt, rcv_wnd
        self.pending0, self.established = 0, True

    def validateIncomingSegment(self, seg):  # control.go:281
        flags = seg.Flags
        hasAck = flags & ACK == ACK
        checkSEQ = not flags & SYN
        established = self.established
        acksOld = hasAck and not go_less_than(self.snd_UNA, seg.ACK)
        acksUnsentData = hasAck and not go_less_than_eq(seg.ACK, self.snd_NXT)
        ctlOrDataSegment = established and (seg.DATALEN > 0 or bool(flags & (FIN | RST)))
        zeroWindowOK = self.rcv_WND == 0 and seg.DATALEN == 0 and seg.SEQ == self.rcv_NXT
        err = None
        if seg.WND > 0xFFFF:
            err = "errWindowOverflow"
        elif checkSEQ and self.rcv_WND == 0 and seg.DATALEN > 0 and seg.SEQ == self.rcv_NXT:
            err = "errZeroWindow"
        elif checkSEQ and not go_in_window(seg.SEQ, self.rcv_NXT, self.rcv_WND) and not zeroWindowOK:
            err = "errSeqNotInWindow"
        elif checkSEQ and not go_in_window(seg.Last(), self.rcv_NXT, self.rcv_WND) and not zeroWindowOK:
            err = "errLastNotInWindow"
        elif checkSEQ and seg.SEQ != self.rcv_NXT:
            err = "errRequireSequential"
        if err is not None:
            return err
        assert not flags & RST, "RST ends the walk before Recv"
        if established and acksOld and not ctlOrDataSegment:
            err = "errDropSegment:dup"
            self.pending0 &= FIN
        elif established and acksUnsentData:
            err = "errDropSegment:unsent"
            self.pending0 = ACK
        return err

    def rcvEstablished(self, seg):  # control.go:217
        pending = 0
        dataToAck = seg.DATALEN > 0
        hasFin = bool(seg.Flags & FIN)
        if dataToAck or hasFin:
            pending = ACK
            if hasFin:
                self.established = False  # StateCloseWait: the walk ends behind an admitted FIN
        return pending

    def Recv(self, seg):  # control_user.go:164
        err = self.validateIncomingSegment(seg)
        if err is not None:
            return err
        pending = self.rcvEstablished(seg)
        self.pending0 |= pending
        self.snd_WND = seg.WND
        if seg.Flags & ACK:
            self.snd_UNA = seg.ACK
        self.rcv_NXT = (self.rcv_NXT + seg.LEN()) % M32
        return None

    def IncomingIsKeepalive(self, seg):  # control_user.go:260
        return seg.SEQ == (self.rcv_NXT - 1) % M32 and seg.Flags == ACK and seg.ACK == self.snd_NXT and seg.DATALEN == 0


GO_CODE = {None: TAKEN, "errDropSegment:dup": DUPLICATE, "errDropSegment:unsent": UNSENT, "errZeroWindow": REJECTED,
           "errSeqNotInWindow": REJECTED, "errLastNotInWindow": REJECTED, "errRequireSequential": REJECTED}


def go_walk(segs, una, wnd, rcv_nxt, snd_nxt, rcv_wnd):
    """TCPConn.recv's order (stacks/tcpconn.go:349: the keepalive test, then Recv) over the segments
    before a SYN or RST, ending behind an accepted FIN. Returns (codes, the block): the block's
    pending0 & ACK is the reference's own pending ACK, which a duplicate clears."""
    tcb, codes = GoBlock(una, snd_nxt, wnd, rcv_nxt, rcv_wnd), []
    for seq, ack, window, flags9, length in segs:
        if flags9 & (SYN | RST) or not tcb.established:
            break
        seg = Segment(seq, ack, window, flags9, length)
        if tcb.IncomingIsKeepalive(seg):
            codes.append(KEEPALIVE)
            continue
        codes.append(GO_CODE[tcb.Recv(seg)])
    return codes, tcb
