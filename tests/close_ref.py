"""The expected output of the close call (fs_close_flows_batch), restated twice with code the kernels do
not share.

contract(): the rules of include/framesum_close.h, sequentially in Python integers, on top of
tests/accept_ref.py's dict (the flows, their order, socks_out and snd_out). expected() is
accept_ref.expected's dict plus closers_out, socks_close and ctl_code.

GoTCB / go_recv(): a literal transliteration of the reference for the states from Established on, branch
for branch, in the manner of tests/recv_ref.py's GoBlock: the two gates of TCPConn.recv
(stacks/tcpconn.go:337 with IsClosed, seqs.go:224; :349 IncomingIsKeepalive, control_user.go:260-264),
validateIncomingSegment (control.go:281-351), handleRST (control.go:407-425), close (control.go:389-395),
Recv (control_user.go:164-224), rcvEstablished / rcvFinWait1 / rcvFinWait2 (control.go:217-261). It knows
nothing of flows, codes or batches."""
import numpy as np

import accept_ref
import flows_ref
import recv_ref
from recv_ref import ACK, FIN, M32, RST, SYN, Segment, go_add, go_in_window, go_less_than, go_less_than_eq

NONE = 0xFFFFFFFF
CLOSED, ESTABLISHED, FIN_WAIT_1, FIN_WAIT_2, CLOSING, TIME_WAIT, CLOSE_WAIT, LAST_ACK = 0, 4, 5, 6, 7, 8, 9, 10
TAKEN, REJECTED, KEEPALIVE, DATA, IGNORED, RESET_CODE, EXPECTED = 1, 4, 5, 7, 8, 9, 10
ENDS = "ends"  # rule 2: no code, the walk ends in front of the frame
ACK_OWED, FIN_TAKEN, RESET = 1, 2, 4


def closers_of(*rows):
    """A CLOSER_DTYPE array of (key 13 bytes, state, rcv_nxt, rcv_wnd, snd_una, snd_nxt, snd_wnd) rows."""
    from seqs_amd.framesum import CLOSER_DTYPE

    a = np.zeros(len(rows), dtype=CLOSER_DTYPE)
    for i, (key, state, rcv_nxt, rcv_wnd, una, snd_nxt, snd_wnd) in enumerate(rows):
        a["key"][i] = np.frombuffer(bytes(key), dtype=np.uint8)
        a["state"][i], a["rcv_nxt"][i], a["rcv_wnd"][i] = state, rcv_nxt % M32, rcv_wnd
        a["snd_una"][i], a["snd_nxt"][i], a["snd_wnd"][i] = una % M32, snd_nxt % M32, snd_wnd
    return a


# ---- 1. the contract -----------------------------------------------------------------------------------

def rule7_state(state, snd_nxt, ack, flags9):
    """The state behind a frame rule 7 judges, or None when the state refuses it (code 10)."""
    fin, has_ack = bool(flags9 & FIN), bool(flags9 & ACK)
    if state == FIN_WAIT_1:
        if fin and has_ack and ack == snd_nxt:
            return TIME_WAIT
        if fin:
            return CLOSING
        return FIN_WAIT_2 if has_ack else None
    if state == FIN_WAIT_2:
        return TIME_WAIT if fin and has_ack else None
    if state == CLOSING:
        return TIME_WAIT if has_ack else CLOSING
    if state == LAST_ACK:
        return CLOSED if has_ack else LAST_ACK
    return state


def code_of(state, nxt, snd_nxt, rcv_wnd, seg):
    """The first rule that applies; rule 5 in its worked-out form (a frame without data passes iff Seq ==
    nxt)."""
    seq, ack, _, flags9, length = seg
    if state in (TIME_WAIT, CLOSED):
        return IGNORED
    if flags9 & SYN:
        return ENDS
    if seq == (nxt - 1) % M32 and flags9 == ACK and ack == snd_nxt and length == 0:
        return KEEPALIVE
    if length > 0:
        return DATA
    if seq != nxt:
        return REJECTED
    if flags9 & RST:
        return RESET_CODE
    return EXPECTED if rule7_state(state, snd_nxt, ack, flags9) is None else TAKEN


class Ctl:
    def __init__(self, state, nxt, una, wnd):
        self.state, self.nxt, self.una, self.wnd, self.flags = state, nxt, una, wnd, 0
        self.n_taken = self.n_rejected = 0

    def record(self, stop):
        zero = self.state == CLOSED
        return (self.state, 0 if zero else self.nxt, 0 if zero else self.una, 0 if zero else self.wnd, self.n_taken,
                self.n_rejected, stop, self.flags)


def step(c, code, snd_nxt, seg):
    seq, ack, window, flags9, _ = seg
    if code == RESET_CODE:
        c.state, c.flags = CLOSED, c.flags | RESET
    elif code == TAKEN:
        nxt_state = rule7_state(c.state, snd_nxt, ack, flags9)
        if c.state in (FIN_WAIT_1, FIN_WAIT_2) and nxt_state != c.state:
            c.flags |= ACK_OWED
        c.state, c.wnd = nxt_state, window
        if flags9 & ACK:
            c.una = ack
        if flags9 & FIN:
            c.nxt, c.flags = (c.nxt + 1) % M32, c.flags | FIN_TAKEN
        c.n_taken += 1
    elif code in (REJECTED, DATA, EXPECTED):
        c.n_rejected += 1


def walk(c, segs, snd_nxt, rcv_wnd):
    """The control walk of rule 2 over `segs` = [(seq, ack, window, flags9, len)]: the codes of the frames
    it handled (it ends in front of a SYN)."""
    codes = []
    for seg in segs:
        code = code_of(c.state, c.nxt, snd_nxt, rcv_wnd, seg)
        if code == ENDS:
            break
        step(c, code, snd_nxt, seg)
        codes.append(code)
    return codes


def contract(frames, e, socks, closers):
    """(closers_out, socks_close, ctl_code) for the batch's frames (a list of bytes) and the accept part `e`."""
    from seqs_amd.framesum import CLOSE_OUT_DTYPE

    closers_out = np.zeros(len(closers), dtype=CLOSE_OUT_DTYPE)
    socks_close = np.zeros(len(socks), dtype=CLOSE_OUT_DTYPE)
    ctl = np.zeros(len(frames), dtype=np.uint8)
    order = e["order"]
    flow_of = {}
    for fl in e.get("flows", ()):
        first, count = int(fl["first_frame"]), int(fl["n_frames"])
        flow_of[flows_ref.flow_key(frames[int(order[first])])] = (first, first + count)
    for i, cl in enumerate(closers):
        c = Ctl(int(cl["state"]), int(cl["rcv_nxt"]), int(cl["snd_una"]), int(cl["snd_wnd"]))
        span = flow_of.get(bytes(cl["key"]))
        stop = NONE
        if span is not None:
            idx = [int(order[k]) for k in range(*span)]
            codes = walk(c, [recv_ref.fields(frames[j]) for j in idx], int(cl["snd_nxt"]), int(cl["rcv_wnd"]))
            ctl[idx[: len(codes)]] = codes
            stop = span[0] + len(codes)
        closers_out[i] = c.record(stop)
    for s, (sk, so, sn) in enumerate(zip(socks, e["socks_out"], e["snd_out"])):
        c = Ctl(ESTABLISHED, int(so["rcv_nxt"]), int(sn["snd_una"]), int(sn["snd_wnd"]))
        stop = int(so["stop"])
        snd_nxt, rcv_wnd = int(sk["snd_nxt"]), int(sk["rcv_wnd"])
        if int(so["flow"]) != NONE:
            fl = e["flows"][int(so["flow"])]
            end = int(fl["first_frame"]) + int(fl["n_frames"])
            idx = [int(order[k]) for k in range(stop, end)]
            segs = [recv_ref.fields(frames[j]) for j in idx]
            if int(sn["flags"]) & recv_ref.FIN_SEEN:
                c.state = CLOSE_WAIT
                codes = walk(c, segs, snd_nxt, rcv_wnd)
                ctl[idx[: len(codes)]] = codes
                stop += len(codes)
            elif segs and segs[0][3] & RST and not segs[0][3] & SYN:
                code = code_of(ESTABLISHED, c.nxt, snd_nxt, rcv_wnd, segs[0])
                step(c, code, snd_nxt, segs[0])
                ctl[idx[0]] = code
                stop += 1
                if code == RESET_CODE:
                    codes = walk(c, segs[1:], snd_nxt, rcv_wnd)
                    ctl[idx[1 : 1 + len(codes)]] = codes
                    stop += len(codes)
        socks_close[s] = c.record(stop)
    return closers_out, socks_close, ctl


def expected(buf, offsets, lengths, mtu, flags, noise, plead, cap, socks, snd, rings, listeners, slots, synack_flags, synacks,
             closers):
    """accept_ref.expected's dict plus closers_out, socks_close and ctl_code."""
    e = accept_ref.expected(buf, offsets, lengths, mtu, flags, noise, plead, cap, socks, snd, rings, listeners, slots,
                            synack_flags, synacks)
    raw = buf.tobytes()
    room = 4 if flags & flows_ref.RX_FCS else 0
    frames = [raw[int(o) : int(o) + max(0, int(l) - room)] for o, l in zip(offsets, lengths)]
    e["closers_out"], e["socks_close"], e["ctl_code"] = contract(frames, e, socks, closers)
    return e


# ---- 2. the reference, transliterated --------------------------------------------------------------------

FINACK = FIN | ACK


class GoTCB:
    """ControlBlock from StateEstablished on (state: the numbers of seqs.go:175-208)."""

    def __init__(self, state, una, snd_nxt, snd_wnd, rcv_nxt, rcv_wnd):
        self.state = state
        self.snd_UNA, self.snd_NXT, self.snd_WND, self.rcv_NXT, self.rcv_WND = una, snd_nxt, snd_wnd, rcv_nxt, rcv_wnd
        self.pending = [0, 0]
        self.challengeAck = False

    def close(self):  # control.go:389
        self.state = CLOSED
        self.pending = [0, 0]
        self.rcv_NXT = self.rcv_WND = 0          # resetRcv(0, 0)
        self.snd_UNA = self.snd_NXT = self.snd_WND = 0  # resetSnd(0, 0)

    def handleRST(self, seq):  # control.go:407
        if seq != self.rcv_NXT:
            self.challengeAck = True
            self.pending[0] |= ACK
            return "errDropSegment"
        # (IsPreestablished is false from Established on)
        self.close()
        return "ErrClosed"

    def validateIncomingSegment(self, seg):  # control.go:281
        flags = seg.Flags
        hasAck = flags & ACK == ACK
        checkSEQ = not flags & SYN
        established = self.state == ESTABLISHED
        acksOld = hasAck and not go_less_than(self.snd_UNA, seg.ACK)
        acksUnsentData = hasAck and not go_less_than_eq(seg.ACK, self.snd_NXT)
        ctlOrDataSegment = established and (seg.DATALEN > 0 or bool(flags & (FIN | RST)))
        zeroWindowOK = self.rcv_WND == 0 and seg.DATALEN == 0 and seg.SEQ == self.rcv_NXT
        err = None
        if seg.WND > 0xFFFF:
            err = "errWindowOverflow"
        elif self.state == CLOSED:
            err = "ErrClosedPipe"
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
        if flags & RST:
            return self.handleRST(seg.SEQ)
        if established and acksOld and not ctlOrDataSegment:
            err = "errDropSegment"
            self.pending[0] &= FIN
        elif established and acksUnsentData:
            err = "errDropSegment"
            self.pending[0] = ACK
        # (preestablished: not from Established on)
        return err

    def rcvEstablished(self, seg):  # control.go:217
        pending = 0
        if seg.DATALEN > 0 or seg.Flags & FIN:
            pending = ACK
            if seg.Flags & FIN:
                self.state = CLOSE_WAIT
                self.pending[1] = FIN
        return pending, None

    def rcvFinWait1(self, seg):  # control.go:234
        hasFin, hasAck = bool(seg.Flags & FIN), bool(seg.Flags & ACK)
        if hasFin and hasAck and seg.ACK == self.snd_NXT:
            self.state = TIME_WAIT
        elif hasFin:
            self.state = CLOSING
        elif hasAck:
            self.state = FIN_WAIT_2
        else:
            return 0, "errFinwaitExpectedACK"
        return ACK, None

    def rcvFinWait2(self, seg):  # control.go:255
        if seg.Flags & FINACK != FINACK:
            return 0, "errFinwaitExpectedFinack"
        self.state = TIME_WAIT
        return ACK, None

    def Recv(self, seg):  # control_user.go:164
        err = self.validateIncomingSegment(seg)
        if err is not None:
            return err
        pending = 0
        if self.state == ESTABLISHED:
            pending, err = self.rcvEstablished(seg)
        elif self.state == FIN_WAIT_1:
            pending, err = self.rcvFinWait1(seg)
        elif self.state == FIN_WAIT_2:
            pending, err = self.rcvFinWait2(seg)
        elif self.state == CLOSE_WAIT:
            pass
        elif self.state == LAST_ACK:
            if seg.Flags & ACK:
                self.close()
        elif self.state == CLOSING:
            if seg.Flags & ACK:
                self.state = TIME_WAIT
        else:
            raise AssertionError("unexpected recv state")  # (the reference panics)
        if err is not None:
            return err
        self.pending[0] |= pending
        self.snd_WND = seg.WND
        if seg.Flags & ACK:
            self.snd_UNA = seg.ACK
        self.rcv_NXT = go_add(self.rcv_NXT, seg.LEN())
        return None

    def IncomingIsKeepalive(self, seg):  # control_user.go:260
        return seg.SEQ == (self.rcv_NXT - 1) % M32 and seg.Flags == ACK and seg.ACK == self.snd_NXT and seg.DATALEN == 0


def go_recv(tcb, seg):
    """TCPConn.recv's control part for one segment (stacks/tcpconn.go:334-361): "EOF:closed" from the
    IsClosed gate, "keepalive", or Recv's error (None: admitted)."""
    if tcb.state in (CLOSED, TIME_WAIT):  # tcpconn.go:337, seqs.go:224
        return "EOF:closed"
    if tcb.IncomingIsKeepalive(seg):      # tcpconn.go:349
        return "keepalive"
    return tcb.Recv(seg)
