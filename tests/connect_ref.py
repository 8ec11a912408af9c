"""The expected output of the connect call (fs_connect_flows_batch), restated twice with code the kernels do
not share.

contract(): the rules of include/framesum_connect.h, sequentially in Python integers, on top of
tests/close_ref.py's dict (the flows, their order, the close call's ctl_code). expected() is
close_ref.expected's dict plus openers_out, the whole replies buffer, reply_out and reply_status, with
ctl_code carrying this call's codes too. The replies' checksums and FCS come from oracle/pyref.py.

GoOpener / go_recv() / go_send(): a literal transliteration of the reference for a connection that dials
out, branch for branch, in the manner of tests/close_ref.py's GoTCB: Open (control_user.go:49-71) and the
Send of the first SYN (stacks/tcpconn.go:282-293), the gates of TCPConn.recv (stacks/tcpconn.go:337, :349
with IncomingIsKeepalive, control_user.go:260-264), validateIncomingSegment (control.go:281-351) with
handleRST (control.go:407-425), rcvSynSent (control.go:175-201), Recv's update (control_user.go:211-217),
PendingSegment (control.go:100-152) and Send (control_user.go:106-158, validateOutgoingSegment
control.go:353-386) for the four replies, synsentSegment (stacks/tcpconn.go:477-484) and CalculateHeaders
(stacks/port_tcp.go:162-194). It knows nothing of flows, codes or batches."""
import numpy as np

import accept_ref
import close_ref
import flows_ref
import recv_ref
from accept_ref import STRIDE, peer_mss, prand16
from recv_ref import ACK, FIN, M32, RST, SYN, Segment, go_add, go_in_window, go_less_than, go_less_than_eq

NONE = 0xFFFFFFFF
LISTEN, SYN_RCVD, SYN_SENT, ESTABLISHED = 1, 2, 3, 4
TAKEN, REJECTED, KEEPALIVE, EXPECTED, BAD_ACK = 1, 4, 5, 10, 11
ENDS_RST, ENDS_SYN = "ends:rst", "ends:syn"  # rules 3 and 4: no code, the walk ends in front of the frame
SEND_SYN = 1
REPLY_NONE, REPLY_ACK, REPLY_SYNACK, REPLY_RST, REPLY_SYN = range(5)
STOP_RST, STOP_SYN = 1, 2
FCS_APPEND = 2
OPEN_WND = 1  # snd.WND of a block Open has made


def openers_of(*rows):
    """An OPENER_DTYPE array of (key 13 bytes, flags, local_mac, remote_mac, iss, rcv_wnd, ip_id) rows."""
    from seqs_amd.framesum import OPENER_DTYPE

    a = np.zeros(len(rows), dtype=OPENER_DTYPE)
    for i, (key, flags, local_mac, remote_mac, iss, rcv_wnd, ip_id) in enumerate(rows):
        a["key"][i] = np.frombuffer(bytes(key), dtype=np.uint8)
        a["local_mac"][i] = np.frombuffer(bytes(local_mac), dtype=np.uint8)
        a["remote_mac"][i] = np.frombuffer(bytes(remote_mac), dtype=np.uint8)
        a["flags"][i], a["iss"][i], a["rcv_wnd"][i], a["ip_id"][i] = flags, iss % M32, rcv_wnd, ip_id
    return a


# ---- 1. the contract -----------------------------------------------------------------------------------

def seq_passes(seq, flags9, length, rcv_wnd):
    """Rule 2 in its worked-out form."""
    fin = 1 if flags9 & FIN else 0
    return seq == 0 and (length == 0 or (rcv_wnd > 0 and length + fin - 1 < rcv_wnd))


def code_of(iss, rcv_wnd, seg):
    """The first rule that applies."""
    seq, ack, _, flags9, length = seg
    nxt = (iss + 1) % M32
    if seq == M32 - 1 and flags9 == ACK and ack == nxt and length == 0:
        return KEEPALIVE
    if not flags9 & SYN and not seq_passes(seq, flags9, length, rcv_wnd):
        return REJECTED
    if flags9 & RST:
        return ENDS_RST
    if flags9 & SYN and (length > 0 or flags9 & ~(SYN | ACK)):
        return ENDS_SYN
    if flags9 & ACK and ack != nxt:
        return BAD_ACK
    if not flags9 & SYN:
        return EXPECTED
    return TAKEN


class Rec:
    """An opener's out record, field by field as fs_cn_out lists them."""

    def __init__(self, iss):
        self.iss = iss
        self.state, self.irs, self.rcv_nxt = SYN_SENT, 0, 0
        self.snd_una, self.snd_nxt, self.snd_wnd = iss, (iss + 1) % M32, OPEN_WND
        self.n_rejected = self.n_keepalive = 0
        self.stop = self.frame = NONE
        self.peer_mss = self.reply = self.flags = self.rst_seq = 0

    def record(self):
        return (self.state, self.irs, self.rcv_nxt, self.snd_una, self.snd_nxt, self.snd_wnd, self.n_rejected,
                self.n_keepalive, self.stop, self.frame, self.peer_mss, self.reply, self.flags, self.rst_seq)


def walk(r, rcv_wnd, segs, first, frames_idx, mss_of):
    """The walk of section 3 over `segs` = [(seq, ack, window, flags9, len)], the flow's slots from `first`
    on (frames_idx[k]: slot first + k's batch index; mss_of(k): the option walk's value for that frame).
    Returns the codes of the frames it handled."""
    codes = []
    r.stop = first
    for k, seg in enumerate(segs):
        seq, ack, window, flags9, _ = seg
        code = code_of(r.iss, rcv_wnd, seg)
        if code in (ENDS_RST, ENDS_SYN):
            r.stop, r.flags = first + k, STOP_RST if code == ENDS_RST else STOP_SYN
            return codes
        codes.append(code)
        r.stop = first + k + 1
        if code == KEEPALIVE:
            r.n_keepalive += 1
        elif code in (REJECTED, EXPECTED):
            r.n_rejected += 1
        elif code == BAD_ACK:
            r.reply, r.rst_seq, r.snd_wnd, r.snd_una, r.snd_nxt, r.frame = REPLY_RST, ack, window, r.iss, r.iss, frames_idx[k]
            return codes
        else:
            r.irs, r.rcv_nxt, r.snd_wnd, r.frame, r.peer_mss = seq, (seq + 1) % M32, window, frames_idx[k], mss_of(k)
            if flags9 & ACK:
                r.state, r.reply, r.snd_una, r.snd_nxt = ESTABLISHED, REPLY_ACK, (r.iss + 1) % M32, (r.iss + 1) % M32
            else:
                r.state, r.reply, r.snd_una, r.snd_nxt = SYN_RCVD, REPLY_SYNACK, r.iss, r.iss
            return codes
    return codes


def reply_header(op, r) -> bytes:
    """The reply of section 4, field by field, its checksum fields still zero."""
    key, iss = bytes(op["key"]), int(op["iss"])
    seq, ack, flags = {REPLY_ACK: ((iss + 1) % M32, (r.irs + 1) % M32, ACK), REPLY_SYNACK: (iss, (r.irs + 1) % M32, SYN | ACK),
                       REPLY_RST: (r.rst_seq, 0, RST), REPLY_SYN: (iss, 0, SYN)}[r.reply]
    h = bytearray(54)
    h[0:6], h[6:12], h[12:14] = bytes(op["remote_mac"]), bytes(op["local_mac"]), b"\x08\x00"
    h[14] = 0x45
    h[16:18] = (40).to_bytes(2, "big")
    h[18:20] = prand16(int(op["ip_id"])).to_bytes(2, "big")
    h[22], h[23] = 64, 6
    h[26:30], h[30:34] = key[5:9], key[1:5]
    h[34:36], h[36:38] = key[11:13], key[9:11]
    h[38:42], h[42:46] = seq.to_bytes(4, "big"), ack.to_bytes(4, "big")
    h[46], h[47] = 0x50, flags
    h[48:50] = min(int(op["rcv_wnd"]), 65535).to_bytes(2, "big")
    return bytes(h)


def contract(frames, e, openers, reply_flags, mtu, replies, ctl_code):
    """The connect part over the batch's frames (a list of bytes, FCS stripped) and the close part `e`.
    `replies`: the buffer the call is given; a copy with the replies in comes back. `ctl_code`: the close
    call's, a copy with this call's codes in comes back."""
    from seqs_amd.framesum import CONNECT_OUT_DTYPE, DIGEST_DTYPE

    out = np.zeros(len(openers), dtype=CONNECT_OUT_DTYPE)
    buf = np.array(replies, dtype=np.uint8, copy=True)
    dig = np.zeros(len(openers), dtype=DIGEST_DTYPE)
    st = np.zeros(len(openers), dtype=np.uint8)
    ctl = np.array(ctl_code, dtype=np.uint8, copy=True)
    order = e.get("order", ())
    flow_of = {}
    for fl in e.get("flows", ()):
        first, count = int(fl["first_frame"]), int(fl["n_frames"])
        flow_of[flows_ref.flow_key(frames[int(order[first])])] = (first, first + count)
    owing, headers = [], []
    for i, op in enumerate(openers):
        r = Rec(int(op["iss"]))
        span = flow_of.get(bytes(op["key"]))
        if span is not None:
            idx = [int(order[k]) for k in range(*span)]

            def mss_of(k):
                fr = frames[idx[k]]
                l4 = 14 + (fr[14] & 15) * 4
                return peer_mss(fr[l4 + 20 : l4 + 4 * (fr[l4 + 12] >> 4)])

            codes = walk(r, int(op["rcv_wnd"]), [recv_ref.fields(frames[j]) for j in idx], span[0], idx, mss_of)
            assert not ctl[idx].any(), "the close call leaves an opener's frames alone"
            ctl[idx[: len(codes)]] = codes
        if r.reply == REPLY_NONE and int(op["flags"]) & SEND_SYN:
            r.reply = REPLY_SYN
        out[i] = r.record()
        if r.reply != REPLY_NONE:
            owing.append(i)
            headers.append(reply_header(op, r))
    fcs = bool(reply_flags & FCS_APPEND)
    for i, (fr, d) in zip(owing, accept_ref.fill_synacks(headers, mtu, fcs)):
        assert len(fr) == (58 if fcs else 54)
        buf[i * STRIDE : i * STRIDE + len(fr)] = np.frombuffer(fr, dtype=np.uint8)
        dig[i] = d[:3]
        st[i] = d[3]
    return dict(openers_out=out, replies=buf, reply_out=dig, reply_status=st, ctl_code=ctl)


def expected(buf, offsets, lengths, mtu, flags, noise, plead, cap, socks, snd, rings, listeners, slots, synack_flags, synacks,
             closers, openers, reply_flags, replies):
    """close_ref.expected's dict plus the connect call's own arrays; `close_ctl_code` keeps the close call's."""
    e = close_ref.expected(buf, offsets, lengths, mtu, flags, noise, plead, cap, socks, snd, rings, listeners, slots,
                           synack_flags, synacks, closers)
    raw = buf.tobytes()
    room = 4 if flags & flows_ref.RX_FCS else 0
    frames = [raw[int(o) : int(o) + max(0, int(l) - room)] for o, l in zip(offsets, lengths)]
    e["close_ctl_code"] = e["ctl_code"]
    e.update(contract(frames, e, openers, reply_flags, mtu, replies, e["ctl_code"]))
    return e


# ---- 2. the reference, transliterated --------------------------------------------------------------------

SYNACK = SYN | ACK
RST_JUMP = None  # (rstJump: handleRST's ISS step; the contract leaves the listener it makes to the host)


class GoOpener:
    """ControlBlock of a connection that dials (state: the numbers of seqs.go:175-208)."""

    def __init__(self, iss, wnd):
        # Open(iss, wnd, StateSynSent), control_user.go:49
        self.state = SYN_SENT
        self.resetRcv(wnd, 0)
        self.resetSnd(iss, 1)
        self.pending = [SYN, 0]
        self.challengeAck = False
        self.rstPtr = 0
        self.became_listener = False

    def resetSnd(self, localISS, remoteWND):  # control.go:263
        self.snd_ISS = self.snd_UNA = self.snd_NXT = localISS
        self.snd_WND = remoteWND

    def resetRcv(self, localWND, remoteISS):  # control.go:273
        self.rcv_IRS = self.rcv_NXT = remoteISS
        self.rcv_WND = localWND

    def handleRST(self, seq):  # control.go:407
        if seq != self.rcv_NXT:
            self.challengeAck = True
            self.pending[0] |= ACK
            return "errDropSegment"
        # IsPreestablished (seqs.go:213)
        self.pending[0] = 0
        self.state = LISTEN
        self.became_listener = True  # (resetSnd(ISS + rstJump, WND), resetRcv(WND, 3141592653 ^ IRS): left to the host)
        return "errDropSegment"

    def validateIncomingSegment(self, seg):  # control.go:281
        flags = seg.Flags
        hasAck = flags & ACK == ACK
        checkSEQ = not flags & SYN
        established = self.state == ESTABLISHED
        preestablished = self.state in (SYN_RCVD, SYN_SENT, LISTEN)
        acksOld = hasAck and not go_less_than(self.snd_UNA, seg.ACK)
        acksUnsentData = hasAck and not go_less_than_eq(seg.ACK, self.snd_NXT)
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
        if flags & RST:
            return self.handleRST(seg.SEQ)
        assert not established
        if preestablished and (acksOld or acksUnsentData):
            err = "errDropSegment"
            self.pending[0] = RST
            self.rstPtr = seg.ACK
            self.resetSnd(self.snd_ISS, seg.WND)
        return err

    def rcvSynSent(self, seg):  # control.go:175
        hasSyn, hasAck = bool(seg.Flags & SYN), bool(seg.Flags & ACK)
        err = None
        if not hasSyn:
            err = "errExpectedSYN"
        elif hasAck and seg.ACK != (self.snd_UNA + 1) % M32:
            err = "errBadSegack"
        if err is not None:
            return 0, err
        if hasAck:
            self.state = ESTABLISHED
            pending = ACK
            self.resetRcv(self.rcv_WND, seg.SEQ)
        else:
            pending = SYNACK
            self.state = SYN_RCVD
            self.resetSnd(self.snd_ISS, seg.WND)
            self.resetRcv(self.rcv_WND, seg.SEQ)
        return pending, None

    def Recv(self, seg):  # control_user.go:164
        err = self.validateIncomingSegment(seg)
        if err is not None:
            return err
        assert self.state == SYN_SENT
        pending, err = self.rcvSynSent(seg)
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

    def PendingSegment(self, payloadLen):  # control.go:100
        if self.challengeAck:
            self.challengeAck = False
            return Segment(self.snd_NXT, self.rcv_NXT, self.rcv_WND, ACK, 0), True
        pending = self.pending[0]
        established = self.state == ESTABLISHED
        if not established:
            payloadLen = 0
        if pending == 0 and payloadLen == 0:
            return None, False
        if established:
            pending |= ACK
        ack = self.rcv_NXT if pending & ACK else 0
        seq = self.rstPtr if pending & RST else self.snd_NXT
        return Segment(seq, ack, self.rcv_WND, pending, payloadLen), True

    def validateOutgoingSegment(self, seg):  # control.go:353
        hasAck = bool(seg.Flags & ACK)
        checkSeq = not seg.Flags & RST
        zeroWindowOK = self.snd_WND == 0 and seg.DATALEN == 0 and seg.SEQ == self.snd_NXT
        outOfWindow = checkSeq and not go_in_window(seg.SEQ, self.snd_NXT, self.snd_WND) and not zeroWindowOK
        if seg.WND > 0xFFFF:
            return "errWindowTooLarge"
        if hasAck and seg.ACK != self.rcv_NXT:
            return "errAckNotNext"
        if outOfWindow:
            return "errZeroWindow" if self.snd_WND == 0 else "errSeqNotInWindow"
        if checkSeq and not go_in_window(seg.Last(), self.snd_NXT, self.snd_WND) and not zeroWindowOK:
            return "errLastNotInWindow"
        return None

    def Send(self, seg):  # control_user.go:106
        err = self.validateOutgoingSegment(seg)
        if err is not None:
            return err
        self.pending[0] &= ~seg.Flags
        if self.pending[0] == 0:
            self.pending = [self.pending[1] & ~(seg.Flags & FIN), 0]
        self.snd_NXT = go_add(self.snd_NXT, seg.LEN())
        self.rcv_WND = seg.WND
        return None

    def synsentSegment(self):  # tcpconn.go:477
        return Segment(self.snd_ISS, 0, self.rcv_WND, SYN, 0)


def go_dial(iss, wnd):
    """openstack's control part (stacks/tcpconn.go:282-293): Open, then Send of the first SYN, so that
    snd.NXT = iss + 1 (a window above 65,535 is the caller's: Open refuses it, the contract clamps the field)."""
    tcb = GoOpener(iss, wnd)
    err = tcb.Send(tcb.synsentSegment()) if wnd <= 0xFFFF else None
    if wnd > 0xFFFF:
        tcb.snd_NXT, tcb.pending = go_add(tcb.snd_NXT, 1), [0, 0]
    assert err is None and tcb.snd_NXT == (iss + 1) % M32 and tcb.pending == [0, 0]
    return tcb


def go_recv(tcb, seg):
    """TCPConn.recv's control part for one segment (stacks/tcpconn.go:334-361): "keepalive", or Recv's error
    (None: admitted)."""
    if tcb.IncomingIsKeepalive(seg):  # tcpconn.go:349
        return "keepalive"
    return tcb.Recv(seg)


def go_headers(seg, op, ip_id) -> bytes:
    """setSrcDest (tcpconn.go:433-441) and CalculateHeaders (port_tcp.go:162-194) for a segment without
    payload of the opener `op`, checksum fields zero; `ip_id`: the packet's ID before this frame."""
    key = bytes(op["key"])
    h = bytearray(54)
    h[0:6], h[6:12], h[12:14] = bytes(op["remote_mac"]), bytes(op["local_mac"]), b"\x08\x00"
    h[14] = 0x45
    h[16:18] = (4 * 5 + 20).to_bytes(2, "big")
    h[18:20] = prand16(ip_id).to_bytes(2, "big")
    h[22], h[23] = 64, 6
    h[26:30], h[30:34] = key[5:9], key[1:5]
    h[34:36], h[36:38] = key[11:13], key[9:11]
    h[38:42], h[42:46] = seg.SEQ.to_bytes(4, "big"), seg.ACK.to_bytes(4, "big")
    h[46] = (5 << 4) | ((seg.Flags >> 8) & 1)
    h[47] = seg.Flags & 0xFF
    h[48:50] = (seg.WND & 0xFFFF).to_bytes(2, "big")  # uint16(seg.WND)
    return bytes(h)
