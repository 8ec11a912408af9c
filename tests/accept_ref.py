"""The expected output of the accept call (fs_accept_flows_batch), restated twice with code the kernels do
not share.

contract(): the rules of include/framesum_accept.h, sequentially in Python integers, on top of
tests/recv_ref.py's dict (the flows, their order, the sockets' flows). expected() is recv_ref.expected's
dict plus conns, listeners_out, accept_of, the whole synacks buffer, synack_out and synack_status. The
SYN-ACK's checksums and FCS come from oracle/pyref.py.

GoListener: a literal transliteration of the reference's first-SYN path, branch for branch, in the manner
of tests/recv_ref.py's GoBlock: TCPListener.recv (stacks/tcplistener.go:128-164), TCPConn.recv
(stacks/tcpconn.go:334-381), validateIncomingSegment (control.go:281-351), rcvListen (control.go:157-173),
Recv (control_user.go:164-224), PendingSegment (control.go:100-152), Send (control_user.go:106-158, with
validateOutgoingSegment, control.go:353-386) and CalculateHeaders (stacks/port_tcp.go:162-194). It knows
nothing of flows, slots or batches."""
import numpy as np

import flows_ref
import recv_ref
from oracle import pyref
from recv_ref import ACK, FIN, M32, NS, RST, SYN, go_add, go_in_window, go_less_than, go_less_than_eq  # noqa: F401

NONE, FULL = 0xFFFFFFFF, 0xFFFFFFFE
STRIDE = 64
FCS_APPEND = 2
SYNACK = SYN | ACK


def prand16(x):
    x ^= (x << 7) & 0xFFFF
    x ^= x >> 9
    x ^= (x << 8) & 0xFFFF
    return x


def listeners_of(*rows):
    """A LISTENER_DTYPE array of (local 6 bytes, mac 6 bytes, slot_first, n_slots) rows."""
    from seqs_amd.framesum import LISTENER_DTYPE

    a = np.zeros(len(rows), dtype=LISTENER_DTYPE)
    for i, (local, mac, first, count) in enumerate(rows):
        a["local"][i] = np.frombuffer(bytes(local), dtype=np.uint8)
        a["mac"][i] = np.frombuffer(bytes(mac), dtype=np.uint8)
        a["slot_first"][i], a["n_slots"][i] = first, count
    return a


def slots_of(*rows):
    """An ACCEPT_SLOT_DTYPE array of (iss, rcv_wnd, ip_id) rows."""
    from seqs_amd.framesum import ACCEPT_SLOT_DTYPE

    a = np.zeros(len(rows), dtype=ACCEPT_SLOT_DTYPE)
    for i, (iss, wnd, ident) in enumerate(rows):
        a[i] = (iss % M32, wnd, ident, 0)
    return a


def local_of(fr: bytes) -> bytes:
    """The destination address and port of a frame, as a listener's `local` holds them."""
    l4 = 14 + (fr[14] & 15) * 4
    return bytes(fr[30:34]) + bytes(fr[l4 + 2 : l4 + 4])


# ---- 1. the contract ---------------------------------------------------------------------------------

def peer_mss(opt: bytes) -> int:
    at = 0
    for _ in range(40):
        if at >= len(opt):
            break
        kind = opt[at]
        if kind == 0:
            break
        if kind == 1:
            at += 1
            continue
        if at + 1 >= len(opt):
            break
        length = opt[at + 1]
        if length < 2 or at + length > len(opt):
            break
        if kind == 2 and length == 4:
            return (opt[at + 2] << 8) | opt[at + 3]
        at += length
    return 0


def is_first_syn(fr: bytes) -> bool:
    """Rule 2 without the socket and the listener, for an accepted frame."""
    if fr[23] != 6:
        return False
    seq, ack, window, flags9, length = recv_ref.fields(fr)
    return flags9 == SYN and ack == 0 and length == 0


def synack_header(fr: bytes, mac: bytes, iss: int, rcv_wnd: int, ip_id: int) -> bytes:
    """The SYN-ACK that answers the SYN `fr`, field by field as the header lists them, its checksum
    fields still zero."""
    l4 = 14 + (fr[14] & 15) * 4
    seq = int.from_bytes(fr[l4 + 4 : l4 + 8], "big")
    h = bytearray(54)
    h[0:6], h[6:12], h[12:14] = fr[6:12], mac, b"\x08\x00"
    h[14], h[15] = 0x45, 0
    h[16:18] = (40).to_bytes(2, "big")
    h[18:20] = prand16(ip_id).to_bytes(2, "big")
    h[20:22] = b"\x00\x00"
    h[22], h[23] = 64, 6
    h[26:30], h[30:34] = fr[30:34], fr[26:30]
    h[34:36], h[36:38] = fr[l4 + 2 : l4 + 4], fr[l4 : l4 + 2]
    h[38:42] = (iss % M32).to_bytes(4, "big")
    h[42:46] = ((seq + 1) % M32).to_bytes(4, "big")
    h[46], h[47] = 0x50, SYNACK
    h[48:50] = min(rcv_wnd, 65535).to_bytes(2, "big")
    return bytes(h)


PYREF_MOST = 600  # headers: beyond that many the C oracle fills (tests/test_oracle.py holds the two together)


def fill_synacks(headers, mtu: int, fcs: bool):
    """[(the finished frame with its FCS when `fcs`, (crc32, ip_csum, l4_csum, verdict))] of the headers:
    checksums, FCS and digest by oracle/pyref.py; by the C oracle for a batch of more than PYREF_MOST."""
    flags = pyref.FILL_CSUM | (pyref.FCS_APPEND if fcs else 0)
    if len(headers) <= PYREF_MOST:
        return [pyref.fill_frame(h, mtu, flags) for h in headers]
    from oracle import coracle

    n = len(headers)
    buf = np.zeros(n * STRIDE + 8, dtype=np.uint8)
    offs = np.arange(n, dtype=np.uint64) * np.uint64(STRIDE)
    lens = np.full(n, 54, dtype=np.uint32)
    buf[: n * STRIDE].reshape(n, STRIDE)[:, :54] = np.frombuffer(b"".join(headers), dtype=np.uint8).reshape(n, 54)
    dig, st = coracle.fill_batch(buf, offs, lens, mtu, flags)
    size = 58 if fcs else 54
    rows = buf[: n * STRIDE].reshape(n, STRIDE)
    return [(rows[k, :size].tobytes(), (int(dig["crc32"][k]), int(dig["ip_csum"][k]), int(dig["l4_csum"][k]), int(st[k])))
            for k in range(n)]


def contract(frames, e, socks, listeners, slots, synack_flags, mtu, synacks):
    """The accept part over the batch's frames (a list of bytes, FCS stripped) and the receive part `e`.
    `synacks`: the buffer the call is given; a copy with the SYN-ACKs in comes back."""
    from seqs_amd.framesum import ACCEPT_CONN_DTYPE, DIGEST_DTYPE, LISTENER_OUT_DTYPE

    n = len(frames)
    conns = np.zeros(len(slots), dtype=ACCEPT_CONN_DTYPE)
    lout = np.zeros(len(listeners), dtype=LISTENER_OUT_DTYPE)
    accept_of = np.full(n, NONE, dtype=np.uint32)
    out = np.array(synacks, dtype=np.uint8, copy=True)
    syn_dig = np.zeros(len(slots), dtype=DIGEST_DTYPE)
    syn_st = np.zeros(len(slots), dtype=np.uint8)
    have_sock = {bytes(s["key"]) for s in socks}
    by_local = {bytes(l["local"]): i for i, l in enumerate(listeners)}
    taken, filled, headers = [0] * len(listeners), [], []
    for f, fl in enumerate(e["flows"]):
        i = int(e["order"][int(fl["first_frame"])])
        fr = frames[i]
        key = flows_ref.flow_key(fr)
        if key in have_sock or not is_first_syn(fr) or local_of(fr) not in by_local:
            continue
        li = by_local[local_of(fr)]
        lis = listeners[li]
        r = taken[li]
        taken[li] += 1
        if r >= int(lis["n_slots"]):
            accept_of[f] = FULL
            continue
        slot = int(lis["slot_first"]) + r
        accept_of[f] = slot
        sl = slots[slot]
        l4 = 14 + (fr[14] & 15) * 4
        seq, _, window, _, _ = recv_ref.fields(fr)
        c = conns[slot]
        c["key"], c["used"], c["remote_mac"] = np.frombuffer(key, dtype=np.uint8), 1, np.frombuffer(fr[6:12], dtype=np.uint8)
        c["peer_mss"] = peer_mss(fr[l4 + 20 : l4 + 4 * (fr[l4 + 12] >> 4)])
        c["frame"], c["flow"], c["irs"], c["rcv_nxt"] = i, f, seq, (seq + 1) % M32
        c["snd_nxt"], c["snd_wnd"] = (int(sl["iss"]) + 1) % M32, window
        filled.append(slot)
        headers.append(synack_header(fr, bytes(lis["mac"]), int(sl["iss"]), int(sl["rcv_wnd"]), int(sl["ip_id"])))
    fcs = bool(synack_flags & FCS_APPEND)
    for slot, (sa, dig) in zip(filled, fill_synacks(headers, mtu, fcs)):
        assert len(sa) == (58 if fcs else 54)
        out[slot * STRIDE : slot * STRIDE + len(sa)] = np.frombuffer(sa, dtype=np.uint8)
        syn_dig[slot] = dig[:3]
        syn_st[slot] = dig[3]
    for li in range(len(listeners)):
        acc = min(taken[li], int(listeners[li]["n_slots"]))
        lout[li] = (taken[li], acc, taken[li] - acc, 0)
    return dict(conns=conns, listeners_out=lout, accept_of=accept_of, synacks=out, synack_out=syn_dig, synack_status=syn_st)


def expected(buf, offsets, lengths, mtu, flags, noise, plead, cap, socks, snd, rings, listeners, slots, synack_flags, synacks):
    """recv_ref.expected's dict plus the accept call's own arrays."""
    e = recv_ref.expected(buf, offsets, lengths, mtu, flags, noise, plead, cap, socks, snd, rings)
    raw = buf.tobytes()
    room = 4 if flags & flows_ref.RX_FCS else 0
    frames = [raw[int(o) : int(o) + max(0, int(l) - room)] for o, l in zip(offsets, lengths)]
    e.update(contract(frames, e, socks, listeners, slots, synack_flags, mtu, synacks))
    return e


# ---- 2. the reference, transliterated ----------------------------------------------------------------

STATE_LISTEN, STATE_SYN_RCVD, STATE_CLOSED = "Listen", "SynRcvd", "Closed"


class GoTCB:
    """ControlBlock as freeConnForReuse leaves it (tcplistener.go:178-185: open(StateListen, port, iss)):
    snd.ISS = iss, rcv.WND = the connection's window."""

    def __init__(self, iss, rcv_wnd):
        self.state = STATE_LISTEN
        self.snd_ISS = self.snd_UNA = self.snd_NXT = iss
        self.snd_WND = 0
        self.rcv_IRS = self.rcv_NXT = 0
        self.rcv_WND = rcv_wnd
        self.pending = [0, 0]
        self.challengeAck = False

    def validateIncomingSegment(self, seg):  # control.go:281
        flags = seg.Flags
        hasAck = flags & ACK == ACK
        checkSEQ = not flags & SYN
        established = False
        preestablished = True  # StateListen, StateSynRcvd
        acksOld = hasAck and not go_less_than(self.snd_UNA, seg.ACK)
        acksUnsentData = hasAck and not go_less_than_eq(seg.ACK, self.snd_NXT)
        zeroWindowOK = self.rcv_WND == 0 and seg.DATALEN == 0 and seg.SEQ == self.rcv_NXT
        err = None
        if seg.WND > 0xFFFF:
            err = "errWindowOverflow"
        elif self.state == STATE_CLOSED:
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
            return "handleRST"  # (TCPListener.recv hands only Flags == SYN to a Listen connection)
        if established:
            pass
        elif preestablished and (acksOld or acksUnsentData):
            err = "errDropSegment"
            self.pending[0] = RST
        return err

    def rcvListen(self, seg):  # control.go:157
        err = None
        if not seg.Flags & SYN == SYN:
            err = "errExpectedSYN"
        if err is not None:
            return 0, err
        self.resetSnd(self.snd_ISS, seg.WND)
        self.resetRcv(self.rcv_WND, seg.SEQ)
        self.pending[0] = SYNACK
        self.state = STATE_SYN_RCVD
        return SYNACK, None

    def resetSnd(self, localISS, remoteWND):  # control.go:263
        self.snd_ISS = self.snd_UNA = self.snd_NXT = localISS
        self.snd_WND = remoteWND

    def resetRcv(self, localWND, remoteISS):  # control.go:273
        self.rcv_IRS = self.rcv_NXT = remoteISS
        self.rcv_WND = localWND

    def Recv(self, seg):  # control_user.go:164
        err = self.validateIncomingSegment(seg)
        if err is not None:
            return err
        assert self.state == STATE_LISTEN
        pending, err = self.rcvListen(seg)
        if err is not None:
            return err
        self.pending[0] |= pending
        self.snd_WND = seg.WND
        if seg.Flags & ACK:
            self.snd_UNA = seg.ACK
        self.rcv_NXT = go_add(self.rcv_NXT, seg.LEN())
        return None

    def PendingSegment(self, payloadLen):  # control.go:100
        if self.challengeAck:
            self.challengeAck = False
            return recv_ref.Segment(self.snd_NXT, self.rcv_NXT, self.rcv_WND, ACK, 0), True
        pending = self.pending[0]
        established = False
        if not established:
            payloadLen = 0
        if pending == 0 and payloadLen == 0:
            return None, False
        ack = self.rcv_NXT if pending & ACK else 0
        seq = self.snd_NXT
        return recv_ref.Segment(seq, ack, self.rcv_WND, pending, payloadLen), True

    def validateOutgoingSegment(self, seg):  # control.go:353
        hasAck = bool(seg.Flags & ACK)
        checkSeq = not seg.Flags & RST
        seglast = seg.Last()
        zeroWindowOK = self.snd_WND == 0 and seg.DATALEN == 0 and seg.SEQ == self.snd_NXT
        outOfWindow = checkSeq and not go_in_window(seg.SEQ, self.snd_NXT, self.snd_WND) and not zeroWindowOK
        err = None
        if self.state == STATE_CLOSED:
            err = "ErrClosedPipe"
        elif seg.WND > 0xFFFF:
            err = "errWindowTooLarge"
        elif hasAck and seg.ACK != self.rcv_NXT:
            err = "errAckNotNext"
        elif outOfWindow:
            err = "errZeroWindow" if self.snd_WND == 0 else "errSeqNotInWindow"
        elif checkSeq and self.snd_WND == 0 and seg.DATALEN > 0 and seg.SEQ == self.snd_NXT:
            err = "errZeroWindow"
        elif checkSeq and not go_in_window(seglast, self.snd_NXT, self.snd_WND) and not zeroWindowOK:
            err = "errLastNotInWindow"
        return err

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


class GoConn:
    """TCPConn in a listener's pool: the control block, the remote and the IPv4 ID of its packet."""

    def __init__(self, iss, rcv_wnd, ip_id):
        self.scb, self.remote, self.remoteMAC, self.ip_id = GoTCB(iss, rcv_wnd), None, None, ip_id
        self.rx = b""

    def recv(self, fr):  # tcpconn.go:334
        if self.scb.state == STATE_CLOSED:
            return "EOF"
        l4 = 14 + (fr[14] & 15) * 4
        sport = int.from_bytes(fr[l4 : l4 + 2], "big")
        if self.remote is not None and self.remote[1] != 0 and sport != self.remote[1]:
            return None
        seq, ack, window, flags9, length = recv_ref.fields(fr)
        seg = recv_ref.Segment(seq, ack, window, flags9, length)
        # IncomingIsKeepalive (control_user.go:260): Flags == ACK cannot hold for a SYN
        if seg.SEQ == (self.scb.rcv_NXT - 1) % M32 and seg.Flags == ACK and seg.ACK == self.scb.snd_NXT and seg.DATALEN == 0:
            return None
        err = self.scb.Recv(seg)
        if err is not None:
            return None  # "Segment not admitted, yield to sender."
        if seg.DATALEN > 0:
            a, b = flows_ref.payload_range(fr)
            self.rx += fr[a:b]
        if seg.Flags & SYN and self.remote is None:
            self.remoteMAC = bytes(fr[6:12])
            self.remote = (bytes(fr[26:30]), sport)
        return None

    def send(self, local_ip, local_port, mac):  # tcpconn.go:383 and CalculateHeaders, port_tcp.go:162
        if self.remote is None:
            return None
        seg, ok = self.scb.PendingSegment(0)
        if not ok:
            return None
        err = self.scb.Send(seg)
        if err is not None:
            return err
        self.ip_id = prand16(self.ip_id)
        h = bytearray(54)
        h[0:6], h[6:12], h[12:14] = self.remoteMAC, mac, b"\x08\x00"
        h[14] = 0x45
        h[16:18] = (4 * 5 + 20).to_bytes(2, "big")
        h[18:20] = self.ip_id.to_bytes(2, "big")
        h[22], h[23] = 64, 6
        h[26:30], h[30:34] = local_ip, self.remote[0]
        h[34:36], h[36:38] = local_port.to_bytes(2, "big"), self.remote[1].to_bytes(2, "big")
        h[38:42], h[42:46] = seg.SEQ.to_bytes(4, "big"), seg.ACK.to_bytes(4, "big")
        h[46] = 5 << 4
        h[46] |= (seg.Flags >> 8) & 1
        h[47] = seg.Flags & 0xFF
        h[48:50] = (seg.WND & 0xFFFF).to_bytes(2, "big")  # uint16(seg.WND)
        return pyref.fill_frame(bytes(h))[0]


class GoListener:
    """TCPListener: the pool of connections in the order freeConnForReuse prepared them."""

    def __init__(self, local_ip, port, mac, conns):
        self.ip, self.port, self.mac, self.conns = bytes(local_ip), port, bytes(mac), conns
        self.used = [False] * len(conns)

    def recv(self, fr):  # tcplistener.go:128
        """Returns (error, the index of the connection that took the frame or None)."""
        l4 = 14 + (fr[14] & 15) * 4
        seq, ack, window, flags9, length = recv_ref.fields(fr)
        isSYN = flags9 == SYN
        sport = int.from_bytes(fr[l4 : l4 + 2], "big")
        freeconn = None
        for connidx, conn in enumerate(self.conns):
            if ack == 0 and isSYN and not self.used[connidx] and conn.scb.state == STATE_LISTEN:
                freeconn = connidx
                break
            if conn.remote is None or sport != conn.remote[1] or bytes(fr[26:30]) != conn.remote[0]:
                continue
            return conn.recv(fr), connidx
        if freeconn is None:
            return "ErrDroppedPacket", None
        err = self.conns[freeconn].recv(fr)  # (`used` is Accept's: a connection that left Listen is no free one)
        return err, freeconn

    def send(self, connidx):
        return self.conns[connidx].send(self.ip, self.port, self.mac)
