"""The ARP call's contract (include/framesum_arp.h) stated twice, with code the kernels do not share.

expected(): from the header's rules, in Python integers and bytes: the candidates by verdict, the support
check, the match of a request to a host by ProtoTarget and MAC filter, the rank in batch order and the
admission by `free`, the match of a reply to a query and the lowest batch index that resolves it, the built
frames with their padding, FCS, digest and verdict.

recv_eth_model(): a branch-for-branch transliteration of PortStack.RecvEth's Ethernet block and ARP branch
(stacks/portstack.go:185, 191-197) and of arpClient.recv, handle and BeginResolve (stacks/arp.go:60-76,
98-166), driving one model client per host: every host is a PortStack on the same wire and sees every frame.
The two statements differ only in the header's stated differences, each of which the model can switch back
to the reference's behaviour (`faithful`):
  (a) the reference holds ONE pendingResponse, the call `free` slots (faithful: at most one);
  (b) the reference drops a frame with a foreign destination MAC before the support check (faithful: such a
      frame is IGNORED even when malformed; the call says UNSUPPORTED);
  (c) the reference keeps the whole reply header as its result; the model does too, and the out record takes
      HardwareSender from it (faithful: `result` is returned beside the tuple);
  (d) the reference has one `result` per client; the call several queries per host (faithful: a later
      BeginResolve of the same client replaces the earlier one, arp.go:34).
tests/test_arp_host.py reaches each.

Verdicts are an input (`status`): the CPU oracle's in the GPU tests, pyref's in the CPU tests.
"""
import zlib

import numpy as np

from oracle import pyref

NONE = 0xFFFFFFFF
STRIDE = 64
PAD, FCS_APPEND = 1, 2
SEND_REQUEST = 1
NOT_ARP, UNSUPPORTED, IGNORED, ANSWERED, FULL, RESOLVED, STALE = range(7)
Q_WAIT, Q_DONE, Q_SENT = range(3)
FS_ARP = 4
BROADCAST = b"\xff" * 6
OP_WAIT = 0xFFFF  # arpOpWait

HOST_DTYPE = np.dtype([("ip", "u1", (4,)), ("mac", "u1", (6,)), ("reserved", "<u2"), ("slot0", "<u4"), ("free", "<u4")])
QUERY_DTYPE = np.dtype([("host", "<u4"), ("target", "u1", (4,)), ("flags", "<u2"), ("reserved", "<u2")])
HOST_OUT_DTYPE = np.dtype([("n_requests", "<u4"), ("n_answered", "<u4"), ("first", "<u4"), ("free", "<u4")])
QUERY_OUT_DTYPE = np.dtype([("state", "u1"), ("reserved", "u1"), ("mac", "u1", (6,)), ("frame", "<u4"), ("n_replies", "<u4")])
DIGEST_DTYPE = np.dtype([("crc32", "<u4"), ("ip_csum", "<u2"), ("l4_csum", "<u2")])


# ---- frames and rows -------------------------------------------------------------------------------------------
def ip4(a) -> bytes:
    if isinstance(a, str):
        return bytes(int(x) for x in a.split("."))
    if isinstance(a, int):
        return a.to_bytes(4, "big")
    return bytes(a)


def mac6(m) -> bytes:
    if isinstance(m, str):
        return bytes(int(x, 16) for x in m.split(":"))
    if isinstance(m, int):
        return m.to_bytes(6, "big")
    return bytes(m)


def arp_frame(op, sha, spa, tha, tpa, dst=BROADCAST, src=None, htype=1, ptype=0x0800, hlen=6, plen=4, pad=b"",
              etype=0x0806) -> bytes:
    """An Ethernet / ARP frame: 42 bytes and `pad` behind them."""
    sha, tha = mac6(sha), mac6(tha)
    hdr = (htype.to_bytes(2, "big") + ptype.to_bytes(2, "big") + bytes([hlen, plen]) + op.to_bytes(2, "big") + sha + ip4(spa) +
           tha + ip4(tpa))
    return mac6(dst) + (sha if src is None else mac6(src)) + etype.to_bytes(2, "big") + hdr + bytes(pad)


def who_has(sha, spa, tpa, dst=BROADCAST, **kw) -> bytes:
    return arp_frame(1, sha, spa, b"\0" * 6, tpa, dst=dst, **kw)


def is_at(sha, spa, tha, tpa, dst=None, **kw) -> bytes:
    return arp_frame(2, sha, spa, tha, tpa, dst=tha if dst is None else dst, **kw)


def host_row(ip, mac, slot0=0, free=1):
    row = np.zeros(1, dtype=HOST_DTYPE)
    row["ip"][0] = np.frombuffer(ip4(ip), dtype=np.uint8)
    row["mac"][0] = np.frombuffer(mac6(mac), dtype=np.uint8)
    row["slot0"], row["free"] = slot0, free
    return row


def query_row(host, target, send=False):
    row = np.zeros(1, dtype=QUERY_DTYPE)
    row["host"], row["flags"] = host, SEND_REQUEST if send else 0
    row["target"][0] = np.frombuffer(ip4(target), dtype=np.uint8)
    return row


def hosts_of(rows):
    """The rows as one HOST_DTYPE array with their slot ranges behind each other; returns (hosts, n_reply_slots)."""
    hosts = np.concatenate(rows) if len(rows) else np.zeros(0, dtype=HOST_DTYPE)
    at = 0
    for h in hosts:
        h["slot0"] = at
        at += int(h["free"])
    return hosts, at


def queries_of(rows):
    return np.concatenate(rows) if len(rows) else np.zeros(0, dtype=QUERY_DTYPE)


def verdicts(frames, mtu=0, fcs=False) -> np.ndarray:
    return np.array([(pyref.frame_digest_fcs(f, mtu) if fcs else pyref.frame_digest(f, mtu))[3] for f in frames], dtype=np.uint8)


def built(eth_dst, host_mac, op, host_ip, tha, tpa, arp_flags) -> bytes:
    """A built frame as rule 9 has it: the 42 bytes, the zero fill, the FCS."""
    f = arp_frame(op, host_mac, host_ip, tha, tpa, dst=eth_dst, src=host_mac)
    if arp_flags & PAD:
        f += b"\0" * 18
    if arp_flags & FCS_APPEND:
        f += zlib.crc32(f).to_bytes(4, "little")
    return f


def digest_of(frame: bytes, arp_flags: int, mtu: int):
    """(crc32, ip_csum, l4_csum, verdict) of a built frame, the FCS not counted."""
    body = frame[:-4] if arp_flags & FCS_APPEND else frame
    verdict, ip_csum, l4 = pyref.recv_eth(body, mtu)
    return zlib.crc32(body), ip_csum, l4, verdict


class Results:
    """The seven arrays of a call, prefilled as the caller's."""

    def __init__(self, n, hosts, queries, n_reply_slots, frames0=None, out0=None, st0=None):
        slots = n_reply_slots + len(queries)
        self.hosts_out = np.zeros(len(hosts), dtype=HOST_OUT_DTYPE)
        self.queries_out = np.zeros(len(queries), dtype=QUERY_OUT_DTYPE)
        self.frames = np.zeros(slots * STRIDE, dtype=np.uint8) if frames0 is None else np.array(frames0, dtype=np.uint8, copy=True)
        self.out = np.zeros(slots, dtype=DIGEST_DTYPE) if out0 is None else np.array(out0, dtype=DIGEST_DTYPE, copy=True)
        self.status = np.zeros(slots, dtype=np.uint8) if st0 is None else np.array(st0, dtype=np.uint8, copy=True)
        self.code = np.zeros(n, dtype=np.uint8)
        self.of = np.full(n, NONE, dtype=np.uint32)

    def put(self, slot, frame, arp_flags, mtu):
        self.frames[slot * STRIDE : slot * STRIDE + len(frame)] = np.frombuffer(frame, dtype=np.uint8)
        crc, ip_csum, l4, verdict = digest_of(frame, arp_flags, mtu)
        self.out[slot] = (crc, ip_csum, l4)
        self.status[slot] = verdict

    def tuple(self):
        return self.hosts_out, self.queries_out, self.frames, self.out, self.status, self.code, self.of


# ---- statement 1: the header's rules ----------------------------------------------------------------------------
def expected(frames, status, hosts, queries, n_reply_slots, arp_flags=0, frames0=None, out0=None, st0=None, mtu=0, fcs=False):
    """(hosts_out, queries_out, arp_frames, arp_out, arp_status, arp_code, arp_of) of one call over `frames`
    (a list of bytes, the FCS still on them when `fcs`) with verdicts `status`."""
    hosts, queries = np.atleast_1d(hosts), np.atleast_1d(queries)
    res = Results(len(frames), hosts, queries, n_reply_slots, frames0, out0, st0)
    by_ip = {bytes(h["ip"]): k for k, h in reversed(list(enumerate(hosts)))}
    by_key = {(int(q["host"]), bytes(q["target"])): k for k, q in reversed(list(enumerate(queries)))}
    res.hosts_out["first"], res.hosts_out["free"] = NONE, hosts["free"]
    res.queries_out["frame"] = NONE
    for k, q in enumerate(queries):
        res.queries_out[k]["state"] = Q_SENT if int(q["flags"]) & SEND_REQUEST else Q_WAIT
    for i, f in enumerate(frames):
        if int(status[i]) != FS_ARP:  # rule 2
            continue
        dst, a = bytes(f[0:6]), bytes(f[14:42])
        htype, ptype, hlen, plen, op = int.from_bytes(a[0:2], "big"), int.from_bytes(a[2:4], "big"), a[4], a[5], int.from_bytes(a[6:8], "big")
        sha, spa, tpa = a[8:14], a[14:18], a[24:28]
        if not (htype == 1 and ptype == 0x0800 and hlen == 6 and plen == 4 and op in (1, 2)):  # rule 3
            res.code[i] = UNSUPPORTED
            continue
        res.code[i] = IGNORED
        h = by_ip.get(tpa)
        if h is None or not (dst == BROADCAST or dst == bytes(hosts[h]["mac"])):
            continue
        host, o = hosts[h], res.hosts_out[h]
        if op == 1:  # rule 4
            r = int(o["n_requests"])
            if r == 0:
                o["first"] = i
            o["n_requests"] += 1
            if r >= int(host["free"]):
                res.code[i] = FULL
                continue
            slot = int(host["slot0"]) + r
            res.code[i], res.of[i] = ANSWERED, slot
            o["n_answered"] += 1
            o["free"] -= 1
            res.put(slot, built(sha, bytes(host["mac"]), 2, bytes(host["ip"]), sha, spa, arp_flags), arp_flags, mtu)
            continue
        q = by_key.get((h, spa))  # rule 5
        if q is None or int(queries[q]["flags"]) & SEND_REQUEST:
            continue
        qo = res.queries_out[q]
        res.of[i] = q
        qo["n_replies"] += 1
        if int(qo["state"]) == Q_DONE:
            res.code[i] = STALE
            continue
        res.code[i] = RESOLVED
        qo["state"], qo["frame"] = Q_DONE, i
        qo["mac"] = np.frombuffer(sha, dtype=np.uint8)
    for k, q in enumerate(queries):  # rule 6
        if int(q["flags"]) & SEND_REQUEST:
            host = hosts[int(q["host"])]
            res.put(n_reply_slots + k, built(BROADCAST, bytes(host["mac"]), 1, bytes(host["ip"]), b"\0" * 6, bytes(q["target"]),
                                             arp_flags), arp_flags, mtu)
    return res.tuple()


# ---- statement 2: RecvEth's ARP branch and arpClient, frame by frame ---------------------------------------------
class ARPv4Header:  # eth.ARPv4Header
    def __init__(self, **kw):
        self.HardwareType = self.ProtoType = self.HardwareLength = self.ProtoLength = self.Operation = 0
        self.HardwareSender = self.HardwareTarget = b"\0" * 6
        self.ProtoSender = self.ProtoTarget = b"\0" * 4
        self.__dict__.update(kw)

    def put(self) -> bytes:
        return (self.HardwareType.to_bytes(2, "big") + self.ProtoType.to_bytes(2, "big") +
                bytes([self.HardwareLength, self.ProtoLength]) + self.Operation.to_bytes(2, "big") + self.HardwareSender +
                self.ProtoSender + self.HardwareTarget + self.ProtoTarget)


def decode_arp(b: bytes) -> ARPv4Header:  # eth.DecodeARPv4Header
    return ARPv4Header(HardwareType=int.from_bytes(b[0:2], "big"), ProtoType=int.from_bytes(b[2:4], "big"), HardwareLength=b[4],
                       ProtoLength=b[5], Operation=int.from_bytes(b[6:8], "big"), HardwareSender=bytes(b[8:14]),
                       ProtoSender=bytes(b[14:18]), HardwareTarget=bytes(b[18:24]), ProtoTarget=bytes(b[24:28]))


class ModelClient:
    """One host as a PortStack with its arpClient. `results`: the client's `result`, one per query of the host
    (difference (d); faithful: one, the last BeginResolve's). `pending`: its pendingResponse, `free` of them
    (difference (a); faithful: one)."""

    def __init__(self, index, row, faithful):
        self.index, self.ip, self.mac = index, bytes(row["ip"]), bytes(row["mac"])
        self.free = min(int(row["free"]), 1) if faithful else int(row["free"])
        self.faithful = faithful
        self.results = {}  # query number -> ARPv4Header
        self.pending = []  # (frame index, ARPv4Header)
        self.seen = []     # every request for this host that passed the filters, in arrival order
        self.counts = {}   # query number -> replies that matched it
        self.won = {}      # query number -> batch index of the reply kept as the result

    def begin_resolve(self, q, target):  # arp.go:60-76
        if self.faithful:
            self.results.clear()  # "If BeginResolveARPv4 is called at any point in resolution, the state is reset"
        self.results[q] = ARPv4Header(Operation=1, HardwareType=1, ProtoType=0x0800, HardwareLength=6, ProtoLength=4,
                                      HardwareSender=self.mac, ProtoSender=self.ip, HardwareTarget=b"\0" * 6, ProtoTarget=target)

    def pending_reply(self):  # pendingReplyToARP(), with `free` pendingResponses
        return len(self.pending) >= self.free

    def recv(self, i, ahdr):  # arp.go:134-166; returns the code
        if ahdr.HardwareLength != 6 or ahdr.ProtoLength != 4 or ahdr.HardwareType != 1 or ahdr.ProtoType != 0x0800:
            return UNSUPPORTED, NONE
        if ahdr.Operation == 1:
            if ahdr.ProtoTarget != self.ip:
                return IGNORED, NONE  # not for us
            self.seen.append(i)
            if self.pending_reply():
                return FULL, NONE  # ARP reply pending
            ahdr.HardwareTarget, ahdr.ProtoTarget = ahdr.HardwareSender, ahdr.ProtoSender
            ahdr.HardwareSender, ahdr.ProtoSender = self.mac, self.ip
            ahdr.Operation = 2
            self.pending.append((i, ahdr))
            return ANSWERED, len(self.pending) - 1
        if ahdr.Operation == 2:
            if ahdr.ProtoTarget != self.ip:
                return IGNORED, NONE  # not meant for us
            for q, r in self.results.items():
                # a result that is done keeps the reply's header, whose ProtoSender is the query's target
                target = r.ProtoSender if r.Operation == 2 else r.ProtoTarget
                if target != ahdr.ProtoSender:
                    continue  # does not correspond to this request
                if r.Operation == 1:
                    return IGNORED, NONE  # the request has not left yet: result.Operation != arpOpWait
                self.counts[q] = self.counts.get(q, 0) + 1
                if r.Operation != OP_WAIT:
                    return STALE, q  # result already received
                self.results[q] = ahdr
                self.won[q] = i
                return RESOLVED, q
            return IGNORED, NONE
        return UNSUPPORTED, NONE

    def recv_eth(self, i, frame):  # portstack.go:184-197 for an ARP frame of at least 42 bytes
        dst = bytes(frame[0:6])
        hears = dst == BROADCAST or dst == self.mac  # :185
        if self.faithful and not hears:
            return IGNORED, NONE  # `return nil // Ignore packet, is not for us.`
        ahdr = decode_arp(frame[14:42])  # :195
        code, of = self.recv(i, ahdr) if hears else self.recv_unheard(ahdr)
        return code, of

    def recv_unheard(self, ahdr):
        """Difference (b): the support check of a frame this host does not hear."""
        supported = (ahdr.HardwareLength == 6 and ahdr.ProtoLength == 4 and ahdr.HardwareType == 1 and ahdr.ProtoType == 0x0800 and
                     ahdr.Operation in (1, 2))
        return (IGNORED if supported else UNSUPPORTED), NONE

    def handle(self, q=None):  # arp.go:98-132: one frame per call, the request of query q or the next reply
        if q is not None:
            r = self.results[q]
            assert r.Operation == 1
            frame = BROADCAST + self.mac + b"\x08\x06" + r.put()
            r.Operation = OP_WAIT
            return frame
        i, p = self.pending.pop(0)
        return p.HardwareTarget + self.mac + b"\x08\x06" + p.put()


def finish(frame: bytes, arp_flags: int) -> bytes:
    """What the call adds to the 42 bytes `handle` emits: the zero fill and the FCS."""
    if arp_flags & PAD:
        frame += b"\0" * 18
    if arp_flags & FCS_APPEND:
        frame += zlib.crc32(frame).to_bytes(4, "little")
    return frame


def recv_eth_model(frames, hosts, queries, n_reply_slots, arp_flags=0, frames0=None, out0=None, st0=None, mtu=0, fcs=False,
                   faithful=False):
    """expected()'s tuple from the transliteration (and, with `faithful`, the clients beside it). With `fcs` a
    frame whose FCS is wrong never reaches RecvEth."""
    hosts, queries = np.atleast_1d(hosts), np.atleast_1d(queries)
    clients = [ModelClient(k, row, faithful) for k, row in enumerate(hosts)]
    ghost = ModelClient(NONE, host_row(0, b"\0" * 6, free=0)[0], False)  # a wire without a host: nobody hears, nobody matches
    res = Results(len(frames), hosts, queries, n_reply_slots, frames0, out0, st0)
    waiting = []
    for k, q in enumerate(queries):
        c = clients[int(q["host"])]
        c.begin_resolve(k, bytes(q["target"]))
        if not int(q["flags"]) & SEND_REQUEST:
            if k in c.results:
                c.handle(k)  # the request left in an earlier call: the result waits
            waiting.append(k)
    for i, f in enumerate(frames):
        if fcs:
            if pyref.frame_digest_fcs(f, mtu)[3] == pyref.FS_ERR_FCS:
                continue
            f = f[:-4]
        if len(f) < 34 or (mtu and len(f) > mtu):  # :167-172
            continue
        if int.from_bytes(f[12:14], "big") != 0x0806 or len(f) < 42:  # :187-194
            continue
        code, of = IGNORED, NONE
        for c in clients or [ghost]:
            got, at = (ghost.recv_unheard(decode_arp(f[14:42])) if c is ghost else c.recv_eth(i, f))
            if got in (ANSWERED, FULL, RESOLVED, STALE):
                code, of = got, (int(hosts[c.index]["slot0"]) + at if got == ANSWERED else at)
                break
            if got == UNSUPPORTED:
                code = UNSUPPORTED
        res.code[i], res.of[i] = code, of
    for c, o in zip(clients, res.hosts_out):
        row = hosts[c.index]
        o["n_requests"], o["n_answered"] = len(c.seen), len(c.pending)
        o["first"] = c.seen[0] if c.seen else NONE
        o["free"] = int(row["free"]) - len(c.pending)
        for r in range(len(c.pending)):
            res.put(int(row["slot0"]) + r, finish(c.handle(), arp_flags), arp_flags, mtu)
    for k, q in enumerate(queries):
        c, o = clients[int(q["host"])], res.queries_out[k]
        o["frame"] = NONE
        r = c.results.get(k)
        if r is None:  # (faithful only: a later BeginResolve replaced it)
            o["state"] = Q_WAIT
            continue
        if r.Operation == 1:
            res.put(n_reply_slots + k, finish(c.handle(k), arp_flags), arp_flags, mtu)
            o["state"] = Q_SENT
        elif r.Operation == 2:
            o["state"], o["frame"] = Q_DONE, c.won[k]
            o["mac"] = np.frombuffer(r.HardwareSender, dtype=np.uint8)
        else:
            o["state"] = Q_WAIT
        o["n_replies"] = c.counts.get(k, 0)
    return (res.tuple(), clients) if faithful else res.tuple()


def same(a, b) -> list:
    """The names of the arrays in which two result tuples differ."""
    names = ("hosts_out", "queries_out", "arp_frames", "arp_out", "arp_status", "arp_code", "arp_of")
    return [n for n, x, y in zip(names, a, b) if np.asarray(x).tobytes() != np.asarray(y).tobytes()]
