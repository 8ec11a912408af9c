"""The UDP call's contract (include/framesum_udp.h) stated twice, with code the kernels do not share.

expected(): from the header's rules, in Python integers: the match by destination with the wildcard as
second choice, the rank in batch order, admission by `free`, the cell header and the truncated copy.

recv_eth_model(): a frame-by-frame transliteration of the UDP branch of PortStack.RecvEth
(stacks/portstack.go:222-281): the gates (oracle/pyref.py's recv_eth, which restates :163-245), findPort over
the stack's open UDP ports, the copy of the headers and of the payload into the packet buffer with Go's
`copy` truncation (:262-270), UDPPacket.Payload()'s numbers (port_udp.go:82-89), and port.ihandler.recv(pkt)
driving one model queue per port. A stack is a PortStack with one address (0.0.0.0: `ps.ip == [4]byte{}`,
:209, takes every destination); a frame goes to the stack that has its destination address if that stack
has the port open, else to the address-less stack. The two statements differ only in the stated difference:
the reference's handler holds ONE pending packet, the model queue `n_cells`; with n_cells = free = 1 they
are the same thing, which tests/test_udp_host.py reaches.

Verdicts are an input (`status`): the CPU oracle's in the GPU tests, pyref's in the CPU tests.
"""
import numpy as np

from oracle import pyref

NONE, FULL = 0xFFFFFFFF, 0xFFFFFFFE
HEADER = 32

PORT_DTYPE = np.dtype([("local", "u1", (6,)), ("reserved", "u1", (2,)), ("n_cells", "<u4"), ("cell_size", "<u4"),
                       ("cells_off", "<u8"), ("wcell", "<u4"), ("free", "<u4")])
CELL_DTYPE = np.dtype([("frame", "<u4"), ("len", "<u2"), ("stored", "<u2"), ("udp_length", "<u2"), ("src_port", "<u2"),
                       ("src_ip", "u1", (4,)), ("dst_ip", "u1", (4,)), ("src_mac", "u1", (6,)), ("dst_mac", "u1", (6,))])
PORT_OUT_DTYPE = np.dtype([("wcell", "<u4"), ("free", "<u4"), ("n_matched", "<u4"), ("n_admitted", "<u4"),
                           ("n_truncated", "<u4"), ("first", "<u4"), ("bytes", "<u8")])


# ---- frames ------------------------------------------------------------------------------------------------
def ip4(a) -> bytes:
    if isinstance(a, str):
        return bytes(int(x) for x in a.split("."))
    if isinstance(a, int):
        return a.to_bytes(4, "big")
    return bytes(a)


def udp_frame(src_ip, dst_ip, sport, dport, payload=b"", src_mac=b"\x02\x00\x00\x00\x00\x01", dst_mac=b"\x02\x00\x00\x00\x00\x02",
              ip_options=b"", udp_length=None, bad_csum=False, proto=17, pad=b"", accepted=True) -> bytes:
    """An Ethernet / IPv4 / UDP frame whose checksums RecvEth accepts (pyref.fill_frame writes them).
    `udp_length`: the UDP Length field when it shall disagree with the IP length. `proto` 6: a TCP frame (a
    bare ACK carrying `payload`) to the same addresses and ports. `pad`: bytes behind TotalLength. `accepted`: whether RecvEth's verdict for it is OK."""
    assert len(ip_options) % 4 == 0 and len(ip_options) <= 40
    ihl = 5 + len(ip_options) // 4
    if proto == 17:
        ulen = 8 + len(payload) if udp_length is None else udp_length
        l4 = sport.to_bytes(2, "big") + dport.to_bytes(2, "big") + ulen.to_bytes(2, "big") + b"\0\0" + bytes(payload)
    else:
        l4 = (sport.to_bytes(2, "big") + dport.to_bytes(2, "big") + (1000).to_bytes(4, "big") + (2000).to_bytes(4, "big") +
              bytes([0x50, 0x10]) + (4096).to_bytes(2, "big") + b"\0\0\0\0" + bytes(payload))
    total = 4 * ihl + len(l4)
    ip = (bytes([0x40 | ihl, 0]) + total.to_bytes(2, "big") + b"\x12\x34\x40\x00" + bytes([64, proto]) + b"\0\0" + ip4(src_ip) +
          ip4(dst_ip) + bytes(ip_options))
    f, dig = pyref.fill_frame(bytes(dst_mac) + bytes(src_mac) + b"\x08\x00" + ip + l4 + bytes(pad))
    assert (dig[3] == pyref.FS_OK) == accepted, dig
    if bad_csum:
        at = 14 + 4 * ihl + (6 if proto == 17 else 16)
        f = f[:at] + bytes([f[at] ^ 0x01]) + f[at + 1:]
    return f


def port_row(local_ip, local_port, n_cells, cell_size, cells_off=0, wcell=0, free=None):
    row = np.zeros(1, dtype=PORT_DTYPE)
    row["local"][0] = np.frombuffer(ip4(local_ip) + int(local_port).to_bytes(2, "big"), dtype=np.uint8)
    row["n_cells"], row["cell_size"], row["cells_off"], row["wcell"] = n_cells, cell_size, cells_off, wcell
    row["free"] = n_cells if free is None else free
    return row


def lay_out(rows, lead=0, gap=0):
    """The rows as one PORT_DTYPE array with their queues behind each other from `lead` on, `gap` bytes
    (multiples of 8) between them; returns (ports, cells_bytes)."""
    ports = np.concatenate(rows) if len(rows) else np.zeros(0, dtype=PORT_DTYPE)
    at = lead
    for p in ports:
        p["cells_off"] = at
        at += int(p["n_cells"]) * int(p["cell_size"]) + gap
    return ports, at + 8


def verdicts(frames, mtu=0, fcs=False) -> np.ndarray:
    return np.array([(pyref.frame_digest_fcs(f, mtu) if fcs else pyref.frame_digest(f, mtu))[3] for f in frames], dtype=np.uint8)


# ---- statement 1: the header's rules ----------------------------------------------------------------------
def local_table(ports) -> dict:
    """`local` (6 bytes) -> the port's index."""
    return {bytes(row["local"]): p for p, row in reversed(list(enumerate(ports)))}


def match(frame: bytes, verdict: int, ports, table=None) -> int:
    if verdict != 0 or frame[23] != 17:
        return NONE
    table = local_table(ports) if table is None else table
    l4 = 14 + 4 * (frame[14] & 15)
    dst, port = bytes(frame[30:34]), bytes(frame[l4 + 2 : l4 + 4])
    exact = table.get(dst + port)
    return table.get(b"\0\0\0\0" + port, NONE) if exact is None else exact


def cell_bytes(frame: bytes, index: int, cell_size: int) -> bytes:
    """A cell's written bytes: the header, then `stored` payload bytes."""
    ihl4 = 4 * (frame[14] & 15)
    l4 = 14 + ihl4
    ln = int.from_bytes(frame[16:18], "big") - ihl4 - 8
    stored = min(ln, cell_size - HEADER)
    h = np.zeros(1, dtype=CELL_DTYPE)
    h["frame"], h["len"], h["stored"] = index, ln, stored
    h["udp_length"], h["src_port"] = int.from_bytes(frame[l4 + 4 : l4 + 6], "big"), int.from_bytes(frame[l4 : l4 + 2], "big")
    for name, at, k in (("src_ip", 26, 4), ("dst_ip", 30, 4), ("src_mac", 6, 6), ("dst_mac", 0, 6)):
        h[name][0] = np.frombuffer(bytes(frame[at : at + k]), dtype=np.uint8)
    return h.tobytes() + bytes(frame[l4 + 8 : l4 + 8 + stored])


def expected(frames, status, ports, cells0, fcs=False):
    """(ports_out, port_of, cell_of, cells) of one call over `frames` (a list of bytes, the FCS still on them
    when `fcs`) with verdicts `status`, the PORT_DTYPE rows `ports` and the prefilled `cells0`."""
    n = len(frames)
    ports = np.atleast_1d(ports)
    cells = np.array(cells0, dtype=np.uint8, copy=True)
    port_of = np.full(n, NONE, dtype=np.uint32)
    cell_of = np.full(n, NONE, dtype=np.uint32)
    out = np.zeros(len(ports), dtype=PORT_OUT_DTYPE)
    out["wcell"], out["free"], out["first"] = ports["wcell"], ports["free"], NONE
    table = local_table(ports)
    for i, f in enumerate(frames):
        f = f[:-4] if fcs and len(f) >= 4 else f
        p = match(f, int(status[i]), ports, table)
        if p == NONE:
            continue
        port_of[i] = p
        o, pt = out[p], ports[p]
        r = int(o["n_matched"])
        if r == 0:
            o["first"] = i
        o["n_matched"] += 1
        if r >= int(pt["free"]):
            cell_of[i] = FULL
            continue
        c = (int(pt["wcell"]) + r) % int(pt["n_cells"])
        cell_of[i] = c
        b = cell_bytes(f, i, int(pt["cell_size"]))
        at = int(pt["cells_off"]) + c * int(pt["cell_size"])
        cells[at : at + len(b)] = np.frombuffer(b, dtype=np.uint8)
        stored = len(b) - HEADER
        o["n_admitted"] += 1
        o["bytes"] += stored
        o["n_truncated"] += int(stored < int.from_bytes(b[4:6], "little"))
        o["wcell"] = (int(pt["wcell"]) + int(o["n_admitted"])) % int(pt["n_cells"])
        o["free"] = int(pt["free"]) - int(o["n_admitted"])
    return out, port_of, cell_of, cells


# ---- statement 2: RecvEth's UDP branch, frame by frame ------------------------------------------------------
class ModelQueue:
    """What stands for port.ihandler: it takes packets while it has room. The reference's handler has room
    for one (the stated difference); this one for `free` of its n_cells."""

    def __init__(self, index, row):
        self.index, self.port = index, int.from_bytes(bytes(row["local"][4:6]), "big")
        self.n_cells, self.cell_size = int(row["n_cells"]), int(row["cell_size"])
        self.wcell, self.free, self.off = int(row["wcell"]), int(row["free"]), int(row["cells_off"])
        self.taken = []  # (frame index, cell, packet) in arrival order
        self.dropped = []

    def recv(self, i, pkt) -> bool:
        if self.free == 0:
            self.dropped.append(i)
            return False
        self.taken.append((i, self.wcell, pkt))
        self.wcell = (self.wcell + 1) % self.n_cells
        self.free -= 1
        return True


class ModelStack:
    """A PortStack: its address (b"\\0\\0\\0\\0": none set, :209) and its open UDP ports."""

    def __init__(self, ip):
        self.ip, self.ports_udp = ip, []

    def find_port(self, number):  # findPort(ps.portsUDP, uhdr.DestinationPort): the first open port with that number
        for q in self.ports_udp:
            if q.port == number:
                return q
        return None


def go_copy(dst_len: int, src: bytes) -> bytes:
    """Go's copy(dst, src): min(len(dst), len(src)) bytes."""
    return bytes(src[:dst_len])


def recv_eth_udp(stack: ModelStack, i: int, frame: bytes, mtu: int = 0):
    """One frame through RecvEth's UDP branch on `stack`: the queue that took it or refused it and the
    packet, or (None, None) for a frame the branch does not deliver."""
    verdict, _, _ = pyref.recv_eth(frame, mtu)  # :163-245, the checksum compare included
    if verdict != pyref.FS_OK or frame[23] != 17:
        return None, None
    ihdr, ip_off = pyref.decode_ipv4_header(frame[14:])
    if stack.ip != b"\0\0\0\0" and bytes(frame[30:34]) != stack.ip:  # :209
        return None, None
    offset, end = 14 + ip_off, 14 + ihdr.total_length
    payload = frame[offset:end]  # :217
    uhdr = pyref.decode_udp_header(payload)  # :223
    q = stack.find_port(uhdr.destination_port)  # :246
    if q is None:
        return None, None
    room = q.cell_size - HEADER  # len(pkt.payload)
    pkt = {"eth": bytes(frame[:14]), "ip": ihdr, "udp": uhdr, "ip_len": ihdr.total_length - ip_off - 8,
           "payload": go_copy(room, payload[8:])}  # :262-270
    return q, pkt


def recv_eth_model(frames, ports, cells0, mtu=0, fcs=False):
    """expected()'s tuple from the transliteration. With `fcs` a frame whose FCS is wrong never reaches
    RecvEth (pyref.frame_digest_fcs)."""
    ports = np.atleast_1d(ports)
    stacks = {}
    queues = []
    for p, row in enumerate(ports):
        q = ModelQueue(p, row)
        queues.append(q)
        stacks.setdefault(bytes(row["local"][:4]), ModelStack(bytes(row["local"][:4]))).ports_udp.append(q)
    n = len(frames)
    port_of = np.full(n, NONE, dtype=np.uint32)
    cell_of = np.full(n, NONE, dtype=np.uint32)
    for i, f in enumerate(frames):
        if fcs:
            if pyref.frame_digest_fcs(f, mtu)[3] == pyref.FS_ERR_FCS:
                continue
            f = f[:-4]
        q = pkt = None
        if len(f) >= 34:
            own = stacks.get(bytes(f[30:34]))
            if own is not None and bytes(f[30:34]) != b"\0\0\0\0":
                q, pkt = recv_eth_udp(own, i, f, mtu)
            if q is None and b"\0\0\0\0" in stacks:
                q, pkt = recv_eth_udp(stacks[b"\0\0\0\0"], i, f, mtu)
        if q is None:
            continue
        port_of[i] = q.index
        at = q.wcell
        cell_of[i] = at if q.recv(i, pkt) else FULL
    cells = np.array(cells0, dtype=np.uint8, copy=True)
    out = np.zeros(len(ports), dtype=PORT_OUT_DTYPE)
    for q, o in zip(queues, out):
        o["wcell"], o["free"] = q.wcell, q.free
        o["n_matched"], o["n_admitted"] = len(q.taken) + len(q.dropped), len(q.taken)
        o["first"] = min([t[0] for t in q.taken] + q.dropped, default=NONE)
        for i, c, pkt in q.taken:
            h = np.zeros(1, dtype=CELL_DTYPE)
            h["frame"], h["len"], h["stored"] = i, pkt["ip_len"], len(pkt["payload"])
            h["udp_length"], h["src_port"] = pkt["udp"].length, pkt["udp"].source_port
            h["src_ip"][0] = np.frombuffer(bytes(frames[i][26:30]), dtype=np.uint8)
            h["dst_ip"][0] = np.frombuffer(bytes(frames[i][30:34]), dtype=np.uint8)
            h["src_mac"][0] = np.frombuffer(pkt["eth"][6:12], dtype=np.uint8)
            h["dst_mac"][0] = np.frombuffer(pkt["eth"][0:6], dtype=np.uint8)
            b = h.tobytes() + pkt["payload"]
            at = q.off + c * q.cell_size
            cells[at : at + len(b)] = np.frombuffer(b, dtype=np.uint8)
            o["bytes"] += len(pkt["payload"])
            o["n_truncated"] += int(len(pkt["payload"]) < pkt["ip_len"])  # Payload(): uLen > len(pkt.payload)
    return out, port_of, cell_of, cells
