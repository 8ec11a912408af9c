"""The batches of tests/test_gpu_udp.py. Every builder returns a Case: the frames, the port list with its
queues laid out, the call's flags, and `reaches(want)`, which asserts on tests/udp_ref.py's expected tuple
(ports_out, port_of, cell_of, cells) that the batch reaches what its name says.
tests/test_udp_case_builders.py runs every `reaches` on the CPU."""
import functools

import numpy as np

import udp_ref as ref

US, OTHER, BCAST = "10.0.0.1", "10.0.0.2", "255.255.255.255"
RANKS = (0, 1, 62, 63, 64, 65, 255, 256, 257)


class Case:
    def __init__(self, frames, ports, cells_bytes, reaches, flags=0, mtu=0, lists=None, batch=None, status=None):
        self.frames, self.ports, self.cells_bytes, self.reaches = frames, ports, cells_bytes, reaches
        self.flags, self.mtu = flags, mtu
        self.lists = lists    # a tests/connect_cases.py case whose lists the call takes beside the ports
        self.batch = batch    # (buf, off, ln) where the frames lie in a buffer of the builder's own
        self.status = status  # the frames' verdicts where the builder knows them (the CPU oracle filled them in)


def expected(case):
    """The reference's tuple for the case over zeroed cells, with pyref's verdicts unless the case has its own."""
    status = ref.verdicts(case.frames, case.mtu, bool(case.flags & 1)) if case.status is None else case.status
    return ref.expected(case.frames, status, case.ports, np.zeros(case.cells_bytes, dtype=np.uint8), bool(case.flags & 1))


def source(k):
    return f"172.{16 + (k >> 16) % 16}.{(k >> 8) & 255}.{k & 255}"


@functools.lru_cache(maxsize=None)
def noisy(n_matched=258, dport=67):
    """`n_matched` datagrams to US:dport from changing sources, with a frame that takes no rank after each: to
    the next port, TCP to the same port, a bad checksum, to another address, in turn."""
    frames = []
    for r in range(n_matched):
        frames.append(ref.udp_frame(source(r), US, 1024 + r, dport, bytes([r & 255]) * (r % 23)))
        frames.append((ref.udp_frame(source(r), US, 1024 + r, dport + 1, b"elsewhere"),
                       ref.udp_frame(source(r), US, 1024 + r, dport, b"tcp", proto=6),
                       ref.udp_frame(source(r), US, 1024 + r, dport, b"damaged", bad_csum=True),
                       ref.udp_frame(source(r), OTHER, 1024 + r, dport, b"not ours"))[r % 4])
    return tuple(frames)


# ---- rank -------------------------------------------------------------------------------------------------------

def rank(free):
    """Ranks 0 .. 257 of one port (RANKS among them) with frames that take no rank between; `free` cells."""
    ports, cells_bytes = ref.lay_out([ref.port_row(US, 67, 300, 56, wcell=7, free=free)], lead=8)

    def reaches(want):
        assert want[0]["n_matched"][0] == 258 and want[0]["n_admitted"][0] == min(free, 258)
        assert list(want[2][::2][list(RANKS)]) == [7 + r if r < free else ref.FULL for r in RANKS]
        assert (want[1][1::2] == ref.NONE).all() and (want[2][1::2] == ref.NONE).all()
        assert want[0]["first"][0] == 0 and want[0]["free"][0] == max(0, free - 258)
    return Case(list(noisy()), ports, cells_bytes, reaches)


def wrap(n_cells):
    """wcell = n_cells - 1: the second datagram goes to cell 0, or finds the one-cell queue full."""
    ports, cells_bytes = ref.lay_out([ref.port_row(US, 67, n_cells, 64, wcell=n_cells - 1)])

    def reaches(want):
        assert list(want[2][:10:2]) == ([0] + [ref.FULL] * 4 if n_cells == 1 else [4, 0, 1, 2, 3])
        assert want[0]["wcell"][0] == (0 if n_cells == 1 else 4) and want[0]["free"][0] == 0
    return Case(list(noisy()[:16]), ports, cells_bytes, reaches)


def three_ports():
    """Three ports (one of them the wildcard, taking a broadcast and a unicast destination) whose frames interleave."""
    rows = [ref.port_row(US, 67, 40, 48, wcell=39), ref.port_row("0.0.0.0", 68, 70, 40, free=50), ref.port_row(OTHER, 67, 64, 64)]
    ports, cells_bytes = ref.lay_out(rows, lead=16, gap=24)
    which = np.random.default_rng(2).integers(0, 4, 200)  # 46, 53, 52 and 49 frames
    frames = []
    for k in range(200):
        dst, dport = ((US, 67), (BCAST, 68), (OTHER, 67), (US, 68))[which[k]]
        frames.append(ref.udp_frame(source(k), dst, 2000 + k, dport, bytes([k]) * (k % 31)))

    def reaches(want):
        assert list(want[0]["n_matched"]) == [46, 102, 52] and list(want[0]["n_admitted"]) == [40, 50, 52]
        assert (want[0]["n_truncated"][:2] > 0).all()  # (payloads of up to 30 bytes into rooms of 16, 8 and 32)
        changes = np.count_nonzero(np.diff(want[1].astype(np.int64)))
        assert changes > 100  # the ports' frames interleave
    return Case(frames, ports, cells_bytes, reaches)


# ---- copy and truncation ------------------------------------------------------------------------------------------

def payload_lengths(cell_size):
    """Payloads of 0 .. 40, 63, 64, 65 and 1,472 bytes. Cells of 1,504 bytes hold each whole (the 16-lane copy);
    cells of 96 bytes are the largest the 4-lane copy serves and cut the last two to four whole pieces."""
    frames = [ref.udp_frame(source(k), US, 3000 + k, 67, bytes((k * 5 + j) & 255 for j in range(k))) for k in list(range(41)) + [63, 64, 65, 1472]]
    ports, cells_bytes = ref.lay_out([ref.port_row(US, 67, 64, cell_size)])

    def reaches(want):
        assert want[0]["n_admitted"][0] == 45 and want[0]["n_truncated"][0] == (0 if cell_size == 1504 else 2)
        assert want[0]["bytes"][0] == sum(range(41)) + 63 + 64 + (65 + 1472 if cell_size == 1504 else 128)
    return Case(frames, ports, cells_bytes, reaches)


def truncation(cell_size):
    """len = cell_size - 32 - 1 / 0 / + 1 (and + 7), across a wrap."""
    room = cell_size - 32
    frames = [ref.udp_frame(source(k), US, 9, 67, bytes((k + j) & 255 for j in range(room + d))) for k, d in enumerate((-1, 0, 1, 7, 0, -1))]
    ports, cells_bytes = ref.lay_out([ref.port_row(US, 67, 8, cell_size, wcell=6)])

    def reaches(want):
        assert want[0]["n_truncated"][0] == 2 and want[0]["bytes"][0] == 6 * room - 2 and list(want[2]) == [6, 7, 0, 1, 2, 3]
        heads = [want[3][c * cell_size : c * cell_size + 32].view(ref.CELL_DTYPE)[0] for c in (6, 7, 0, 1)]
        assert [(int(h["len"]), int(h["stored"])) for h in heads] == [(room - 1, room - 1), (room, room), (room + 1, room), (room + 7, room)]
    return Case(frames, ports, cells_bytes, reaches)


def largest():
    """A 65,507-byte datagram with mtu 0: its frame is 65,549 bytes, and the reference's `end` is a uint16
    (portstack.go:202), so its verdict is errBadIPTotalLenOrIHL and no cell takes it. The largest datagram the
    verdict accepts has 65,493 bytes (14 + TotalLength = 65,535); it fills the largest cell but 43 bytes."""
    data = np.random.default_rng(3).integers(0, 256, 65507, dtype=np.uint8).tobytes()
    refused, big = ref.udp_frame(OTHER, US, 9, 67, data, accepted=False), ref.udp_frame(OTHER, US, 9, 67, data[:65493])
    frames = [ref.udp_frame(OTHER, US, 9, 67, b"before"), refused, ref.udp_frame(OTHER, US, 9, 68, b"after"), big, big]
    ports, cells_bytes = ref.lay_out([ref.port_row(US, 67, 2, 65568, wcell=1), ref.port_row(US, 68, 2, 40)], gap=8)

    def reaches(want):
        assert len(refused) == 65549 and list(want[2]) == [1, ref.NONE, 0, 0, ref.FULL] and want[0]["bytes"][0] == 6 + 65493
    return Case(frames, ports, cells_bytes, reaches, mtu=0)


# ---- headers and key matching -------------------------------------------------------------------------------------

def header_frames():
    """Per IHL 5, 6 and 15: a unicast and a broadcast datagram, UDP Length above and below the IP length,
    padding behind TotalLength, and a TCP frame to the same address and port."""
    frames = []
    for k, opts in enumerate((b"", b"\x01\x01\x01\x00", b"\x01" * 40)):
        frames.append(ref.udp_frame(source(k), US, 4000 + k, 67, b"ihl %d" % k, ip_options=opts))
        frames.append(ref.udp_frame(source(k), BCAST, 4000 + k, 67, b"broadcast", ip_options=opts))
        frames.append(ref.udp_frame(source(k), US, 4000 + k, 67, b"length above", ip_options=opts, udp_length=60))
        frames.append(ref.udp_frame(source(k), US, 4000 + k, 67, b"length below", ip_options=opts, udp_length=9))
        frames.append(ref.udp_frame(source(k), US, 4000 + k, 67, b"padded", ip_options=opts, pad=b"\xEE" * 11))
        frames.append(ref.udp_frame(source(k), US, 4000 + k, 67, b"tcp", ip_options=opts, proto=6))
    return frames


def headers(listed):
    """header_frames() to an exact port, a wildcard port, or both for one port number."""
    rows = ([ref.port_row(US, 67, 32, 64)] if listed != "wildcard" else []) + ([ref.port_row("0.0.0.0", 67, 32, 48)] if listed != "exact" else [])
    ports, cells_bytes = ref.lay_out(rows, lead=8)
    frames = header_frames()

    def reaches(want):
        assert [f[14] & 15 for f in frames[::6]] == [5, 6, 15]
        unicast, bcast = want[1][0::6], want[1][1::6]
        assert list(unicast) == [0] * 3 and list(bcast) == [{"exact": ref.NONE, "wildcard": 0, "both": 1}[listed]] * 3
        assert (want[1][5::6] == ref.NONE).all() and (want[1][2::6] == 0).all() and (want[1][3::6] == 0).all()
        at = int(ports[0]["cells_off"]) + int(want[2][2]) * int(ports[0]["cell_size"])  # frame 2's cell: UDP Length above
        h = want[3][at : at + 32].view(ref.CELL_DTYPE)[0]
        assert (int(h["frame"]), int(h["len"]), int(h["udp_length"])) == (2, 12, 60)
    return Case(frames, ports, cells_bytes, reaches)


def with_fcs():
    """header_frames() with their FCS (FS_RX_FCS), one of them with a damaged FCS."""
    from oracle import pyref

    wire = [pyref.fill_frame(f, 0, pyref.FCS_APPEND)[0] for f in header_frames()]
    wire[6] = wire[6][:-2] + bytes([wire[6][-2] ^ 0x10]) + wire[6][-1:]
    ports, cells_bytes = ref.lay_out([ref.port_row(US, 67, 32, 48)])

    def reaches(want):
        assert want[1][6] == ref.NONE and want[1][0] == 0 and want[0]["n_matched"][0] == 11
        at = int(want[2][4]) * 48  # frame 4 is padded: the pad and the FCS are no payload
        pad = want[3][at : at + 32].view(ref.CELL_DTYPE)[0]
        assert (int(pad["frame"]), int(pad["len"])) == (4, 6)
    return Case(wire, ports, cells_bytes, reaches, flags=1)


def near_keys():
    """Frames whose destination differs from the port's in one bit of the address or of the port number."""
    local = ref.ip4(US) + (67).to_bytes(2, "big")
    frames = [ref.udp_frame(OTHER, US, 9, 67, b"the port's own")]
    for bit in range(48):
        near = bytearray(local)
        near[bit // 8] ^= 1 << (bit % 8)
        frames.append(ref.udp_frame(OTHER, bytes(near[:4]), 9, int.from_bytes(near[4:6], "big"), b"near %d" % bit))
    frames.append(frames[0])
    ports, cells_bytes = ref.lay_out([ref.port_row(US, 67, 4, 48)])

    def reaches(want):
        assert len(frames) == 50 and want[0]["n_matched"][0] == 2 and (want[1][1:-1] == ref.NONE).all()
    return Case(frames, ports, cells_bytes, reaches)


# ---- launch shapes ------------------------------------------------------------------------------------------------

def many_ports(n_ports, cell_size=40, n_cells=2):
    rows = [ref.port_row((10 << 24) | (1 + p // 251), 1 + p % 65535, n_cells, cell_size) for p in range(n_ports)]
    return ref.lay_out(rows)


@functools.lru_cache(maxsize=None)
def table_load():
    """300 ports and 700 frames: frame k goes to port 37 k mod 300, every fifth to the port number above it, which
    is the next port's; every fifth port so gets none, and ports with three frames find their two cells full."""
    ports, cells_bytes = many_ports(300)
    frames = [ref.udp_frame(source(k), bytes(ports[(k * 37) % 300]["local"][:4]), 9,
                            int.from_bytes(bytes(ports[(k * 37) % 300]["local"][4:]), "big") + (k % 5 == 4), bytes([k & 255]) * (k % 9))
              for k in range(700)]

    def reaches(want):
        assert (want[0]["n_matched"] > 0).sum() == 240 and (want[2] == ref.FULL).any() and (want[1] != ref.NONE).all()
    return Case(frames, ports, cells_bytes, reaches)


def two_queues():
    """noisy() to two ports (the next port's frames are the noise of the first), one wrapping with 200 free cells."""
    ports, cells_bytes = ref.lay_out([ref.port_row(US, 67, 300, 56, wcell=299, free=200), ref.port_row(US, 68, 200, 40)])

    def reaches(want):
        assert list(want[0]["n_matched"]) == [258, 65] and list(want[0]["n_admitted"]) == [200, 65] and want[0]["wcell"][0] == 199
    return Case(list(noisy()), ports, cells_bytes, reaches)


def columns():
    """300 frames of noisy() to an exact and a wildcard port, for every engine column."""
    ports, cells_bytes = ref.lay_out([ref.port_row(US, 67, 100, 48, wcell=99), ref.port_row("0.0.0.0", 68, 100, 40)])

    def reaches(want):
        assert list(want[0]["n_matched"]) == [150, 38] and list(want[0]["n_admitted"]) == [100, 38]
    return Case(list(noisy()[:300]), ports, cells_bytes, reaches)


# ---- mixed and large batches --------------------------------------------------------------------------------------

def mixed():
    """tests/connect_cases.py's three_lists() (sockets, a listener, closers, openers) with 60 datagrams to two
    ports between its frames."""
    import connect_cases

    case = connect_cases.three_lists()
    frames = list(case.frames)
    for k in range(60):
        frames.insert(min(len(frames), 3 * k + 1), ref.udp_frame(source(k), US, 5000 + k, 67 + k % 2, b"between the flows %d" % k))
    ports, cells_bytes = ref.lay_out([ref.port_row(US, 67, 16, 64), ref.port_row("0.0.0.0", 68, 64, 48)], lead=8)

    def reaches(want):
        assert list(want[0]["n_matched"]) == [30, 30] and list(want[0]["n_admitted"]) == [16, 30]
        assert len(case.socks) and len(case.listeners) and len(case.closers) and len(case.openers)
        assert (want[1] == ref.NONE).sum() == len(case.frames)  # the case's own stray datagrams reach no port
    return Case(frames, ports, cells_bytes, reaches, lists=case)


@functools.lru_cache(maxsize=None)
def benchmark_rows():
    from seqs_amd import synth

    return synth.make_frames(65793, 47, 17, np.random.default_rng(65793))


def benchmark(n_ports):
    """The reference's benchmark shape (stacks/benchmark_test.go:12-46) at 65,793 frames, more than 2^16 and no
    multiple of a workgroup's 256: 47-byte UDP frames (5 payload bytes) from random sources. One port with room
    for all (a third of every second frame goes to port 68, which nobody has); 1,000 ports of 2 cells for 65 or
    66 frames each; 65,536 ports of one cell, 257 of which get two frames."""
    from oracle import coracle

    n = 65793
    arr = benchmark_rows().copy()
    ports, cells_bytes = (many_ports(n_ports, 40, 2 if n_ports == 1000 else 1) if n_ports > 1 else
                          ref.lay_out([ref.port_row(US, 67, 65600, 40, wcell=65000)]))
    which = (np.arange(n) * 7919) % max(n_ports, 2)
    if n_ports == 1:
        arr[:, 30:34] = np.frombuffer(ref.ip4(US), dtype=np.uint8)
        arr[:, 36], arr[:, 37] = 0, 67 + (which % 2 == 1) * (np.arange(n) % 3 == 0)
    else:
        arr[:, 30:38][:, [0, 1, 2, 3, 6, 7]] = ports["local"][which % n_ports]
    buf = np.concatenate([arr.reshape(-1), np.zeros(64, np.uint8)])
    off, ln = np.arange(n, dtype=np.uint64) * 47, np.full(n, 47, dtype=np.uint32)
    _, st = coracle.fill_batch(buf, off, ln)
    assert not st.any()
    frames = [buf[47 * i : 47 * i + 47].tobytes() for i in range(n)]

    def reaches(want):
        m = want[0]["n_matched"]
        if n_ports == 1:
            assert 54000 < m[0] < 55000 and want[0]["n_admitted"][0] == m[0] and want[0]["wcell"][0] < 65000  # it wraps
        elif n_ports == 1000:
            assert set(m) == {65, 66} and (want[0]["n_admitted"] == 2).all()
        else:
            assert m.sum() == n and (m == 2).sum() == 257 and (want[2] == ref.FULL).sum() == 257
    return Case(frames, ports, cells_bytes, reaches, batch=(buf, off, ln), status=st)


# ---- calls --------------------------------------------------------------------------------------------------------

def empty_batch():
    """n == 0: every port keeps its state."""
    ports, cells_bytes = ref.lay_out([ref.port_row(US, 67, 4, 48, wcell=3, free=2), ref.port_row(US, 68, 2, 40)])

    def reaches(want):
        assert list(want[0]["wcell"]) == [3, 0] and list(want[0]["free"]) == [2, 2] and (want[0]["first"] == ref.NONE).all()
        assert not want[0]["n_matched"].any() and not want[0]["bytes"].any()
    return Case([], ports, cells_bytes, reaches)


def no_ports(n=40):
    """n_ports == 0: the two fills alone."""
    def reaches(want):
        assert want[0].size == 0 and (want[1] == ref.NONE).all() and (want[2] == ref.NONE).all() and want[1].size == n
    return Case(list(noisy()[:n]), np.zeros(0, dtype=ref.PORT_DTYPE), 8, reaches)


def in_flight(k):
    """The k-th of eight calls in flight: 120 frames of noisy() from 2 k on, a queue of its own size and start."""
    ports, cells_bytes = ref.lay_out([ref.port_row(US, 67, 50 + k, 56, wcell=k)], lead=8 * k)

    def reaches(want):
        assert want[0]["n_matched"][0] == 60 and want[0]["n_admitted"][0] == min(60, 50 + k)
    return Case(list(noisy()[2 * k : 2 * k + 120]), ports, cells_bytes, reaches)


def host_span():
    """The host form's batch: the queues start 4,096 bytes into `cells`, with gaps between them."""
    rows = [ref.port_row(US, 67, 40, 48, wcell=39), ref.port_row("0.0.0.0", 68, 70, 40, free=50)]
    ports, cells_bytes = ref.lay_out(rows, lead=4096, gap=64)
    frames = list(noisy()[:200]) + [ref.udp_frame(source(k), BCAST, 9, 68, bytes([k]) * k) for k in range(60)]

    def reaches(want):
        assert ports["cells_off"].min() == 4096 and list(want[0]["n_admitted"]) == [40, 50] and list(want[0]["n_matched"]) == [100, 85]
        assert not want[3][:4096].any()
    return Case(frames, ports, cells_bytes, reaches)


def rejected_ports():
    """Two good ports whose second queue ends at cells_bytes exactly: (ports, cells_bytes)."""
    ports, cells_bytes = ref.lay_out([ref.port_row(US, 67, 4, 48), ref.port_row(US, 68, 4, 48)])
    return ports, cells_bytes - 8


REJECTIONS = [
    (lambda p: p["reserved"].__setitem__((1, 0), 1), "port 1: reserved must be 0"),
    (lambda p: p["local"].__setitem__((1, slice(4, 6)), 0), "port 1: its local has port 0"),
    (lambda p: p["local"].__setitem__(1, p["local"][0]), "port 1: its local equals an earlier port's"),
    (lambda p: p["cell_size"].__setitem__(1, 44), "port 1: cell_size must be a multiple of 8 from 40 to 65,568"),
    (lambda p: p["cell_size"].__setitem__(1, 32), "port 1: cell_size must be a multiple of 8 from 40 to 65,568"),
    (lambda p: p["cell_size"].__setitem__(1, 65576), "port 1: cell_size must be a multiple of 8 from 40 to 65,568"),
    (lambda p: p["cells_off"].__setitem__(1, p["cells_off"][1] + 4), "port 1: cells_off must be a multiple of 8"),
    (lambda p: p["n_cells"].__setitem__(1, 0), "port 1: n_cells must be from 1 to 2^31"),
    (lambda p: p["n_cells"].__setitem__(1, (1 << 31) + 1), "port 1: n_cells must be from 1 to 2^31"),
    (lambda p: p["wcell"].__setitem__(1, 4), "port 1: wcell must be below n_cells"),
    (lambda p: p["free"].__setitem__(1, 5), "port 1: free must be at most n_cells"),
    (lambda p: p["cells_off"].__setitem__(1, p["cells_off"][1] + 8), "port 1: its queue ends past cells_bytes"),
    (lambda p: p["cells_off"].__setitem__(1, p["cells_off"][1] - 8), "port 1: its queue overlaps another port's"),
]
