"""Frame and payload offsets beyond 4 GiB through every entry point. `offsets`, fs_tx_send.payload_off,
fs_rx_run.payload_off, fs_rx_flow.payload_off / payload_len and the offsets fs_segment_batch writes are
64-bit so that batches larger than 4 GiB work (DESIGN.md's layout table, include/framesum.h); the other
suites keep every batch in the first few hundred MiB of a small tensor, where a dropped high half of an
offset or of an address never shows.

Method: one uninitialised device tensor of 2^32 + 64 MiB bytes per module. A case is built small on the
host with the generators of the other suites, uploaded into the big tensor at a base B between 256
bytes of known noise, and run with offsets + B. The reference (the C oracle, or the Python restatements
of tests/*_ref.py) runs on the small host copy: a digest does not depend on where a frame lies, so
every comparison stays bit for bit. After a call that writes, the window [B - 256, B + size + 256) is
read back and compared whole. Three placements:
  offset   B just below 2^32: the batch straddles OFFSET 2^32 inside a frame (after its first byte,
           inside its IPv4 and its L4 header, mid-payload, on a 64-byte block edge, on its last byte,
           between two frames), and B mod 64 is swept;
  address  B chosen from data_ptr() so that the ABSOLUTE address straddles a multiple of 2^32 at the
           same places (the allocation is longer than 4 GiB, so one such address lies inside it): a
           32-bit add of base and offset shows here even where every offset is below 2^32;
  both     frames alternate between a copy of the batch below 1 MiB and one above 2^32, so every tile
           holds frames of both sides, and the tile's longest frame is high in one run, low in the other.
Every case asserts from its offsets and data_ptr() that it is where it claims to be.

The payloads gathered beyond 4 GiB (fs_coalesce_batch, fs_coalesce_flows_batch) list a handful of
distinct jumbo frames ~66,000 times (frames may overlap, so the frame buffer stays 400 KB); what is
expected comes from the references applied to the distinct frames only and is expanded over the index
list with numpy. test_expansion_equals_the_restatements checks that expansion, without a GPU, against
the sequential restatements on a short list.
"""
import functools
import random

import numpy as np
import pytest

import coalesce_ref as cref
import deliver_cases as dcases
import deliver_ref as dref
import engines
import flows_ref as fref
import framegen
import segment_ref as sref
from oracle import coracle

gpu = pytest.mark.gpu

G = 1 << 32
BIG_BYTES = G + (64 << 20)
MARGIN = 256   # known noise on both sides of a placed batch, compared after every call that writes
FILL = 0x5A    # what bytes that must stay unwritten hold
FCS = 2
PLACEMENTS = ["offset", "address", "both"]
JUMBO = 65481  # the longest TCP payload RecvEth accepts: 14 + TotalLength must not wrap its uint16 `end`
               # (a 65,495-byte payload, TotalLength 65,535, is FS_ERR_BAD_IP_TOTAL_LEN_OR_IHL and carries nothing)


# ---- fixtures ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big():
    """The module's one big device tensor, uninitialised. (A failed allocation fails the tests.)"""
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()  # (torch's runtime first, as in the other GPU suites)
    t = torch.empty(BIG_BYTES, dtype=torch.uint8, device="cuda:0")
    assert t.numel() == BIG_BYTES and t.numel() >= G + (64 << 20) and t.data_ptr() % 4 == 0
    yield t
    del t
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def eng():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", params=engines.VARIANTS, ids=engines.IDS)
def engine(request):
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()
    e = engines.engine_for(request.param)
    yield e, request.param
    e.close()


def dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


# ---- placing a small batch in the big tensor -----------------------------------------------------

class Placed:
    """A small host batch (buf, off, ln), its window (the buffer between two margins of noise) and
    that window's device copy."""

    def __init__(self, buf, off, ln, cuts=(), seed=0):
        noise = np.random.default_rng(900 + seed).integers(0, 256, 2 * MARGIN, dtype=np.uint8)
        self.buf = np.ascontiguousarray(buf, dtype=np.uint8)
        self.off = np.asarray(off).astype(np.int64)
        self.ln = np.asarray(ln).astype(np.int32)
        self.size = int(self.buf.size)
        self.window = np.concatenate([noise[:MARGIN], self.buf, noise[MARGIN:]])
        self.cuts = list(cuts)  # (frame, byte of it) pairs the 2^32 boundary is put on
        self._dev = None

    def put(self, big, base):
        if self._dev is None:
            self._dev = dev(self.window)
        assert MARGIN <= base and base + self.size + MARGIN <= big.numel()
        big[base - MARGIN : base + self.size + MARGIN].copy_(self._dev)

    def fetch(self, big, base):
        return big[base - MARGIN : base + self.size + MARGIN].cpu().numpy()


def frame_cuts(ln, f):
    """Where the boundary falls in frame f: after its first byte, inside the IPv4 header, inside the L4
    header, mid-payload, on a 64-byte block edge (the frame then starts on one), on its last byte, and
    between it and the next frame."""
    L = int(ln[f])
    return [(f, p) for p in (1, 20, 44, L // 2, 128, L - 1, L) if 0 < p <= L]


def placements(case, big, which):
    """(label, bases) per placement of the kind: bases[i] is what frame i's offset is moved by; the
    batch is uploaded at every distinct base."""
    n, ptr = case.off.size, big.data_ptr()
    if which == "both":
        for k, (lo, hi) in enumerate([(MARGIN, G + 4096), (MARGIN + 3, G + 77)]):
            assert lo + int((case.off + case.ln).max()) < 1 << 20, "the low copy lies below 1 MiB"
            for par in (0, 1):
                yield f"low {lo} / high 2^32+{hi - G}, parity {par}", np.where((np.arange(n) + par) % 2 == 0, lo, hi)
        return
    for f, pos in case.cuts:
        at = int(case.off[f]) + pos  # the byte of the batch that lands on the boundary
        if which == "offset":
            base = G - at
        else:  # the multiple of 2^32 inside the allocation that leaves room for the batch on both sides
            x = -(-(ptr + MARGIN + at) // G) * G
            base = x - ptr - at
            assert (ptr + base + at) % G == 0
        assert MARGIN <= base and base + case.size + MARGIN <= big.numel()
        yield f"frame {f} byte {pos} on the boundary (base mod 64 = {base % 64})", np.full(n, base, dtype=np.int64)


def assert_beyond(big, which, off, ln, bases):
    """The case is where it claims to be (a later refactor must not shrink the buffer unnoticed)."""
    o, ptr = off + bases, big.data_ptr()
    assert big.numel() > G and int(o.min()) >= MARGIN and int((o + ln).max()) + MARGIN <= big.numel()
    if which == "offset":
        assert int(o.min()) < G <= int((o + ln).max()) and int(o.max()) >= G - int(ln.max())
    elif which == "address":
        assert (ptr + int(o.min())) >> 32 != (ptr + int((o + ln).max())) >> 32
    else:
        assert int(o.min()) < 1 << 20 and int(o.max()) > G and int((o >= G).sum()) in (o.size // 2, (o.size + 1) // 2)


def put_all(case, big, bases):
    for b in np.unique(bases):
        case.put(big, int(b))


# ---- 1. digest, FCS verify and fill under every kernel -------------------------------------------

def pack(frames, room=0, seed=0):
    """Frames back to back, `room` spare bytes behind each, noise between."""
    ln = np.array([len(f) for f in frames], dtype=np.int32)
    off = np.zeros(ln.size, dtype=np.int64)
    off[1:] = np.cumsum(ln[:-1].astype(np.int64) + room)
    buf = np.random.default_rng(500 + seed).integers(0, 256, int(off[-1]) + int(ln[-1]) + room, dtype=np.uint8)
    for o, f in zip(off, frames):
        buf[int(o) : int(o) + len(f)] = np.frombuffer(bytes(f), dtype=np.uint8)
    return buf, off, ln


@functools.lru_cache(maxsize=None)
def digest_frames():
    """A few hundred frames that take every kernel's own address paths: a tile of a 128-KB frame and 15
    64-byte ones (the segment kernel's chunk walk, the small-frame kernel's long-frame path), the edge
    batch (frames under 4 bytes, every rejection class), lengths on both sides of the mixed kernel's
    768-byte pieces (its mode B and the per-wave frame table), and a second such tile whose long frame
    stands at an odd index. Returns (frames, the frames the 2^32 boundary is put in)."""
    rnd = random.Random(4242)

    def short():
        return framegen.valid_frame(rnd, 6, payload=10) if rnd.random() < 0.5 else framegen.valid_frame(rnd, 17, payload=22)

    def giant(proto):
        hdr = 54 if proto == 6 else 42
        return framegen.valid_frame(rnd, proto, payload=1000, pad=131072 - hdr - 1000)

    frames = [giant(6)] + [short() for _ in range(15)]
    frames += framegen.edge_batch(11, n_random=150)
    long_at = len(frames) + 3 * 3 + 1  # the 3,072-byte frame below
    for k in (1, 2, 3, 4, 5, 12):
        for d in (-1, 0, 1):
            tcp = (k + d) & 1
            frames.append(framegen.valid_frame(rnd, 6 if tcp else 17, payload=768 * k + d - (54 if tcp else 42)))
    while len(frames) % 16:
        frames.append(short())
    giant2_at = len(frames) + 7
    frames += [short() for _ in range(7)] + [giant(17)] + [short() for _ in range(8)]
    assert len(frames[0]) == len(frames[giant2_at]) == 131072 and giant2_at % 2 == 1 and len(frames[long_at]) == 3072
    assert all(len(f) == 64 for f in frames[1:16]) and len(frames) >= 256 and min(len(f) for f in frames) == 0
    mid_at = next(i for i, f in enumerate(frames) if 1000 <= len(f) <= 1500 and f[12:15] == b"\x08\x00\x45" and f[23] == 6)
    return frames, (mid_at, 0, giant2_at, long_at)


@functools.lru_cache(maxsize=None)
def digest_case(kind):
    """kind "rx": the frames back to back; "fcs": each with its FCS (every 7th damaged), lengths
    including it; "fill": 4 spare bytes behind each. With what the oracle says of the small copy."""
    frames, targets = digest_frames()
    if kind == "fcs":
        frames = cref.with_fcs(frames, damage=range(0, len(frames), 7))
    buf, off, ln = pack(frames, 4 if kind == "fill" else 0, seed=len(kind))
    assert {int(x) for x in off % 4} == {0, 1, 2, 3}, "every start alignment"
    mid = targets[0]
    cuts = [c for f in targets for c in frame_cuts(ln, f)]
    cuts += [(mid, int(ln[mid]) // 2 + r) for r in range(1, 64)]  # with the cut above: every base mod 64
    case = Placed(buf, off, ln, cuts, seed=len(kind))
    if kind == "rx":
        case.exp = {mtu: coracle.digest_batch(buf, off, ln, mtu) for mtu in (0, 1514)}
    elif kind == "fcs":
        case.exp = {mtu: coracle.digest_fcs_batch(buf, off, ln, mtu) for mtu in (0, 1514)}
        assert 14 in case.exp[0][1] and 0 in case.exp[0][1]
    else:
        case.filled = {}
    return case


def words(dig):
    return np.stack([dig["crc32"].astype(np.uint32),
                     dig["ip_csum"].astype(np.uint32) | (dig["l4_csum"].astype(np.uint32) << 16)], axis=1)


def same_digests(out, st, exp, ln, label):
    w = out.cpu().numpy().view(np.uint32).reshape(-1, 2)
    bad = np.flatnonzero((w != words(exp[0])).any(axis=1) | (st.cpu().numpy() != exp[1]))
    assert bad.size == 0, f"{label}: {bad.size} of {ln.size} frames differ; first i={int(bad[0])} len={int(ln[bad[0]])}"


FORCED = {4: 4, 2: 2, 3: 3, engines.SMALL_EXACT: 8}  # the kernel a forced variant must have run


def rx_sweep(engine, big, which, kind, call):
    import torch

    e, variant = engine
    case = digest_case(kind)
    ln_dev, seen = dev(case.ln), 0
    try:
        for label, bases in placements(case, big, which):
            assert_beyond(big, which, case.off, case.ln, bases)
            put_all(case, big, bases)
            off_dev = dev(case.off + bases)
            for wg in (0, 1):  # the whole grid (tiles of 4 frames at this size), and one workgroup (tiles of 16)
                e.set_workgroups(wg)
                for mtu in (0, 1514):
                    out, st = call(e)(big, off_dev, ln_dev, mtu=mtu)
                    torch.cuda.synchronize()
                    if variant in FORCED:
                        assert e.last_kernel() == FORCED[variant], (label, e.last_kernel())
                    same_digests(out, st, case.exp[mtu], case.ln, f"{label}, mtu {mtu}, workgroups {wg}")
            seen += 1
    finally:
        e.set_workgroups(0)
    assert seen == (4 if which == "both" else len(case.cuts)) and seen >= 4


@gpu
@pytest.mark.parametrize("which", PLACEMENTS)
def test_digest(engine, big, which):
    rx_sweep(engine, big, which, "rx", lambda e: e.digest_device)


@gpu
@pytest.mark.parametrize("which", PLACEMENTS)
def test_digest_fcs(engine, big, which):
    rx_sweep(engine, big, which, "fcs", lambda e: e.digest_fcs_device)


def filled_window(case, mask):
    """The window after a fill of the frames in `mask`, by the oracle on the small copy."""
    key = mask.tobytes()
    if key not in case.filled:
        w = case.window.copy()
        coracle.fill_batch(w, (case.off + MARGIN)[mask], case.ln[mask], 0, 3)
        case.filled[key] = w
    return case.filled[key]


@gpu
@pytest.mark.parametrize("which", PLACEMENTS)
def test_fill(engine, big, which):
    import torch

    e, variant = engine
    case = digest_case("fill")
    if not hasattr(case, "exp"):
        case.exp = coracle.fill_batch(case.window.copy(), case.off + MARGIN, case.ln, 0, 3)
    ln_dev = dev(case.ln)
    try:
        for label, bases in placements(case, big, which):
            assert_beyond(big, which, case.off, case.ln + 4, bases)
            off_dev = dev(case.off + bases)
            for wg in (0, 1):
                e.set_workgroups(wg)
                put_all(case, big, bases)
                out, st = e.fill_device(big, off_dev, ln_dev, flags=3)
                torch.cuda.synchronize()
                if variant in (2, 3, 4):
                    assert e.last_kernel() == variant, (label, e.last_kernel())
                assert e.last_kernel() != 8, "a TX fill never runs the small-frame kernel"
                same_digests(out, st, case.exp, case.ln, f"{label}, workgroups {wg}")
                for b in np.unique(bases):  # the whole window of every copy, margins included
                    diff = np.flatnonzero(case.fetch(big, int(b)) != filled_window(case, bases == b))
                    assert diff.size == 0, f"{label}, copy at {int(b)}: {diff.size} bytes differ, first at {int(diff[0]) - MARGIN}"
    finally:
        e.set_workgroups(0)


# ---- 2. TX frame build ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tx_case():
    from test_gpu_segment import edge_specs

    specs, payload = edge_specs()
    at = np.array([s[1] for s in specs], dtype=np.int64)
    ln = np.array([s[2] for s in specs], dtype=np.int32)
    longest = int(np.argmax(ln))
    one = next(i for i, s in enumerate(specs) if s[3] == 1 and s[2] > 4)  # one payload byte per frame
    udp = next(i for i, s in enumerate(specs) if s[0][23] == 17 and s[2] >= 63)
    cuts = [(f, p) for f in (longest, one, udp) for p in (1, int(ln[f]) // 2, int(ln[f]) - 1, int(ln[f]))]
    case = Placed(payload, at, ln, cuts, seed=2)
    case.specs = specs
    return case


@gpu
@pytest.mark.parametrize("which", PLACEMENTS)
def test_tx_payload_beyond_4gib(eng, big, which):
    """payload_off >= 2^32 for every send, a send whose payload range straddles 2^32 (offset and
    address), and sends that read in turn below 1 MiB and above 2^32; payload_bytes is the big tensor's
    size. The frames go to a small tensor and everything is compared with the restatement."""
    import torch

    from seqs_amd import segment_layout
    from test_gpu_segment import TAIL, compare

    case = tx_case()
    sends0 = sref.make_sends(case.specs)
    expected, inside = {}, 0
    todo = list(placements(case, big, which))
    if which == "offset":
        todo.append(("every payload_off above 2^32", np.full(case.off.size, G + 4099, dtype=np.int64)))
    for k, (label, bases) in enumerate(todo):
        flags, align = (FCS, 1) if k % 2 else (0, 64)
        if (flags, align) not in expected:
            _, nbytes = segment_layout(sends0, flags, align)
            noise = np.random.default_rng(align).integers(0, 256, nbytes + TAIL, dtype=np.uint8)
            expected[flags, align] = (noise, sref.expected(case.specs, case.buf, 0, flags, align, noise))
        noise, exp = expected[flags, align]
        if label.startswith("every"):
            assert int((case.off + bases).min()) >= G
        else:
            assert_beyond(big, which, case.off, case.ln, bases)
        put_all(case, big, bases)
        sends = sends0.copy()
        sends["payload_off"] = (case.off + bases).astype(np.uint64)
        po = case.off + bases
        inside += int(((po < G) & (po + case.ln > G)).any())  # a send whose own range straddles 2^32
        buf = dev(noise)
        _, off, ln, out, st = eng.segment_device(sends, big, 0, flags, align, frames=buf)
        torch.cuda.synchronize()
        compare(buf.cpu().numpy(), off, ln, out, st, *exp)
        for b in np.unique(bases):  # the payload is only read
            assert np.array_equal(case.fetch(big, int(b)), case.window), label
    assert which != "offset" or inside >= 6


@functools.lru_cache(maxsize=None)
def big_layout(flags=FCS):
    """259 TCP sends of about 4,090 frames each with a small mss and align 4096, all reading one shared
    payload range: 1.05 M frames whose slots end above 2^32 while few bytes are written. Returns (sends,
    lengths, offsets, frames_bytes, first frame of each send (and the frame count), specs), the layout
    computed here with numpy."""
    rng = np.random.default_rng(2024)
    k = np.arange(259)
    mss = np.array([7, 16, 5, 13])[k % 4]
    nf = 4096 - (k % 5) * 13
    last = 1 + k % mss  # the last frame's chunk
    plen = mss * (nf - 1) + last
    specs = [(sref.tcp_header(rng, seq=int(rng.integers(0, 1 << 32))), int((13 * i) % 1000), int(plen[i]), int(mss[i]))
             for i in k]
    first = np.concatenate([[0], np.cumsum(nf)]).astype(np.int64)
    lens = np.repeat(54 + mss, nf).astype(np.uint32)
    lens[first[1:] - 1] = 54 + last
    assert int(lens.max()) + (4 if flags & FCS else 0) <= 4096  # every slot is one 4,096-byte block
    offs = np.arange(lens.size, dtype=np.uint64) * np.uint64(4096)
    return sref.make_sends(specs), lens, offs, int(lens.size) * 4096, first, specs


@gpu
def test_tx_frames_beyond_4gib(eng, big):
    """Slots that pass 4 GiB: offsets and lengths in full against the numpy layout, every verdict, the
    frames of the first send, of the send whose slots straddle 2^32 and of the last send byte for byte
    (with their digests) against the restatement, and every gap byte of every slot on the device."""
    import torch

    from seqs_amd import segment_layout, split_digests

    sends, lens, offs, total, first, specs = big_layout(FCS)
    n = lens.size
    assert segment_layout(sends, FCS, 4096) == (n, total) and G < total and total + MARGIN <= big.numel()
    payload = np.random.default_rng(5).integers(0, 256, 1000 + (1 << 16) + 64, dtype=np.uint8)
    big[: total + MARGIN].fill_(FILL)
    _, off, ln, out, st = eng.segment_device(sends, dev(payload), 0, FCS, 4096, frames=big)
    torch.cuda.synchronize()
    assert int(off.max()) >= G and int(off[-1]) + 4096 == total
    assert torch.equal(off, dev(offs.astype(np.int64))) and torch.equal(ln, dev(lens.astype(np.int32)))
    assert int(st.max()) == 0 and st.numel() == n
    base = offs[first[:-1]]
    straddle = int(np.searchsorted(base, G)) - 1
    assert 0 < straddle < sends.size - 1 and int(base[straddle]) < G < int(base[straddle + 1])
    crc, ipc, l4c = split_digests(out.cpu().numpy())
    for k in (0, straddle, sends.size - 1):
        f0, f1 = int(first[k]), int(first[k + 1])
        ebuf, eoff, eln, edig, est = sref.expected([specs[k]], payload, 0, FCS, 4096,
                                                   np.full((f1 - f0) * 4096, FILL, dtype=np.uint8))
        assert np.array_equal(eoff + offs[f0], offs[f0:f1]) and np.array_equal(eln, lens[f0:f1]) and (est == 0).all()
        diff = np.flatnonzero(big[f0 * 4096 : f1 * 4096].cpu().numpy() != ebuf)
        assert diff.size == 0, f"send {k}: {diff.size} bytes differ, first at {int(diff[0])} of its slots"
        assert np.array_equal(crc[f0:f1], edig["crc32"]) and np.array_equal(ipc[f0:f1], edig["ip_csum"])
        assert np.array_equal(l4c[f0:f1], edig["l4_csum"])
    # the gap bytes of every slot (what lies behind a frame and its FCS), and the bytes behind the last slot
    cols = torch.arange(4096, device=big.device, dtype=torch.int32)
    for r0 in range(0, n, 1 << 16):
        r1 = min(n, r0 + (1 << 16))
        rows = big[r0 * 4096 : r1 * 4096].view(-1, 4096)
        used = cols[None, :] < (ln[r0:r1] + 4)[:, None]
        assert bool(((rows == FILL) | used).all()), f"a gap byte of frames {r0}..{r1} was written"
    assert bool((big[total : total + MARGIN] == FILL).all())


# ---- 3. RX coalesce and flow-aware coalesce ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rx_cases(fcs):
    """The batches of test_two_interleaved_flows and test_rejected_frames, and 257 segments of 28 flows
    in random interleave with rejects; with their FCS (some damaged) when `fcs`."""
    import test_gpu_flows as tf

    rng = np.random.default_rng(51)
    a = fref.finish(fref.segments(rng, fref.flow_header(rng, 0x5151), 700, [40, 50, 60, 70]))
    b = fref.finish(fref.segments(rng, fref.flow_header(rng, 0x5252), 9, [11, 12]))
    lists = [tf.two_flows(), [a[0], a[1], tf.damaged(b[0]), a[2], a[3], b[1]], tf.small_batch(257, 28, 257, reject=0.1)]
    cases = []
    for k, frames in enumerate(lists):
        if fcs:
            frames = cref.with_fcs(frames, damage=range(3, len(frames), 11))
        buf, off, ln = cref.pack(frames, lead=1 + k, seed=k)
        mid = len(frames) // 2
        cuts = frame_cuts(ln, mid) + [(mid, 2 + (7 * j) % (int(ln[mid]) - 2)) for j in range(9)]  # (more bases mod 64)
        cases.append(Placed(buf, off, ln, cuts, seed=10 + k))
    return cases


@gpu
@pytest.mark.parametrize("fcs", [False, True])
def sockets_of_the_flows(case, e):
    """One socket per TCP flow of the batch (flows_ref.expected's dict `e`), expecting the Seq of the
    flow's first frame; rings one sentinel byte apart in a small buffer of their own, every second one
    too short for its flow. Returns (socks, rings_bytes)."""
    socks, at = [], 1
    for k, fl in enumerate(e["flows"]):
        i = int(e["order"][int(fl["first_frame"])])
        f = case.buf[int(case.off[i]) : int(case.off[i]) + int(case.ln[i])].tobytes()
        if f[23] != 6:
            continue
        size = max(1, int(fl["payload_len"]) * (3 if k % 2 else 4) // 4)
        socks.append(dcases.sock_of(f, dcases.seq_of(f), at, size, ring_wpos=size - 1 - k % size))
        at += size + 1
    return dref.socks_of(*socks), at + 2


@gpu
@pytest.mark.parametrize("fcs", [False, True])
@pytest.mark.parametrize("call", ["coalesce", "flows", "deliver", "recv"])
@pytest.mark.parametrize("which", PLACEMENTS)
def test_rx_source_beyond_4gib(eng, big, which, call, fcs):
    """The frames read from beyond 2^32: payload with its noise margins, runs, (flows, order,) run_of,
    totals, digests and verdicts against the restatement of the small copy; for the delivery also
    socks_out, delivered and the whole of a small rings buffer, one socket per TCP flow; for the receive
    call (whose gather forms a 64-bit frame address of its own) also snd_out and code, each socket's
    snd.UNA 100 behind its snd.NXT."""
    import torch

    import recv_ref as rref
    import test_gpu_coalesce as tc
    import test_gpu_deliver as td
    import test_gpu_flows as tf
    import test_gpu_recv as tr

    flags = cref.RX_FCS if fcs else 0
    for k, case in enumerate(rx_cases(fcs)):
        room, plead = int(case.ln.sum()), 3 + k
        noise = np.random.default_rng(77 + k).integers(0, 256, plead + room + tc.TAIL, dtype=np.uint8)
        ref = cref if call == "coalesce" else fref
        e = ref.expected(case.buf, case.off, case.ln, 0, flags, noise, plead, room)
        assert e["n_runs"] >= 2 and e["payload_bytes"] > 0 and (k == 0 or (e["st"] != 0).any())
        ln_dev, noise_dev = dev(case.ln), dev(noise)
        if call in ("deliver", "recv"):
            socks, rings_bytes = sockets_of_the_flows(case, e)
            rings = td.sentinel(rings_bytes, k)
            if call == "recv":
                snd = tr.snd_behind(socks)
                e = rref.expected(case.buf, case.off, case.ln, 0, flags, noise, plead, room, socks, snd, rings)
                assert int((e["code"] != 0).sum()) == int((e["delivered"] != 0).sum()) and {1, 6} <= {int(c) for c in e["code"]}
            else:
                e = dref.expected(case.buf, case.off, case.ln, 0, flags, noise, plead, room, socks, rings)
            assert socks.size == e["n_flows"] >= 2 and (e["delivered"] == 1).any() and (k == 0 or (e["delivered"] == 2).any())
            rings_dev = dev(rings)
        for label, bases in placements(case, big, which):
            assert_beyond(big, which, case.off, case.ln, bases)
            put_all(case, big, bases)
            pt = noise_dev.clone()
            if call == "coalesce":
                res = eng.coalesce_device(big, dev(case.off + bases), ln_dev, 0, flags, payload=pt[plead : plead + room])
                torch.cuda.synchronize()
                tc.compare(e, pt.cpu().numpy(), *res[1:])
            elif call == "deliver":
                rt = rings_dev.clone()
                res = eng.deliver_flows_device(big, dev(case.off + bases), ln_dev, socks, rt, 0, flags,
                                               payload=pt[plead : plead + room])
                torch.cuda.synchronize()
                td.compare_delivery(e, res[0], res[1], rt)
                tf.compare(e, pt.cpu().numpy(), *res[3:])
            elif call == "recv":
                rt = rings_dev.clone()
                res = eng.recv_flows_device(big, dev(case.off + bases), ln_dev, socks, snd, rt, 0, flags,
                                            payload=pt[plead : plead + room])
                torch.cuda.synchronize()
                tr.compare_recv(e, res[0], res[1])
                td.compare_delivery(e, res[2], res[3], rt)
                tf.compare(e, pt.cpu().numpy(), *res[5:])
            else:
                res = eng.coalesce_flows_device(big, dev(case.off + bases), ln_dev, 0, flags, payload=pt[plead : plead + room])
                torch.cuda.synchronize()
                tf.compare(e, pt.cpu().numpy(), *res[1:])


@gpu
def test_deliver_rings_beyond_4gib(eng, big):
    """The rings tensor longer than 4 GiB. Ring A has the maximal 2^31 bytes at ring_off 2^31 + 32 MiB,
    so it spans offset 2^32: three 100-byte segments from wpos 2^31 - 100 wrap at its end; a second
    call with wpos 2^31 - 32 MiB - 50 puts a payload across offset 2^32 itself. Ring B (4,096 bytes)
    lies wholly beyond 2^32 and ends with the tensor. Every flow is in order and fits, so what is
    expected is the closed form: byte j of a flow's payloads at (wpos + j) mod ring_size. Windows of
    MARGIN bytes around every write are compared on the host; the rest of the tensor is checked on the
    device to hold FILL still."""
    import torch

    import test_gpu_flows as tf
    from seqs_amd import split_socks

    rng = np.random.default_rng(4321)
    A_OFF, A_SIZE, B_OFF, B_SIZE = (1 << 31) + (32 << 20), 1 << 31, BIG_BYTES - 4096, 4096
    assert A_OFF < G < A_OFF + A_SIZE <= B_OFF and G < B_OFF and B_OFF + B_SIZE == big.numel()
    hdrs = [fref.flow_header(rng, 0xA100), fref.flow_header(rng, 0xB100)]
    seq = [(1 << 32) - 250, 5000]
    wpos = {0: [A_SIZE - 100, 4000], 1: [A_SIZE - (32 << 20) - 50, None]}
    big.fill_(FILL)
    written = []
    for call in (0, 1):
        segs = [fref.segments(rng, hdrs[f], seq[f], [100] * 3) for f in (0, 1)]
        frames = fref.finish([segs[g][k] for g, k in fref.interleave([range(3)] * 2)])
        buf, off, ln = fref.pack(frames, lead=call + 1)
        if wpos[1][1] is None:
            wpos[1][1] = (4000 + 300) % B_SIZE
        wa, wb = wpos[call]
        assert A_OFF + wa < G < A_OFF + wa + 100 or call == 0
        socks = dref.socks_of(dcases.sock_of(segs[0][0], seq[0], A_OFF, A_SIZE, ring_wpos=wa),
                              dcases.sock_of(segs[1][0], seq[1], B_OFF, B_SIZE, ring_wpos=wb))
        room = int(ln.sum())
        noise = np.random.default_rng(call).integers(0, 256, room + 96, dtype=np.uint8)
        e = fref.expected(buf, off, ln, 0, 0, noise, 0, room)
        pt = dev(noise)
        res = eng.deliver_flows_device(dev(buf), dev(off.astype(np.int64)), dev(ln.astype(np.int32)), socks, big,
                                       payload=pt[:room])
        torch.cuda.synchronize()
        tf.compare(e, pt.cpu().numpy(), *res[3:])
        assert bool((res[1] == 1).all())
        so = split_socks(res[0])
        for f, (lo, size, w) in enumerate(((A_OFF, A_SIZE, wa), (B_OFF, B_SIZE, wb))):
            assert [int(so[f][k]) for k in so.dtype.names] == [(seq[f] + 300) % G, (w + 300) % size, size - 300, 300, 3, 0, f, 3 * (f + 1)]
            data = np.frombuffer(b"".join(s[54:] for s in segs[f]), dtype=np.uint8)
            first = min(300, size - w)
            for at, piece in ((lo + w, data[:first]), (lo, data[first:])):
                if piece.size == 0:
                    continue
                w0, w1 = max(0, at - MARGIN), min(big.numel(), at + piece.size + MARGIN)
                written.append((at, piece))
                want = np.full(w1 - w0, FILL, dtype=np.uint8)
                for x, p in written:  # (an earlier call's bytes may lie in this window)
                    a, b = max(x, w0), min(x + p.size, w1)
                    if a < b:
                        want[a - w0 : b - w0] = p[a - x : b - x]
                got = big[w0:w1].cpu().numpy()
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, f"call {call}, ring {f}: {bad.size} bytes differ around {at}, first at {w0 + int(bad[0])}"
            seq[f] += 300
    written = [(at, at + p.size) for at, p in written]
    assert any(a < G < b for a, b in written) and any(a == A_OFF for a, _ in written) and any(b == big.numel() for _, b in written)
    assert any(b == A_OFF + A_SIZE for _, b in written)
    for a, b in written:  # what was written (and compared above) back to FILL: the whole tensor holds it again
        big[a:b].fill_(FILL)
    for c0 in range(0, big.numel(), 1 << 28):
        assert bool((big[c0 : c0 + (1 << 28)] == FILL).all()), f"a byte of {c0}..{c0 + (1 << 28)} outside the writes was written"


@functools.lru_cache(maxsize=None)
def jumbo_table():
    """Six distinct jumbo TCP frames: three consecutive segments of flow A (its Seq wraps inside the
    second), two of flow B, and a damaged copy of A's second segment. With what the references say of
    each: verdict, digest, payload range, flags, flow key, and the table of which continues which."""
    import test_gpu_flows as tf

    rng = np.random.default_rng(JUMBO)
    a = cref.segments(rng, cref.flow_header(rng, 0xA000), G - 100000, [JUMBO] * 3)
    b = cref.segments(rng, cref.flow_header(rng, 0xB000), 12345, [JUMBO] * 2)
    frames = cref.finish(a + b)
    frames.append(tf.damaged(frames[1], 54 + 30000))
    buf, off, ln = cref.pack(frames, lead=3)
    dig, st = coracle.digest_batch(buf, off, ln, 0)
    assert list(st) == [0, 0, 0, 0, 0, 13]
    D = len(frames)
    rng_ = [cref.payload_range(f) for f in frames]
    joins = np.array([[bool(st[p] == 0 and st[c] == 0 and cref.joins(frames[p], frames[c])) for c in range(D)]
                      for p in range(D)])
    assert joins[0, 1] and joins[1, 2] and joins[3, 4] and int(joins.sum()) == 3
    keys = [fref.flow_key(f) for f in frames]
    return dict(frames=frames, buf=buf, off=off.astype(np.int64), ln=ln.astype(np.int32), dig=dig, st=st,
                start=np.array([r[0] for r in rng_]), plen=np.array([r[1] - r[0] for r in rng_], dtype=np.uint64),
                flags=np.array([f[47] for f in frames], dtype=np.uint8), joins=joins,
                key=np.array([keys.index(k) for k in keys]))


BLOCKS = [[0, 1, 2], [0, 2], [1, 5, 2], [2, 1], [3, 4], [4, 3]]
WEIGHTS = [0.5, 0.2, 0.2, 0.098, 0.001, 0.001]


def index_list(accepted, seed):
    """Indices into the distinct frames, made of blocks in which some entries continue each other and
    some do not, some with the rejected frame between them; flow A comes first and is the long one. Cut
    where `accepted` accepted frames are listed."""
    rng = np.random.default_rng(seed)
    out = [0, 1, 2]
    for b in rng.choice(len(BLOCKS), size=accepted // 2 + 16, p=WEIGHTS):
        out += BLOCKS[int(b)]
    idx = np.array(out, dtype=np.int64)
    ok = np.cumsum(idx != 5)
    idx = idx[: int(np.searchsorted(ok, accepted)) + 1]
    assert int((idx != 5).sum()) == accepted
    return idx


def run_records(d, allowed, tab, first_frame):
    """RUN_DTYPE records of the delivery sequence `d` (distinct-frame indices, all accepted) in which
    entry k may continue entry k - 1 where allowed[k]. payload_len is the run's length modulo 2^32
    (include/framesum.h); everything else is exact. Returns (runs, run of each entry, byte offsets)."""
    from seqs_amd.framesum import RUN_DTYPE

    m = d.size
    start = np.ones(m, dtype=bool)
    start[1:] = ~(allowed[1:] & tab["joins"][d[:-1], d[1:]])
    rid = np.cumsum(start) - 1
    at = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(tab["plen"][d], dtype=np.uint64)])
    firsts = np.flatnonzero(start)
    counts = np.diff(np.append(firsts, m))
    lasts = firsts + counts - 1
    runs = np.zeros(firsts.size, dtype=RUN_DTYPE)
    runs["payload_off"] = at[firsts]
    runs["payload_len"] = ((at[lasts + 1] - at[firsts]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    runs["first_frame"] = first_frame[firsts]
    runs["n_frames"] = counts
    runs["tcp_flags"] = tab["flags"][d[firsts]] | (tab["flags"][d[lasts]] & (cref.FIN | cref.PSH))
    return runs, rid.astype(np.uint32), at


def expand_coalesce(tab, idx):
    """fs_coalesce_batch of the frames listed by idx, expanded from the distinct frames with numpy."""
    ai = np.flatnonzero(tab["st"][idx] == 0)
    d = idx[ai]
    allowed = np.ones(d.size, dtype=bool)
    allowed[1:] = np.diff(ai) == 1  # a rejected frame between two frames breaks the run
    runs, rid, at = run_records(d, allowed, tab, ai)
    run_of = np.full(idx.size, cref.NO_RUN, dtype=np.uint32)
    run_of[ai] = rid
    return dict(runs=runs, run_of=run_of, payload_bytes=int(at[-1]), n_runs=runs.size, deliv=d, at=at)


def expand_flows(tab, idx):
    """fs_coalesce_flows_batch of the same: flows numbered by their first frames, the delivery order flow
    by flow and in batch order inside a flow, the join rule along that order."""
    from seqs_amd.framesum import FLOW_DTYPE

    ai = np.flatnonzero(tab["st"][idx] == 0)
    key = tab["key"][idx[ai]]
    uniq, first_seen = np.unique(key, return_index=True)
    number = np.zeros(int(uniq.max()) + 1, dtype=np.int64)
    number[uniq[np.argsort(first_seen)]] = np.arange(uniq.size)
    fno = number[key]
    by_flow = np.argsort(fno, kind="stable")
    order, fno = ai[by_flow], fno[by_flow]
    d = idx[order]
    allowed = np.ones(d.size, dtype=bool)
    allowed[1:] = fno[1:] == fno[:-1]
    runs, rid, at = run_records(d, allowed, tab, np.arange(d.size))
    run_of = np.full(idx.size, cref.NO_RUN, dtype=np.uint32)
    run_of[order] = rid
    flows = np.zeros(uniq.size, dtype=FLOW_DTYPE)
    lo = np.searchsorted(fno, np.arange(uniq.size))
    hi = np.searchsorted(fno, np.arange(uniq.size), side="right")
    flows["payload_off"], flows["payload_len"] = at[lo], at[hi] - at[lo]
    flows["first_run"], flows["n_runs"] = rid[lo], rid[hi - 1] - rid[lo] + 1
    flows["first_frame"], flows["n_frames"] = lo, hi - lo
    return dict(runs=runs, run_of=run_of, payload_bytes=int(at[-1]), n_runs=runs.size, deliv=d, at=at, flows=flows,
                order=order.astype(np.uint32), n_flows=flows.size, n_accepted=d.size)


def test_expansion_equals_the_restatements(oracle_lib):
    """The numpy expansion above against the sequential restatements, on a list short enough for them."""
    tab = jumbo_table()
    idx = index_list(300, 3)
    idx[40:44] = [3, 4, 4, 3]  # (flow B is rare in the list: make sure it is in this short one)
    assert {0, 1, 2, 3, 4, 5} <= set(idx.tolist())
    off, ln = tab["off"][idx], tab["ln"][idx]
    none = np.zeros(0, dtype=np.uint8)
    for ref, mine in ((cref, expand_coalesce(tab, idx)), (fref, expand_flows(tab, idx))):
        e = ref.expected(tab["buf"], off, ln, 0, 0, none, 0, 0)
        assert e["runs"].tobytes() == mine["runs"].tobytes() and np.array_equal(e["run_of"], mine["run_of"])
        assert (e["payload_bytes"], e["n_runs"]) == (mine["payload_bytes"], mine["n_runs"])
        assert 1 < int(e["runs"]["n_frames"].max()) <= 3 and int((e["runs"]["n_frames"] == 1).sum()) > 10
        if ref is fref:
            assert e["flows"].tobytes() == mine["flows"].tobytes() and np.array_equal(e["order"], mine["order"])
            assert e["n_flows"] == 2 and e["n_accepted"] == mine["n_accepted"] >= 300
    # in the flow-aware form the rejected frame between two segments does not break their run
    assert expand_flows(tab, idx)["n_runs"] < expand_coalesce(tab, idx)["n_runs"]


def check_tiled(big, tab, exp, fit, label):
    """The gathered payload on the device: entry k of the delivery order holds the payload of its
    distinct frame, for the first `fit` entries, compared in chunks of 8,000 frames (under 512 MiB)."""
    import torch

    pays = dev(np.stack([np.frombuffer(f[int(s) : int(s) + JUMBO], dtype=np.uint8)
                         for f, s in zip(tab["frames"], tab["start"])]))
    d = dev(exp["deliv"])
    for c0 in range(0, fit, 8000):
        c1 = min(fit, c0 + 8000)
        got = big[c0 * JUMBO : c1 * JUMBO].view(-1, JUMBO)
        assert torch.equal(got, pays[d[c0:c1]]), f"{label}: payload of delivered frames {c0}..{c1} differs"


@gpu
@pytest.mark.parametrize("call", ["coalesce", "flows"])
def test_rx_destination_beyond_4gib(eng, big, call):
    """A gathered payload longer than 4 GiB: 66,000 accepted jumbo frames. Runs (payload_off as a 64-bit
    running sum), run_of, totals, (flows and order,) digests and verdicts in full; the payload on the
    device; once more with payload_cap = 2^32 + 1000, which cuts the copy short above 4 GiB and
    changes nothing else. In the flow-aware form flow A alone passes 2^32, so flow B's payload_off
    lies above it."""
    import torch

    from seqs_amd import TOTALS_DTYPE, split_digests, split_flows, split_runs

    tab = jumbo_table()
    idx = index_list(66000, 7)
    exp = (expand_coalesce if call == "coalesce" else expand_flows)(tab, idx)
    total = exp["payload_bytes"]
    assert total == 66000 * JUMBO > G and total + MARGIN <= big.numel()
    assert int(exp["runs"]["payload_off"].max()) >= G and int(exp["runs"]["n_frames"].max()) == 3
    assert (tab["st"][idx] != 0).any() and 1000 < exp["n_runs"] < 66000
    if call == "flows":
        assert exp["n_flows"] == 2 and int(exp["flows"]["payload_off"][1]) > G
        assert int(exp["flows"]["payload_len"][0]) > G and int(exp["flows"]["payload_len"][1]) >= 2 * JUMBO
    frames, off, ln = dev(tab["buf"]), dev(tab["off"][idx]), dev(tab["ln"][idx])
    for cap in (total, G + 1000):
        fit = min(66000, cap // JUMBO)  # (every accepted frame carries JUMBO bytes)
        assert cap > G and (fit == 66000 or fit * JUMBO <= cap < (fit + 1) * JUMBO)
        big[: total + MARGIN].fill_(FILL)  # (also what an earlier run gathered)
        if call == "coalesce":
            _, runs, run_of, totals, out, st = eng.coalesce_device(frames, off, ln, 0, 0, payload=big[:cap])
            torch.cuda.synchronize()
            r, nbytes, n_runs = split_runs(runs, totals)
            t = np.ascontiguousarray(totals.cpu().numpy()).view(TOTALS_DTYPE)[0]
        else:
            _, runs, flows, order, run_of, totals, out, st = eng.coalesce_flows_device(frames, off, ln, 0, 0,
                                                                                       payload=big[:cap])
            torch.cuda.synchronize()
            r, f, o, t = split_flows(runs, flows, order, totals)
            nbytes, n_runs = int(t["payload_bytes"]), int(t["n_runs"])
            assert (int(t["n_flows"]), int(t["n_accepted"])) == (2, 66000)
            assert f.tobytes() == exp["flows"].tobytes(), (f, exp["flows"])
            assert np.array_equal(o, exp["order"])
        assert (nbytes, n_runs, int(t["reserved"])) == (total, exp["n_runs"], 0)
        bad = np.flatnonzero(r != exp["runs"])
        assert bad.size == 0, (cap, bad[:4], r[bad[:4]], exp["runs"][bad[:4]])
        assert np.array_equal(run_of.cpu().numpy().view(np.uint32), exp["run_of"])
        crc, ipc, l4c = split_digests(out.cpu().numpy())
        dig = tab["dig"][idx]
        assert np.array_equal(crc, dig["crc32"]) and np.array_equal(ipc, dig["ip_csum"]) and np.array_equal(l4c, dig["l4_csum"])
        assert np.array_equal(st.cpu().numpy(), tab["st"][idx])
        check_tiled(big, tab, exp, fit, f"cap {cap}")
        # nothing behind the last frame that fits, and nothing behind the payload
        assert bool((big[fit * JUMBO : total + MARGIN] == FILL).all()), f"cap {cap}: bytes behind frame {fit} were written"


@gpu
def test_run_longer_than_4gib(eng, big):
    """fs_rx_run.payload_len is 32-bit and the join rule compares Seq modulo 2^32, so one run can carry
    more than 4 GiB. The contract (include/framesum.h): payload_len then holds the run's length modulo
    2^32, while n_frames, the next run's payload_off, fs_rx_flow.payload_len and the totals stay exact.
    A chain cannot revisit a frame before 2^32 bytes have passed (each frame's Seq is fixed), so this
    one is 65,596 distinct jumbo segments, built by fs_segment_batch into the big tensor: 16 sends of
    4,096 frames and one of 60, each send's Seq continuing the one before, then one frame of another
    flow."""
    import torch

    from seqs_amd import FLOW_DTYPE, RUN_DTYPE, segment_layout, split_flows, split_runs

    rng = np.random.default_rng(17)
    S, seq0 = 4096, 0xFFF00000
    src_len, tail_len = S * JUMBO, 100
    counts = [S] * 16 + [60]
    hdr = bytearray(sref.tcp_header(rng, flags=cref.ACK))
    specs, n_chain = [], 0
    for c in counts:
        h = bytearray(hdr)
        h[18:20] = int(rng.integers(0, 1 << 16)).to_bytes(2, "big")
        h[38:42] = ((seq0 + n_chain * JUMBO) % G).to_bytes(4, "big")
        specs.append((bytes(h), 0, c * JUMBO, JUMBO))
        n_chain += c
    specs.append((sref.tcp_header(rng, flags=cref.ACK | cref.PSH), src_len, tail_len, 0))
    chain_bytes = n_chain * JUMBO
    assert n_chain == 65596 and chain_bytes > G and chain_bytes - G < JUMBO * 60
    sends = sref.make_sends(specs)
    n, nbytes = segment_layout(sends, 0, 1)
    assert n == n_chain + 1 and G < nbytes <= big.numel()
    src = torch.randint(0, 256, (src_len + tail_len,), dtype=torch.uint8, device=big.device)
    _, off, ln, _, st = eng.segment_device(sends, src, 0, 0, 1, frames=big)
    torch.cuda.synchronize()
    assert int(st.max()) == 0 and int(off.max()) >= G
    total = chain_bytes + tail_len
    dest = torch.empty(total + MARGIN, dtype=torch.uint8, device=big.device)
    dest[total:].fill_(FILL)

    runs = np.zeros(2, dtype=RUN_DTYPE)
    runs["payload_off"], runs["payload_len"] = [0, chain_bytes], [chain_bytes % G, tail_len]
    runs["first_frame"], runs["n_frames"] = [0, n_chain], [n_chain, 1]
    runs["tcp_flags"] = [cref.ACK, cref.ACK | cref.PSH]
    run_of = np.concatenate([np.zeros(n_chain, dtype=np.uint32), [1]]).astype(np.uint32)

    def payload_is_the_source(label):
        for k, c in enumerate(counts):
            assert torch.equal(dest[k * src_len : k * src_len + c * JUMBO], src[: c * JUMBO]), f"{label}: send {k}"
        assert torch.equal(dest[chain_bytes:total], src[src_len:]) and bool((dest[total:] == FILL).all()), label

    _, r, ro, totals, _, vd = eng.coalesce_device(big, off, ln, 0, 0, payload=dest[:total])
    torch.cuda.synchronize()
    got, nb, nr = split_runs(r, totals)
    assert int(vd.max()) == 0 and (nb, nr) == (total, 2)
    assert got.tobytes() == runs.tobytes(), (got, runs)
    assert np.array_equal(ro.cpu().numpy().view(np.uint32), run_of)
    payload_is_the_source("fs_coalesce_batch")

    dest[:total].zero_()
    _, r, fl, order, ro, totals, _, vd = eng.coalesce_flows_device(big, off, ln, 0, 0, payload=dest[:total])
    torch.cuda.synchronize()
    got, f, o, t = split_flows(r, fl, order, totals)
    flows = np.zeros(2, dtype=FLOW_DTYPE)
    flows["payload_off"], flows["payload_len"] = [0, chain_bytes], [chain_bytes, tail_len]  # 64-bit: exact
    flows["first_run"], flows["n_runs"], flows["first_frame"], flows["n_frames"] = [0, 1], [1, 1], [0, n_chain], [n_chain, 1]
    assert (int(t["payload_bytes"]), int(t["n_runs"]), int(t["n_flows"]), int(t["n_accepted"])) == (total, 2, 2, n)
    assert got.tobytes() == runs.tobytes(), (got, runs)
    assert f.tobytes() == flows.tobytes(), (f, flows)
    assert np.array_equal(o, np.arange(n, dtype=np.uint32)) and np.array_equal(ro.cpu().numpy().view(np.uint32), run_of)
    payload_is_the_source("fs_coalesce_flows_batch")


# ---- 4. the host-staged entry points with a span above 2^32 --------------------------------------

HOST_BYTES = G + (2 << 20)
HOST_BASE = G + (1 << 20) + 4099  # inside the last MiB


@pytest.fixture(scope="module")
def host():
    """A host buffer longer than 4 GiB. Its pages are committed when they are touched, and only the
    last MiB ever is: the staged span stays about 1 MiB while its start lies above 2^32."""
    a = np.zeros(HOST_BYTES, dtype=np.uint8)
    a[G + (1 << 20) :] = np.random.default_rng(1).integers(0, 256, 1 << 20, dtype=np.uint8)
    yield a
    del a


@functools.lru_cache(maxsize=None)
def host_case():
    frames = framegen.edge_batch(5, n_random=60)
    buf, off, ln = pack(frames, 4, seed=9)
    assert buf.size + 8192 < 1 << 20
    return buf, off.astype(np.uint64), ln.astype(np.uint32)


def put_host(host, buf):
    last = host[G + (1 << 20) :]
    last[:] = np.random.default_rng(1).integers(0, 256, 1 << 20, dtype=np.uint8)
    at = HOST_BASE - (G + (1 << 20))
    last[at : at + buf.size] = buf
    return last.copy(), at


@gpu
def test_host_digest_and_fill(eng, host):
    from seqs_amd import DIGEST_DTYPE, Engine, digest_host_multi

    buf, off, ln = host_case()
    n = ln.size
    before, at = put_host(host, buf)
    hi = off + np.uint64(HOST_BASE)
    assert int(hi.min()) > G and host.nbytes > G
    edig, est = coracle.digest_batch(buf, off, ln, 1514)
    dig, st = eng.digest_host(host, hi, ln, 1514)  # pageable arrays
    assert np.array_equal(dig, edig) and np.array_equal(st, est)
    # offsets, lengths and the results in pinned memory (the frames stay pageable: pinning 4 GiB is not cheap)
    po, pl = eng.host_empty(n, np.uint64), eng.host_empty(n, np.uint32)
    pd, ps = eng.host_empty(n, DIGEST_DTYPE), eng.host_empty(n, np.uint8)
    po[:], pl[:] = hi, ln
    eng.digest_host(host, po, pl, 1514, out=pd, status=ps)
    assert np.array_equal(pd, edig) and np.array_equal(ps, est)
    del po, pl, pd, ps
    # two contexts on the one GPU, each with its own block of the span
    e2 = Engine(0)
    try:
        dig, st = digest_host_multi([eng, e2], host, hi, ln, 1514)
        assert np.array_equal(dig, edig) and np.array_equal(st, est)
        perm = np.random.default_rng(2).permutation(n)  # unordered: the blocks go by buffer order
        dig, st = digest_host_multi([e2, eng], host, hi[perm], ln[perm], 1514)
        assert np.array_equal(dig, edig[perm]) and np.array_equal(st, est[perm])
    finally:
        e2.close()
    assert np.array_equal(host[G + (1 << 20) :], before), "a digest writes no frame byte"
    # the fill, in place: the untouched bytes of the last MiB come back as they were
    exp = before.copy()
    edig, est = coracle.fill_batch(exp, off + np.uint64(at), ln, 0, 3)
    dig, st = eng.fill_host(host, hi, ln, 0, 3)
    assert np.array_equal(dig, edig) and np.array_equal(st, est)
    diff = np.flatnonzero(host[G + (1 << 20) :] != exp)
    assert diff.size == 0, f"{diff.size} bytes of the last MiB differ, first at {int(diff[0])}"
    assert not host[G - 4096 : G + 4096].any()


@gpu
def test_host_coalesce_and_segment(eng, host):
    import test_gpu_coalesce as tc
    import test_gpu_flows as tf

    frames = tf.small_batch(257, 28, 257, reject=0.1) + tf.two_flows()
    buf, off, ln = cref.pack(frames, lead=2)
    before, at = put_host(host, buf)
    hi = off + np.uint64(HOST_BASE)
    assert int(hi.min()) > G
    room = int(ln.sum())
    noise = np.random.default_rng(61).integers(0, 256, room + tc.TAIL, dtype=np.uint8)
    e = cref.expected(buf, off, ln, 0, 0, noise, 0, room)
    mine = noise.copy()
    _, runs, run_of, totals, dig, st = eng.coalesce_host(host, hi, ln, payload=mine[:room])
    assert np.array_equal(mine, e["payload"]) and runs.tobytes() == e["runs"].tobytes()
    assert np.array_equal(run_of, e["run_of"]) and np.array_equal(dig, e["dig"]) and np.array_equal(st, e["st"])
    assert (int(totals["payload_bytes"]), int(totals["n_runs"])) == (e["payload_bytes"], e["n_runs"])
    e = fref.expected(buf, off, ln, 0, 0, noise, 0, room)
    mine = noise.copy()
    _, runs, flows, order, run_of, t, dig, st = eng.coalesce_flows_host(host, hi, ln, payload=mine[:room])
    assert np.array_equal(mine, e["payload"]) and runs.tobytes() == e["runs"].tobytes()
    assert flows.tobytes() == e["flows"].tobytes() and np.array_equal(order, e["order"])
    assert np.array_equal(run_of, e["run_of"]) and np.array_equal(dig, e["dig"]) and np.array_equal(st, e["st"])
    assert (int(t["payload_bytes"]), int(t["n_runs"]), int(t["n_flows"]), int(t["n_accepted"])) == \
        (e["payload_bytes"], e["n_runs"], e["n_flows"], e["n_accepted"])
    # the TX build reading its payload from above 2^32 into a small frames array
    from seqs_amd import segment_layout

    case = tx_case()
    before, at = put_host(host, case.buf)
    sends = sref.make_sends(case.specs)
    _, nbytes = segment_layout(sends, FCS, 4)
    fnoise = np.random.default_rng(4).integers(0, 256, nbytes + 64, dtype=np.uint8)
    ebuf, eoff, eln, edig, est = sref.expected(case.specs, case.buf, 0, FCS, 4, fnoise)
    sends["payload_off"] += np.uint64(HOST_BASE)
    assert int(sends["payload_off"].min()) > G
    out = fnoise.copy()
    _, o, l, dig, st = eng.segment_host(sends, host, 0, FCS, 4, frames=out)
    assert np.array_equal(out, ebuf) and np.array_equal(o, eoff) and np.array_equal(l, eln)
    assert np.array_equal(dig, edig) and np.array_equal(st, est)
    assert np.array_equal(host[G + (1 << 20) :], before)


@gpu
def test_host_calls_reject_a_frame_past_the_buffer(eng, host):
    """One frame ending one byte past frames_bytes, above 2^32: FS_E_INVALID from every host-staged call
    (and from the TX build for a payload range ending one byte past payload_bytes)."""
    from seqs_amd import Engine, FramesumError, digest_host_multi

    buf, off, ln = host_case()
    put_host(host, buf)
    hi = off + np.uint64(HOST_BASE)
    k = int(np.argmax(ln))
    ok = hi.copy()
    ok[k] = HOST_BYTES - int(ln[k]) - 4  # the frame and its FCS room end with the buffer: accepted
    eng.digest_host(host, ok, ln)
    eng.fill_host(host, ok, ln, 0, 3)
    bad = hi.copy()
    bad[k] = HOST_BYTES - int(ln[k]) + 1
    e2 = Engine(0)
    try:
        for call in (lambda: eng.digest_host(host, bad, ln), lambda: eng.fill_host(host, bad, ln, 0, 1),
                     lambda: eng.coalesce_host(host, bad, ln), lambda: eng.coalesce_flows_host(host, bad, ln),
                     lambda: digest_host_multi([eng, e2], host, bad, ln)):
            with pytest.raises(FramesumError, match=r"\(-1\)"):
                call()
        fcs_bad = ok.copy()
        fcs_bad[k] += 1  # the frame fits, its FCS does not
        with pytest.raises(FramesumError, match=r"\(-1\)"):
            eng.fill_host(host, fcs_bad, ln, 0, 3)
    finally:
        e2.close()
    sends = sref.make_sends([(sref.tcp_header(np.random.default_rng(1)), HOST_BYTES - 999, 1000, 100)])
    with pytest.raises(FramesumError, match=r"\(-1\)"):
        eng.segment_host(sends, host, 0, 0, 4)
    sends["payload_off"] -= np.uint64(1)
    eng.segment_host(sends, host, 0, 0, 4)
