"""Checksum sums at saturating bytes and under 128-512 KiB of Ethernet padding.

A 32-bit one's-complement accumulator that wraps moves the L4 checksum by one (2^32 = 1 mod
65535): a valid frame gets verdict 13 and the TX fill writes a wrong checksum. The sums that can get
that large are the sum of the Ethernet padding [end, len) that the parse subtracts, and the
small-frame kernel's single lane over a long frame; both take a padding of 128 KiB or more, or
random padding of 256 KiB or more, which no other test has below the 512-KiB recompute. Here:

  A1  valid TCP / UDP frames followed by 2,001 B .. 512 KiB - 1 of padding (random, all-0xFF,
      all-zero), each in a tile of 15 short frames, at every start alignment;
  A2  saturating (all-0xFF) and all-zero L4 payloads at ordinary sizes up to the longest IP
      datagram, and frames whose computed checksum is 0x0000;

through the RX digest (device and host-staged), the TX fill and the FCS verify, in every kernel
column, bit for bit against the C oracle. The module first proves on the CPU (numpy, uint64) that
the cases it calls wrapping do exceed 2^32 and that the ones just below do not, so the cases cannot
quietly stop testing what they are here for.

With the 32-bit padding sum and the unfolded one-lane loop these tests were written against, the
4-lane columns (one_pass, mixed, segments, auto, and the host-staged path) got the L4 checksum and
verdict of exactly the ten giants whose padding sum reaches 2^32 wrong, in all three ops. The
small-frame kernel got those right -- its one lane wrapped as often as the padding sum it then
subtracted -- and instead missed the two where the counts differ (rand262000, ff131000).
"""
import functools
import random

import numpy as np
import pytest

import engines
import framegen
from oracle import coracle
from seqs_amd import FCS_APPEND, FILL_CSUM, FS_ERR_FCS
from test_tx_fcs import check_fill, gpu_fcs, stale, words

M32 = 1 << 32
MAXLEN = (1 << 19) - 1  # the longest frame whose streamed sum the finish still uses
ERR_MTU = 2


class Batch:
    """Frames packed at byte granularity (random gaps of 0..3 B on top of the 4 spare bytes after
    every frame for the FCS, so every start alignment occurs; `want_sa` pins some)."""

    def __init__(self, frames, names, want_sa=None, seed=0):
        self.frames, self.names = frames, names
        rng = np.random.default_rng(seed)
        off, o = [], 0
        for i, f in enumerate(frames):
            o += int(rng.integers(0, 4))
            if want_sa and i in want_sa:
                o += (want_sa[i] - o) & 3
            off.append(o)
            o += len(f) + 4
        self.off = np.array(off, dtype=np.int64)
        self.ln = np.array([len(f) for f in frames], dtype=np.int32)
        self.noise = rng.integers(0, 256, o + 16, dtype=np.uint8)
        self.buf = self.place(frames)
        self.giants = [i for i, n in enumerate(names) if n != "short"]

    def place(self, frames):
        buf = self.noise.copy()
        for f, o in zip(frames, self.off):
            buf[o : o + len(f)] = np.frombuffer(f, dtype=np.uint8)
        return buf

    def half_sum(self, i, p0, p1):
        """Exact sum of frame i's bytes [p0, p1) as the kernels weigh them: the 16-bit halves of the
        buffer's dwords, i.e. a byte at absolute address a weighs 256^(a & 1)."""
        a0 = int(self.off[i]) + p0
        b = self.buf[a0 : int(self.off[i]) + p1].astype(np.uint64)
        return int(b[a0 & 1 :: 2].sum()) + 256 * int(b[1 - (a0 & 1) :: 2].sum())

    def l4_end(self, i):
        return 14 + int.from_bytes(self.frames[i][16:18], "big")


def _shorts(rnd, k):
    # 64-B and 1500-B valid frames, TCP and UDP in turn
    out = []
    for j in range(k):
        proto = (6, 17)[(j >> 1) & 1]
        out.append(framegen.valid_frame(rnd, proto, payload=(64 if j & 1 else 1500) - (54 if proto == 6 else 42)))
    return out


# (padding length, content): MAX = the padding that makes the frame 524,287 B long
MAX = -1
A1_PADS = [(n, "rand") for n in (2001, 65536, 131000, 131100, 200000, 262000, 300000, 400000, 500000, MAX)] + [
    (131000, "ff"), (131100, "ff"), (400000, "ff"), (MAX, "ff"), (MAX, "ff"), (MAX, "ff"), (MAX, "ff"), (300000, "zero")]
# what the exact sums must say of them: the padding sum reaches 2^32 (every kernel subtracts it) /
# the whole frame's sum does (the small-frame kernel's one lane adds all of it)
PAD_WRAPS = {"rand300000", "rand400000", "rand500000", "randmax", "ff131100", "ff400000", "ffmax"}
PAD_BELOW = {"rand2001", "rand65536", "rand131000", "rand131100", "rand200000", "ff131000", "zero300000"}
FRAME_WRAPS = PAD_WRAPS | {"ff131000"}
FRAME_BELOW = PAD_BELOW - {"ff131000"}


@functools.lru_cache(maxsize=None)
def a1_batch():
    rnd = random.Random(41)
    combos = [(p, n) for n in (0, 1000, 1446) for p in (6, 17)]
    frames, names, want = [], [], {}
    ffmax_seen = 0
    for t, (padlen, kind) in enumerate(A1_PADS):
        proto, payload = combos[t % len(combos)]
        base = framegen.valid_frame(rnd, proto, payload=payload)
        n = MAXLEN - len(base) if padlen == MAX else padlen
        pad = {"rand": rnd.randbytes(n), "ff": b"\xff" * n, "zero": bytes(n)}[kind]
        tile = _shorts(rnd, 15)
        tile.insert((5 * t) % 16, base + pad)  # the giant's group differs from tile to tile
        if padlen == MAX and kind == "ff":  # one 524,287-B frame at each start alignment
            want[len(frames) + (5 * t) % 16] = ffmax_seen
            ffmax_seen += 1
        for j, f in enumerate(tile):
            names.append(f"{kind}{'max' if padlen == MAX else padlen}" if j == (5 * t) % 16 else "short")
        frames += tile
    return Batch(frames, names, want, seed=42)


@functools.lru_cache(maxsize=None)
def a2_batch():
    rnd = random.Random(43)
    frames, names = [], []

    def add(name, f):
        frames.append(f)
        names.append(name)
        for s in _shorts(rnd, 3):  # 4 of these and 12 short frames per tile
            frames.append(s)
            names.append("short")

    for proto, hdr in ((6, 54), (17, 42)):
        for fill, tag in ((b"\xff", "ff"), (b"\0", "zero")):
            for L in (60, 1500, 1514, 9000, 767, 769, 4607, 4609, 9215, 9217):
                add(f"{tag}/{proto}/len{L}", framegen.valid_frame(rnd, proto, payload_bytes=fill * (L - hdr)))
            # IP total lengths: the largest RecvEth accepts (14 + 65,521 = 65,535: its frame end is a
            # uint16) and the two largest the field allows (the end wraps; rejected, digests compared)
            for tl in (65521, 65534, 65535):
                add(f"{tag}/{proto}/tl{tl}", framegen.valid_frame(rnd, proto, payload_bytes=fill * (tl + 14 - hdr)))
        for L in (9000, 60000):
            add(f"zerosum/{proto}/len{L}", framegen.zero_sum_frame(rnd, proto, payload=L - hdr))
    return Batch(frames, names, seed=44)


BATCHES = {"a1": a1_batch, "a2": a2_batch}


# ---------------------------------------------------------------- CPU: the cases are what they claim


def test_a1_cases_wrap_where_named():
    b = a1_batch()
    assert len(b.giants) == len(A1_PADS) and set(b.names) == PAD_WRAPS | PAD_BELOW | {"rand262000", "short"}
    for i in b.giants:
        name, ln, end = b.names[i], int(b.ln[i]), b.l4_end(i)
        pad, whole = b.half_sum(i, end, ln), b.half_sum(i, 0, ln)
        assert ln - end in (2001, 65536, 131000, 131100, 200000, 262000, 300000, 400000, 500000) or ln == MAXLEN
        if name in PAD_WRAPS:
            assert pad >= M32, name
        if name in PAD_BELOW:
            assert pad < M32, name
        if name in FRAME_WRAPS:
            assert whole >= M32, name
        if name in FRAME_BELOW:
            assert whole < M32, name
    # the 524,287-B frames: every start alignment; a lane of the 4-lane kernels adds 2^15 + 1 dwords
    # of those at alignments 2 and 3
    ffmax = [i for i in b.giants if b.names[i] == "ffmax"]
    assert sorted(int(b.off[i]) & 3 for i in ffmax) == [0, 1, 2, 3] and all(int(b.ln[i]) == MAXLEN for i in ffmax)
    assert sorted(((int(b.off[i]) & 3) + MAXLEN + 3) >> 2 for i in ffmax) == [1 << 17, 1 << 17, (1 << 17) + 1, (1 << 17) + 1]
    assert {int(o) & 3 for o in b.off[b.giants]} == {0, 1, 2, 3}
    # every tile: one giant among fifteen 64-B and 1500-B frames
    for t in range(0, len(b.names), 16):
        lens = sorted(int(x) for x in b.ln[t : t + 16])
        assert lens[:15] == [64] * 7 + [1500] * 8 and lens[15] > 2000
    # the oracle takes every frame; with an MTU the giants are rejected for it
    _, st = coracle.digest_batch(b.buf, b.off, b.ln)
    assert (st == 0).all()
    _, st = coracle.digest_batch(b.buf, b.off, b.ln, mtu=1514)
    assert (st[b.giants] == ERR_MTU).all() and (np.delete(st, b.giants) == 0).all()


def test_a2_cases_saturate():
    b = a2_batch()
    _, st = coracle.digest_batch(b.buf, b.off, b.ln)
    dig, _ = coracle.digest_batch(b.buf, b.off, b.ln)
    for i in b.giants:
        name, f = b.names[i], b.frames[i]
        hdr = 54 if f[23] == 6 else 42
        if name.startswith("ff/"):
            assert set(f[hdr:]) <= {0xFF} and len(f) >= 60
        if name.startswith("zero/"):
            assert set(f[hdr:]) <= {0}
        if name.startswith("zerosum"):
            assert int(dig["l4_csum"][i]) == 0 and st[i] == 0
        # accepted unless 14 + total length leaves 16 bits
        assert st[i] == (7 if name.endswith(("tl65534", "tl65535")) else 0), name
    assert {int(o) & 3 for o in b.off[b.giants]} == {0, 1, 2, 3}
    assert int(b.ln.max()) == 14 + 65535


# ---------------------------------------------------------------- GPU parity


@pytest.fixture(scope="module", params=engines.VARIANTS, ids=engines.IDS)
def engine(request):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = engines.engine_for(request.param)
    yield e
    e.close()


def compare(b, gw, gst, edig, est, label):
    """Digest words and verdicts against the oracle's; the message names every case that differs."""
    ew = words(edig)
    bad = np.nonzero((gw != ew).any(axis=1) | (gst != est))[0]
    what = [f"{b.names[i]}[{i}] sa={int(b.off[i]) & 3} len={int(b.ln[i])} "
            f"gpu=({gw[i][0]:#010x},{gw[i][1] & 0xffff:#06x},{gw[i][1] >> 16:#06x},{gst[i]}) "
            f"oracle=({ew[i][0]:#010x},{ew[i][1] & 0xffff:#06x},{ew[i][1] >> 16:#06x},{est[i]})" for i in bad]
    print(f"{label}: {len(bad)} of {len(est)} differ" + "".join("\n  " + w for w in what))
    assert bad.size == 0, f"{label}: {len(bad)} differ: " + "; ".join(what[:24])


def gpu_digest(engine, buf, off, ln, mtu):
    import torch

    dev = torch.device("cuda:0")
    tb = torch.from_numpy(np.ascontiguousarray(buf)).to(dev)
    out, st = engine.digest_device(tb, torch.from_numpy(off).to(dev), torch.from_numpy(ln).to(dev), mtu=mtu)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(-1, 2), st.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("mtu", [0, 1514])
@pytest.mark.parametrize("which", ["a1", "a2"])
def test_gpu_digest_saturation(engine, which, mtu):
    b = BATCHES[which]()
    gw, gst = gpu_digest(engine, b.buf, b.off, b.ln, mtu)
    edig, est = coracle.digest_batch(b.buf, b.off, b.ln, mtu=mtu, nthreads=8)
    compare(b, gw, gst, edig, est, f"digest/{which}/mtu{mtu}")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["a1", "a2"])
def test_gpu_fill_saturation(engine, which):
    # the TX fill on copies with stale checksum fields: the frames as written (checksums, FCS),
    # digests and verdicts, byte for byte
    b = BATCHES[which]()
    buf = b.place(stale(b.frames, 45))
    check_fill(engine, (buf, b.off, b.ln), 0, FILL_CSUM | FCS_APPEND, f"fill/{which}")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["a1", "a2"])
def test_gpu_fcs_saturation(engine, which):
    # the wire frames the oracle's fill wrote (FCS appended), one FCS and one giant's body damaged
    b = BATCHES[which]()
    buf = b.place(stale(b.frames, 45))
    coracle.fill_batch(buf, b.off, b.ln, 0, FILL_CSUM | FCS_APPEND)
    hit_fcs = b.names.index("rand300000" if which == "a1" else "zero/17/len9000")
    hit_body = b.names.index("ff400000" if which == "a1" else "ff/6/tl65521")
    buf[int(b.off[hit_fcs]) + int(b.ln[hit_fcs]) + 2] ^= 0x08
    buf[int(b.off[hit_body]) + int(b.ln[hit_body]) // 2] ^= 0x40
    wl = b.ln + 4
    for mtu in (0, 1514):
        gw, gst = gpu_fcs(engine, buf, b.off, wl, mtu)
        edig, est = coracle.digest_fcs_batch(buf, b.off, wl, mtu)
        if mtu == 0:
            assert sorted(np.nonzero(est == FS_ERR_FCS)[0]) == sorted((hit_fcs, hit_body))
        compare(b, gw, gst, edig, est, f"fcs/{which}/mtu{mtu}")


@pytest.mark.gpu
def test_gpu_digest_host_saturation():
    # the host-staged path (automatic kernel choice) over the padded giants
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    b = a1_batch()
    e = engines.engine_for(0)
    try:
        dig, st = e.digest_host(b.buf, b.off.astype(np.uint64), b.ln.astype(np.uint32))
    finally:
        e.close()
    edig, est = coracle.digest_batch(b.buf, b.off, b.ln)
    compare(b, words(dig), st, edig, est, "digest_host/a1")
