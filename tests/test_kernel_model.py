"""CPU check of the kernel's arithmetic decomposition (tests/kernel_model.py mirrors
seqs_amd/csrc/framesum_kernel.hip): stream/lane-tree CRC-32 vs zlib, and the
native-domain one's-complement split vs the reference restatement."""
import random
import zlib

import kernel_model as km
import framegen
from oracle import pyref


def test_crc_decomposition_vs_zlib():
    rnd = random.Random(11)
    for _ in range(400):
        L = rnd.choice([0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1500, rnd.randrange(0, 4000)])
        pre = rnd.randrange(0, 13)
        buf = rnd.randbytes(pre + L + 8)
        assert km.crc32_model(buf, pre, L) == zlib.crc32(buf[pre : pre + L])


def test_final_step_equals_unshift():
    rnd = random.Random(4)
    for _ in range(200):
        w = rnd.getrandbits(32)
        for t in range(4):
            c = km.apply(km.ZFIN[t], w)
            # Z_(4-t)(W) shifted forward by t bytes is Z_4(W)
            assert km.zero_shift(c, t) == km.apply(km.Z4, w)


def test_tables_properties():
    # Z_a o Z_b = Z_(a+b) on random registers; the one-byte inverse undoes Z_1.
    rnd = random.Random(2)
    for _ in range(200):
        r = rnd.getrandbits(32)
        assert km.apply(km.Z4, km.apply(km.Z4, r)) == km.zero_shift(r, 8)
        assert km.apply(km.Z32, r) == km.apply(km.Z16, km.apply(km.Z16, r))
        assert km.apply(km.Z64, r) == km.zero_shift(r, 64)
        c = km.zero_shift(r, 1)
        j = km.INV[c >> 24]
        assert ((((c ^ km.T1[j]) << 8) & 0xFFFFFFFF) | j) == r
    assert sorted(km.INV) == list(range(256))


def test_l4_native_split_matches_reference():
    # For every frame the reference checksums, the kernel's split (streamed inside dwords +
    # partial bytes + exact pseudo/excluded-word corrections, folded in the native domain)
    # reproduces RecvEth's gotsum bit-exactly, including unaligned frame starts.
    import struct

    frames = framegen.edge_batch(7, n_random=120)
    rnd = random.Random(9)
    checked = 0
    for f in frames:
        v, ipc, got = pyref.recv_eth(f)
        if v not in (pyref.FS_OK, pyref.FS_ERR_CHECKSUM):
            continue
        pre = rnd.randrange(0, 8)
        buf = bytes(rnd.randbytes(pre)) + f + bytes(8)
        ihl = f[14] & 0xF
        l4s, l4e = 14 + 4 * ihl, 14 + struct.unpack(">H", f[16:18])[0]
        total, parity = km.l4_native_sum(buf, pre, len(f), l4s, l4e)
        assert total == km.native_sum(buf, pre, l4s, l4e)
        sa = pre & 3
        proto = f[23]
        skip0 = l4s + (16 if proto == 6 else 6)
        for p in range(skip0, skip0 + (4 if proto == 6 else 2)):
            total -= f[p] << (8 * ((sa + p) & 3))
        lenword = ((struct.unpack(">H", f[16:18])[0] - 4 * ihl) & 0xFFFF) if proto == 6 else struct.unpack(">H", f[l4s + 4 : l4s + 6])[0]
        words = [struct.unpack(">H", f[i : i + 2])[0] for i in (26, 28, 30, 32)] + [proto, lenword]
        for w in words:
            total += w if parity else ((w & 0xFF) << 8) | (w >> 8)
        assert total >= 0
        assert km.fold_native_to_be(total, parity) == got
        checked += 1
    assert checked > 100


def test_block_aligned_rows_vs_zlib():
    # digest_kernel_a<kOps, true>: rows on 64-B blocks, skipped updates past the frame end and
    # the rotated combine reproduce zlib at every block phase, length and start alignment
    rnd = random.Random(12)
    for _ in range(300):
        L = rnd.choice([4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, rnd.randrange(4, 1600)])
        pre = rnd.randrange(0, 70)
        buf = rnd.randbytes(pre + L + 8)
        assert km.crc32_model_al(buf, pre, L, rnd.randrange(16)) == zlib.crc32(buf[pre : pre + L])


def test_lane_per_frame_crc_vs_zlib():
    """The small-frame kernel's CRC (one lane per frame, one or two Horner chains) at every start
    alignment and the lengths round the dword and chain boundaries."""
    import random
    import zlib

    from kernel_model import crc32_model_lane

    rnd = random.Random(5)
    buf = bytes(rnd.randrange(256) for _ in range(400))
    for S in range(8):
        for length in list(range(0, 40)) + [47, 60, 64, 65, 127, 128, 129, 200]:
            want = zlib.crc32(buf[S:S + length])
            for chains in (1, 2):
                assert crc32_model_lane(buf, S, length, chains) == want, (S, length, chains)


def test_tile_segments_vs_zlib():
    """The segment kernel's decomposition (km.crc32_tile_segments): random tiles of mixed lengths
    (empty and sub-4-byte frames, gaps, every start alignment and block phase, 1 to 16 groups), the
    C3 tile (64/576/1500/9000 B), and a tile of 64-B frames beside a jumbo frame; and the tail select
    is needed (without it every frame of the C3 tile is wrong)."""
    rnd = random.Random(21)
    for _ in range(60):
        n = rnd.choice([1, 2, 3, 5, 16])
        lens = [rnd.choice([0, 1, 3, 4, 5, 7, 20, 63, 64, 65, 70, 130, 200, 577, 1000]) for _ in range(n)]
        buf = rnd.randbytes(sum(lens) + 4 * n + 64)
        frames, o = [], rnd.randrange(4)
        for ln in lens:
            frames.append((o, ln))
            o += ln + rnd.randrange(4)
        got = km.crc32_tile_segments(buf, frames, rnd.randrange(16), groups=rnd.choice([1, 2, 4, 16]))
        assert got == [zlib.crc32(buf[S:S + ln]) for S, ln in frames]
    buf = rnd.randbytes(50000)
    for lens in ([64, 576, 1500, 9000] * 4, [64] * 15 + [9000]):
        frames, o = [], 0
        for ln in lens:
            frames.append((o, ln))
            o += ln
        exp = [zlib.crc32(buf[S:S + ln]) for S, ln in frames]
        assert km.crc32_tile_segments(buf, frames, 3) == exp
    bad = km.crc32_tile_segments(buf, frames, 3, model_tail_select=False)
    assert sum(g != e for g, e in zip(bad, exp)) > 0


# ---------------------------------------------------------------------------------------
# The one's-complement sum's 32-bit accumulators (km.l4_checksum_model) at saturating bytes and
# long Ethernet paddings.

KERNELS = ("one_pass", "mixed", "segments", "small")


def _place(frame, sa, rnd):
    S = 4 + sa
    return bytes(rnd.randbytes(S)) + frame + bytes(rnd.randbytes(8)), S


def _saturation_patterns(rnd):
    """(name, frame, padding sum wraps 32 bits, whole frame wraps 32 bits in one lane)."""
    ff, z = b"\xff", b"\0"
    t = lambda k: framegen.valid_frame(rnd, 6, payload=1000) + k  # noqa: E731
    u = lambda k: framegen.valid_frame(rnd, 17, payload=1000) + k  # noqa: E731
    out = [
        ("rand2001", t(rnd.randbytes(2001)), False, False),
        ("rand200000", u(rnd.randbytes(200000)), False, False),
        ("rand300000", t(rnd.randbytes(300000)), True, True),
        ("zero300000", u(z * 300000), False, False),
        ("ff131000", t(ff * 131000), False, True),
        ("ff131100", u(ff * 131100), True, True),
        ("ff400000", t(ff * 400000), True, True),
    ]
    for proto, hdr in ((6, 54), (17, 42)):
        out.append((f"ffmax{proto}", framegen.valid_frame(rnd, proto, payload=1000) + ff * (524287 - hdr - 1000), True, True))
        # saturating and all-zero L4 payloads at ordinary sizes, the longest datagram RecvEth takes
        # (14 + total length = 65535) and a computed checksum of 0x0000
        for L in (60, 769, 1514, 9217, 65535):
            for fill in (ff, z):
                out.append((f"pay{fill[0]:02x}/{proto}/{L}", framegen.valid_frame(rnd, proto, payload_bytes=fill * (L - hdr)), False, False))
        out.append((f"zerosum{proto}", framegen.zero_sum_frame(rnd, proto, payload=9000 - hdr), False, False))
    return out


def test_checksum_accumulators_vs_reference():
    """The kernels' summation (4 lanes x 32 bits by row position, one lane for the small-frame
    kernel, segment cuts, the 64-bit padding sum, the folds and finish_l4) gives RecvEth's checksum
    on saturating and long-padded frames with no accumulator reaching 2^32; the summation as it was
    before the fix (32-bit padding sum, no fold in the small kernel's long-frame loop) does not."""
    rnd = random.Random(31)
    wrong_before = {k: [] for k in KERNELS}
    expect_4lane, expect_small = [], []
    for i, (name, frame, pad_wraps, lane_wraps) in enumerate(_saturation_patterns(rnd)):
        v, _, got = pyref.recv_eth(frame)
        assert v == pyref.FS_OK, name
        end = 14 + int.from_bytes(frame[16:18], "big")
        for sa in range(4) if name.startswith("ffmax") else ((i & 3),):
            buf, S = _place(frame, sa, rnd)
            pad_sum, frame_sum = km.half_sum(buf, S, end, len(frame)), int(km.sad_terms(buf, S, len(frame)).sum())
            assert (pad_sum >= km.M32) == pad_wraps and (frame_sum >= km.M32) == lane_wraps, name
            # 2^32 = 1 (mod 65535): a 32-bit padding sum that wrapped p times moves the checksum by p;
            # the small kernel's one lane wraps too, and only the difference of the two counts shows
            expect_4lane += [name] * (pad_sum >= km.M32)
            expect_small += [name] * (frame_sum >> 32 != pad_sum >> 32)
            rows = (15 + len(frame) // 4) // 16
            for kernel in KERNELS:
                ph = rnd.randrange(16)
                cuts = sorted(rnd.sample(range(1, rows), min(3, rows - 1))) if rows > 1 else ()
                l4, accs = km.l4_checksum_model(buf, S, len(frame), kernel, ph, cuts)
                assert l4 == got, (name, sa, kernel, ph)
                assert max(accs) < km.M32, (name, sa, kernel, ph)
                if km.l4_checksum_model(buf, S, len(frame), kernel, ph, cuts, fixed=False)[0] != got:
                    wrong_before[kernel].append(name)
    assert expect_4lane == ["rand300000", "ff131100", "ff400000"] + ["ffmax6"] * 4 + ["ffmax17"] * 4
    for kernel in KERNELS[:3]:
        assert wrong_before[kernel] == expect_4lane, kernel
    assert wrong_before["small"] == expect_small and "ff131000" in expect_small


def test_no_accumulator_wraps_below_the_recompute_gate():
    """All-0xFF frames of 524,200 .. 524,287 bytes (the longest finish_l4 does not recompute) at
    every start alignment and row phase: some lane adds 2^15 + 1 dwords (sa + len > 2^19), yet that
    lane holds the frame's first and last dword, which together hold at most 3 frame bytes, so no
    lane sum reaches 2^32; nor does the small-frame kernel's folded accumulator."""
    ff = b"\xff" * (524287 + 8)
    most = 0
    for length in range(524200, 524288):
        for sa in range(4):
            terms = km.sad_terms(ff, sa, length)
            nd = len(terms)
            assert nd == (sa + length + 3) // 4
            total = km.half_sum(ff, sa, 0, length)
            # every block phase for the last 16 lengths, else the two extreme phases and the
            # end-anchored layout (pos0 = -nd mod 16)
            for pos0 in range(16) if length >= 524272 else sorted({0, 15, -nd % 16}):
                (lanes,) = km.lane_sums(terms, pos0)
                assert max(lanes) < km.M32, (length, sa, pos0)
                assert sum(lanes) == total
                cnt = km.lane_dwords(nd, pos0)
                assert sum(cnt) == nd
                most = max(most, max(cnt))
                for c, v in zip(cnt, lanes):
                    if c > 1 << 15:
                        assert sa + length > 1 << 19 and v <= ((1 << 15) - 1) * 0x1FFFE + 0xFFFF + 0xFF00
    assert most == (1 << 15) + 1
    # one more byte and a saturated lane wraps: the gate cannot move up
    terms = km.sad_terms(ff, 0, 524288 + 4)
    assert max(km.lane_sums(terms, 0)[0]) >= km.M32
    for sa in range(4):
        terms = km.sad_terms(ff, sa, 524287)
        for xo in range(4):
            cs, peak = km.small_lane_sum(terms, xo)
            assert peak < km.M32 and cs % 65535 == km.half_sum(ff, sa, 0, 524287) % 65535
            assert km.small_lane_sum(terms, xo, fixed=False)[1] >= km.M32
