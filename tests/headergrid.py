"""Header-geometry grids for the parity suites (test infrastructure, no tests here).

Every kernel shares one header parse (parse_frame / parse_tile in seqs_amd/csrc/framesum_kernel.hip),
instantiated with four header-slot geometries whose paths depend on where the headers fall: the IHL,
the TCP data offset, the frame's start offset and length, and what else stands in the 16-frame tile.
The builders here walk those dimensions systematically:

  valid_grid()   accepted frames: IHL 5..15 x {UDP, TCP data offset 5..15} x payload x padding
  cut_series()   every truncation of a base frame per IHL, TotalLength kept / following the cut
  gate_series()  both sides of every RecvEth gate (stacks/portstack.go:163-308) per IHL, each case
                 labelled with the verdict its construction intends
  mtu_cases()    the MTU values that sit on a length boundary of a series
  place()        frames at chosen start offsets modulo 128, non-zero noise everywhere else
  in_tiles()     batch orders that put every case at every tile position in five tile contexts
  Table          the distinct frames of a suite and their C-oracle digests, computed once per MTU
  context_cases()  which cases of the cut and gate series run in which tile context

Frames are built with framegen.valid_frame and refilled with oracle/pyref.py; a digest depends only on
the frame's bytes, so the expected words are computed per distinct frame and reused for every placement.
"""
from __future__ import annotations

import collections
import functools
import random
import struct

import numpy as np

import framegen
from oracle import pyref

Case = collections.namedtuple("Case", "label frame intent")  # label = (series, ihl, kind, ...); intent: verdict or None

IHLS = tuple(range(5, 16))
KINDS = ("udp",) + tuple(f"tcp{d}" for d in range(5, 16))
CUT_KINDS = ("udp", "tcp5", "tcp8", "tcp15")
GATE_KINDS = ("udp", "tcp5", "tcp15")
GRID_PAYLOADS = (0, 1, 2, 3, 5, 70, 1400)
GRID_PADS = (0, 1, 3, 50)
GATE_SIZES = (("small", 5, 0), ("large", 1400, 50))
START_PAYLOADS = (0, 3, 70)
START_PADS = (0, 3)
CONTEXTS = ("grid", "mtu_tile", "mixed_tile", "giant_tile", "partial_tile")  # (i) .. (v)
TAIL = 64        # noise behind the last frame of a placed batch
SHARE_FROM = 65536  # place(): a filler at least this long is stored once and listed at the same offset again


def proto_of(kind: str) -> int:
    return 17 if kind == "udp" else 6


def doff_of(kind: str) -> int:
    """TCP data offset in dwords (0 for UDP)."""
    return 0 if kind == "udp" else int(kind[3:])


def l4_header(kind: str) -> int:
    return 8 if kind == "udp" else 4 * doff_of(kind)


def base_frame(rnd, ihl: int, kind: str, payload: int, pad: int = 0, corrupt: bool = False) -> bytes:
    return framegen.valid_frame(rnd, proto_of(kind), payload=payload, ip_opts=ihl - 5,
                                tcp_opts=max(0, doff_of(kind) - 5), pad=pad, corrupt=corrupt)


def refill(f: bytearray) -> bytearray:
    """Store the L4 checksum RecvEth computes, when the frame reaches the compare (neither checksum
    sums the stored field: eth/headers.go:382-393, :510-527)."""
    v, _, got = pyref.recv_eth(bytes(f))
    if v in (pyref.FS_OK, pyref.FS_ERR_CHECKSUM):
        pos = 14 + 4 * (f[14] & 0xF) + (16 if f[23] == 6 else 6)
        struct.pack_into(">H", f, pos, got)
    return f


def _set_tl(f: bytearray, tl: int) -> bytearray:
    struct.pack_into(">H", f, 16, tl & 0xFFFF)
    return f


# ---- the three series ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def valid_grid() -> tuple:
    """IHL x kind x payload x padding, one case in eight with a corrupted stored checksum (verdict 13),
    and one zero-sum frame per protocol. Labels: ("valid", ihl, kind, payload, pad)."""
    rnd = random.Random(0x9a1d)
    out = []
    for ihl in IHLS:
        for kind in KINDS:
            for payload in GRID_PAYLOADS:
                for pad in GRID_PADS:
                    bad = len(out) % 8 == 3
                    out.append(Case(("valid", ihl, kind, payload, pad), base_frame(rnd, ihl, kind, payload, pad, bad),
                                    pyref.FS_ERR_CHECKSUM if bad else pyref.FS_OK))
    out.append(Case(("valid", 5, "tcp5", "zero_sum", 0), framegen.zero_sum_frame(rnd, 6), pyref.FS_OK))
    out.append(Case(("valid", 5, "udp", "zero_sum", 0), framegen.zero_sum_frame(rnd, 17), pyref.FS_OK))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cut_series() -> tuple:
    """Per IHL and kind, a base frame with a 5-byte payload cut to every length L: (a) TotalLength as it
    was, (b) TotalLength L - 14 and the L4 checksum refilled where RecvEth reaches the compare, (c)
    TotalLength L - 13, one byte past the frame. Labels: ("cut_a" | "cut_b" | "cut_c", ihl, kind, L)."""
    rnd = random.Random(0xc075)
    out = []
    for ihl in IHLS:
        for kind in CUT_KINDS:
            base = base_frame(rnd, ihl, kind, 5)
            for L in range(len(base) + 1):
                out.append(Case(("cut_a", ihl, kind, L), base[:L], None))
                if L >= 34:
                    out.append(Case(("cut_b", ihl, kind, L), bytes(refill(_set_tl(bytearray(base[:L]), L - 14))), None))
                    out.append(Case(("cut_c", ihl, kind, L), bytes(_set_tl(bytearray(base[:L]), L - 13)), None))
    return tuple(out)


def _gates(base: bytes, ihl: int, kind: str, size: str, payload: int) -> list:
    """Both sides of every gate for one base frame. The intended verdict comes from the construction
    (which gate the edit trips first in stacks/portstack.go:163-308), never from running a reference."""
    V = pyref
    out = []
    off, d, l4h = 14 + 4 * ihl, doff_of(kind), l4_header(kind)
    l4len = l4h + payload

    def add(name, f, intent, fill=False):
        f = bytearray(f)
        out.append(Case(("gate", ihl, kind, size, name), bytes(refill(f) if fill else f), intent))

    def edit(pos, val):
        f = bytearray(base)
        f[pos : pos + len(val)] = val
        return f

    add("base", base, V.FS_OK)
    add("etype_0806", edit(12, b"\x08\x06"), V.FS_ARP)
    add("etype_86dd", edit(12, b"\x86\xdd"), V.FS_IGNORED_NOT_IPV4)
    add("etype_0801", edit(12, b"\x08\x01"), V.FS_IGNORED_NOT_IPV4)
    add("arp_41", edit(12, b"\x08\x06")[:41], V.FS_ERR_PACKET_SMOL)
    add("arp_42", edit(12, b"\x08\x06")[:42], V.FS_ARP)
    add("version_5", edit(14, bytes([0x50 | ihl])), V.FS_ERR_IP_VERSION)
    for nib in range(5):
        add(f"ihl_nibble_{nib}", edit(14, bytes([0x40 | nib])), V.FS_ERR_INVALID_IHL)
    add("tl_ihl_minus_1", _set_tl(bytearray(base), 4 * ihl - 1), V.FS_ERR_BAD_IP_TOTAL_LEN_OR_IHL)
    add("tl_ihl", _set_tl(bytearray(base), 4 * ihl), V.FS_ERR_TOO_SHORT_TCP_OR_UDP)
    if kind == "udp":
        add("tl_l4_7", _set_tl(bytearray(base), 4 * ihl + 7), V.FS_ERR_TOO_SHORT_TCP_OR_UDP)
        add("tl_l4_8", _set_tl(bytearray(base), 4 * ihl + 8), V.FS_OK, fill=True)
    else:
        add("tl_l4_19", _set_tl(bytearray(base), 4 * ihl + 19), V.FS_ERR_TOO_SHORT_TCP_OR_UDP)
        add("tl_l4_20", _set_tl(bytearray(base), 4 * ihl + 20), V.FS_OK if d == 5 else V.FS_ERR_BAD_TCP_OFFSET, fill=True)
    add("tl_65522", _set_tl(bytearray(base), 65522), V.FS_ERR_BAD_IP_TOTAL_LEN_OR_IHL)  # end wraps to 0
    add("tl_65535", _set_tl(bytearray(base), 65535), V.FS_ERR_BAD_IP_TOTAL_LEN_OR_IHL)  # end wraps to 13
    add("proto_1", edit(23, b"\x01"), V.FS_ERR_UNKNOWN_IP_PROTO)
    if kind == "udp":  # read as TCP: 13 bytes are too short; the long one gets a data offset of 5
        f = edit(23, b"\x06")
        if l4len >= 20:
            f[off + 12] = 0x50 | (f[off + 12] & 0xF)
        add("proto_other", f, V.FS_OK if l4len >= 20 else V.FS_ERR_TOO_SHORT_TCP_OR_UDP, fill=True)
    else:  # read as UDP: its length field is the upper half of Seq, made >= 8 here
        f = edit(23, b"\x11")
        f[off + 4] |= 0x80
        add("proto_other", f, V.FS_OK, fill=True)
    add("sport_0", edit(off, b"\0\0"), V.FS_ERR_ZERO_PORT)
    add("dport_0", edit(off + 2, b"\0\0"), V.FS_ERR_ZERO_PORT)
    add("ports_0", edit(off, b"\0\0\0\0"), V.FS_ERR_ZERO_PORT)
    stored = off + (6 if kind == "udp" else 16)
    add("csum_bad", edit(stored, bytes([base[stored] ^ 0x04])), V.FS_ERR_CHECKSUM)
    if kind == "udp":
        add("ulen_7", edit(off + 4, b"\x00\x07"), V.FS_ERR_BAD_UDP_LENGTH)
        add("ulen_8", edit(off + 4, b"\x00\x08"), V.FS_OK, fill=True)  # differs from l4len: accepted, enters the sum
        add("ulen_l4len_plus_1", edit(off + 4, struct.pack(">H", l4len + 1)), V.FS_OK, fill=True)
    else:
        add("doff_4", edit(off + 12, bytes([0x40 | (base[off + 12] & 0xF)])), V.FS_ERR_BAD_TCP_OFFSET)
        add("doff_eq_l4len", _set_tl(bytearray(base), 4 * ihl + 4 * d), V.FS_OK, fill=True)
        add("doff_eq_l4len_plus_4", _set_tl(bytearray(base), 4 * ihl + 4 * d - 4),
            V.FS_ERR_TOO_SHORT_TCP_OR_UDP if d == 5 else V.FS_ERR_BAD_TCP_OFFSET)
    return out


@functools.lru_cache(maxsize=None)
def gate_series() -> tuple:
    """Labels: ("gate", ihl, kind, "small" | "large", gate name); `intent` is the intended verdict."""
    rnd = random.Random(0x6a7e)
    out = []
    for ihl in IHLS:
        for kind in GATE_KINDS:
            for size, payload, pad in GATE_SIZES:
                out += _gates(base_frame(rnd, ihl, kind, payload, pad), ihl, kind, size, payload)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def start_cases() -> tuple:
    """(case, start): every start offset 0..127 x IHL x {udp, tcp5, tcp15} x payload {0, 3, 70} x padding
    {0, 3}, the frames taken from valid_grid()."""
    by = {c.label: c for c in valid_grid()}
    out = []
    for ihl in IHLS:
        for kind in GATE_KINDS:
            for payload in START_PAYLOADS:
                for pad in START_PADS:
                    c = by[("valid", ihl, kind, payload, pad)]
                    out += [(c, s) for s in range(128)]
    random.Random(0x57a7).shuffle(out)  # tiles of unrelated IHLs (header_dma's ballot sees a mix)
    return tuple(out)


def grid_at_every_alignment():
    """(case, start): valid_grid() four times over, case k at starts k, k + 1, k + 2 and k + 3 modulo 128,
    so that every case of the grid (the 1,400-byte ones and those with 1 and 50 bytes of padding, which
    start_cases() leaves out) meets every start alignment S & 3."""
    v = valid_grid()
    return tuple((c, (k + r) % 128) for r in range(4) for k, c in enumerate(v))


def mtu_cases(cases, trailer: int = 0) -> list:
    """The MTU values m at which some frame has len - trailer == m and some frame len - trailer == m + 1
    (`trailer` = 4 for wire frames that carry their FCS)."""
    lens = {len(c.frame) - trailer for c in cases}
    return sorted(m for m in lens if m >= 0 and m + 1 in lens)


# ---- placement -------------------------------------------------------------------------------------

def place(frames, starts, room: int = 0, seed: int = 0):
    """Frame i at the first free offset congruent to starts[i] modulo 128, `room` spare bytes behind each,
    every byte outside the frames non-zero noise (an over-read that reaches a sum shows). A filler of
    SHARE_FROM bytes or more that was placed before is listed at its first offset again. Returns
    (buf, offsets int64, lengths int32)."""
    n = len(frames)
    off = np.zeros(n, dtype=np.int64)
    shared, at = {}, 0
    for i, (f, s) in enumerate(zip(frames, starts)):
        if len(f) >= SHARE_FROM and id(f) in shared:
            off[i] = shared[id(f)]
            continue
        o = at + ((int(s) - at) % 128)
        off[i] = o
        at = o + len(f) + room
        if len(f) >= SHARE_FROM:
            shared[id(f)] = o
    buf = np.random.default_rng(seed).integers(1, 256, at + TAIL, dtype=np.uint8)
    done = set()
    for f, o in zip(frames, off):
        if f and int(o) not in done:
            buf[o : o + len(f)] = np.frombuffer(f, dtype=np.uint8)
            if len(f) >= SHARE_FROM:
                done.add(int(o))
    return buf, off, np.array([len(f) for f in frames], dtype=np.int32)


# ---- tile contexts ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fillers() -> dict:
    rnd = random.Random(0xf111)
    return {
        1500: tuple(framegen.valid_frame(rnd, p, payload=1500 - 34 - h) for p, h in ((6, 20), (17, 8), (6, 20), (17, 8))),
        64: tuple(framegen.valid_frame(rnd, p, payload=64 - 34 - h) for p, h in ((6, 20), (17, 8), (17, 8))),
        9000: (framegen.valid_frame(rnd, 6, payload=9000 - 54),),
        131072: (bytes(rnd.randbytes(131072)),),
    }


Entry = collections.namedtuple("Entry", "src frame slot")  # src: index in `frames` or -1 (filler); slot: its place in memory


def in_tiles(frames, context: str, rotations=range(16)) -> list:
    """Batch orders that give the tiles of 16 frames the `context`; one order per rotation r, so that
    over r = 0..15 every frame visits every tile position. Each order is a list of Entry: `src` is the
    frame's index in `frames`, or -1 for a filler; `slot` names the entry's place in memory, the same in
    every rotation, so that one buffer serves them all and a rotation only permutes the offsets.

      grid          only the given frames
      mtu_tile      one of them per tile among 1,500-byte valid frames
      mixed_tile    one of them and one 9,000-byte frame among 64-byte frames
      giant_tile    one 131,072-byte random frame, one of them and 64-byte frames
      partial_tile  the given frames, then a last tile of 1..15 of them
    """
    F = fillers()
    n = len(frames)
    assert n > 0 and context in CONTEXTS
    out = []
    for r in rotations:
        if context in ("grid", "partial_tile"):
            m = -(-n // 16) * 16
            src = [k % n for k in range(m)]  # a multiple of 16: a rotation by r moves every frame r positions
            src = src[m - r :] + src[: m - r]
            if context == "partial_tile":
                src += [k % n for k in range(r % 15 + 1)]
            out.append([Entry(k, frames[k], ("g", k)) for k in src])
            continue
        order = []
        for t in range(n):
            p = (t + r) % 16
            if context == "mtu_tile":
                tile = [Entry(-1, F[1500][(t + k) % 4], ("f", t, k)) for k in range(16)]
            else:
                tile = [Entry(-1, F[64][(t + k) % 3], ("f", t, k)) for k in range(16)]
                big = F[9000][0] if context == "mixed_tile" else F[131072][0]
                tile[(p + 5 + t // 16 % 7) % 16] = Entry(-1, big, ("b", t))
            tile[p] = Entry(t, frames[t], ("g", t))
            order += tile
        out.append(order)
    return out


def lay_out(orders, starts_mod: int = 64, room: int = 0, seed: int = 0):
    """One buffer for all the orders of in_tiles(): every slot placed once (in the order the slots first
    appear, the k-th at a start congruent to k modulo `starts_mod`), and per order the (offsets, lengths,
    src) arrays in batch order. Returns (buf, [(off, ln, src, entries), ...])."""
    slots, frames = {}, []
    for order in orders:
        for e in order:
            if e.slot not in slots:
                slots[e.slot] = len(frames)
                frames.append(e.frame)
    buf, off, ln = place(frames, [k % starts_mod for k in range(len(frames))], room, seed)
    out = []
    for order in orders:
        at = np.array([slots[e.slot] for e in order], dtype=np.int64)
        out.append((off[at], ln[at], np.array([e.src for e in order], dtype=np.int64), order))
    return buf, out


# ---- expected digests, once per distinct frame -------------------------------------------------------

class Table:
    """The distinct frames of a suite and their C-oracle digests: expected(mtu) runs the oracle once
    over the distinct frames, and every placed batch indexes the result with ids()."""

    def __init__(self, fcs: bool = False):
        self.fcs = fcs
        self.frames, self.index, self._packed, self._cache = [], {}, None, {}

    def ids(self, frames) -> np.ndarray:
        out = np.zeros(len(frames), dtype=np.int64)
        for i, f in enumerate(frames):
            k = self.index.get(f)
            if k is None:
                k = self.index[f] = len(self.frames)
                self.frames.append(f)
                self._packed, self._cache = None, {}
            out[i] = k
        return out

    def expected(self, mtu: int = 0):
        """(crc32, ip_csum, l4_csum, verdict) arrays over the distinct frames."""
        from oracle import coracle
        from seqs_amd import pack_frames

        if mtu not in self._cache:
            if self._packed is None:
                self._packed = pack_frames(self.frames, align=1)
            buf, off, ln = self._packed
            call = coracle.digest_fcs_batch if self.fcs else coracle.digest_batch
            dig, st = call(buf, off, ln, mtu=mtu, nthreads=8)
            self._cache[mtu] = (dig["crc32"].astype(np.uint32), dig["ip_csum"].astype(np.uint32),
                                dig["l4_csum"].astype(np.uint32), st)
        return self._cache[mtu]


def boundary_subset(cases, verdicts) -> list:
    """Indices of the cases that stand at a boundary: every gate case, and of a cut series (per IHL and
    kind, in order of L) the first, the last and both neighbours of every change of verdict."""
    keep, groups = [], collections.OrderedDict()
    for i, c in enumerate(cases):
        if c.label[0].startswith("cut_"):
            groups.setdefault(c.label[:3], []).append(i)
        else:
            keep.append(i)
    for idx in groups.values():
        for k, i in enumerate(idx):
            edge = k == 0 or k == len(idx) - 1
            if not edge:
                edge = verdicts[i] != verdicts[idx[k - 1]] or verdicts[i] != verdicts[idx[k + 1]]
            if edge:
                keep.append(i)
    return sorted(keep)


def one_per_label(cases, verdicts) -> list:
    """One case per (series, ihl, kind): the verdicts taken in turn, so that the few cases differ."""
    groups = collections.OrderedDict()
    for i, c in enumerate(cases):
        groups.setdefault(c.label[:3], []).append(i)
    keep = []
    for g, idx in enumerate(groups.values()):
        kinds = sorted({int(verdicts[i]) for i in idx})
        want = kinds[g % len(kinds)]
        keep.append(next(i for i in idx if verdicts[i] == want))
    return keep


# ---- which cases run in which tile context -----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def series_cases() -> tuple:
    return cut_series() + gate_series()


@functools.lru_cache(maxsize=None)
def series_verdicts() -> np.ndarray:
    t = Table()
    ids = t.ids([c.frame for c in series_cases()])
    return t.expected(0)[3][ids]


@functools.lru_cache(maxsize=None)
def context_cases(context: str) -> tuple:
    """The cases of the cut and gate series a tile context runs: all of them where the tiles hold nothing
    else; the boundary subset (without the 1,500-byte gate frames, whose tile is an MTU tile already)
    among fillers; one per (series, IHL, kind) in the few giant tiles. Every (series, IHL, kind) is in
    every context."""
    cg = series_cases()
    if context in ("grid", "partial_tile"):
        return cg
    if context == "giant_tile":
        return tuple(cg[i] for i in one_per_label(cg, series_verdicts()))
    keep = [i for i in boundary_subset(cg, series_verdicts()) if cg[i].label[0] != "gate" or cg[i].label[3] != "large"]
    return tuple(cg[i] for i in keep)
