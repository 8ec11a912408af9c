"""The builders of tests/headergrid.py reach what they claim, and the references agree on every frame
they build, before any GPU is involved (CPU only). tests/test_gpu_header_grid.py runs the same batches
on every kernel."""
import collections

import numpy as np
import pytest

import headergrid as hg
from oracle import coracle, pyref
from test_go_gate_order import BROADCAST, Stack, recv_eth_reference

ERR = {"errPacketSmol": 1, "errPacketExceedsMTU": 2, "errIPVersion": 5, "errInvalidIHL": 6, "errBadIPTotalLenOrIHL": 7,
       "errUnknownIPProto": 8, "errTooShortTCPOrUDP": 9, "errZeroPort": 10, "errBadUDPLength": 11, "errBadTCPOffset": 12,
       "ErrChecksumTCPorUDP": 13}
BIG_MTU = 1 << 20


def go_verdict(f: bytes) -> int:
    """recv_eth_reference's outcome as a verdict: broadcast MAC, IP 0.0.0.0, both sockets open on the
    frame's port, a large MTU."""
    ps = Stack(BROADCAST, b"\0\0\0\0", 1, 1, False, BIG_MTU)
    o = recv_eth_reference(BROADCAST + f[6:] if len(f) >= 6 else f, ps)
    if o[0] == "err":
        return ERR[o[1]]
    if o[0] == "arp":
        return 4
    if o == ("nil", "etype"):
        return 3
    assert o[0] == "deliver", o
    return 0


@pytest.fixture(scope="module")
def series():
    return hg.valid_grid() + hg.cut_series() + hg.gate_series()


@pytest.fixture(scope="module")
def table(series):
    t = hg.Table()
    return t, t.ids([c.frame for c in series])


def test_series_sizes():
    v, c, g = hg.valid_grid(), hg.cut_series(), hg.gate_series()
    assert len(v) == 11 * 12 * 7 * 4 + 2 and max(len(x.frame) for x in v) == 14 + 60 + 60 + 1400 + 50
    assert len(c) == 8888 and max(len(x.frame) for x in c) == 139
    assert {x.label[:3] for x in c} == {(s, i, k) for s in ("cut_a", "cut_b", "cut_c") for i in hg.IHLS for k in hg.CUT_KINDS}
    assert {x.label[:4] for x in g} == {("gate", i, k, s) for i in hg.IHLS for k in hg.GATE_KINDS for s in ("small", "large")}
    assert len({x.label for x in v + c + g}) == len(v) + len(c) + len(g)  # every label names one case
    assert sum(x.intent == 13 for x in v) == len(v) // 8


def test_references_agree_on_every_frame(series, table):
    t, ids = table
    crc, ipc, l4c, st = t.expected(0)
    seen = set()
    for c, i in zip(series, ids):
        i = int(i)
        if i not in seen:  # every distinct frame once
            seen.add(i)
            want = (int(st[i]), int(ipc[i]), int(l4c[i]))
            assert pyref.recv_eth(c.frame) == want, c.label
            assert go_verdict(c.frame) == want[0], c.label
            assert int(crc[i]) == pyref.crc32_ieee(c.frame), c.label
        if c.intent is not None:
            assert int(st[i]) == c.intent, (c.label, c.intent, int(st[i]))
    assert len(seen) == len(t.frames) > 14000


def test_series_b_walks_every_l4len(series, table):
    """Series (b): TotalLength follows the cut, so l4len takes every value from 0 to the full segment:
    both sides of l4len < 8 (UDP), l4len < 20 and toff > l4len (TCP) for every IHL, and every frame that
    reaches the compare is accepted (its checksum was refilled)."""
    t, ids = table
    st = t.expected(0)[3]
    got = collections.defaultdict(dict)
    for c, i in zip(series, ids):
        if c.label[0] == "cut_b":
            _, ihl, kind, L = c.label
            got[(ihl, kind)][L - 14 - 4 * ihl] = int(st[i])
    assert set(got) == {(i, k) for i in hg.IHLS for k in hg.CUT_KINDS}
    for (ihl, kind), by in got.items():
        h = hg.l4_header(kind)
        assert set(by) >= set(range(0, h + 6)), (ihl, kind)
        for l4len, v in by.items():
            if l4len < 0:
                want = 7
            elif l4len < (8 if kind == "udp" else 20):
                want = 9
            elif kind != "udp" and h > l4len:
                want = 12
            else:
                want = 0
            assert v == want, (ihl, kind, l4len, v, want)


def test_every_verdict_at_every_ihl(series, table):
    """Verdicts 0..13 for every IHL 5..15 of the frame's geometry (label). Verdict 6 is the one tied to
    the IHL nibble: its frames keep the geometry of the labelled IHL and carry a nibble below 5. Verdict
    2 needs an MTU: it is reached at the mtu_cases() values."""
    t, ids = table
    st0 = t.expected(0)[3]
    mtu = hg.mtu_cases(hg.cut_series())[60]
    stm = t.expected(mtu)[3]
    seen = collections.defaultdict(set)
    for c, i in zip(series, ids):
        seen[c.label[1]].add(int(st0[i]))
        seen[c.label[1]].add(int(stm[i]))
        if st0[i] == 6:
            assert (c.frame[14] & 0xF) < 5 and c.label[0] == "gate"
    for ihl in hg.IHLS:
        assert seen[ihl] == set(range(14)), (ihl, sorted(seen[ihl]))


def _placed_geometry():
    """(label, S, frame, verdict) of the start-offset batch, of the grid at every alignment and of the cut and gate series at starts
    cycling through 0..63: the placements the GPU tests run."""
    t = hg.Table()
    rows = []
    for sc in (hg.start_cases(), hg.grid_at_every_alignment()):
        _, off, _ = hg.place([c.frame for c, _ in sc], [s for _, s in sc])
        rows += [(c.label, int(o), c.frame) for (c, _), o in zip(sc, off)]
    cg = hg.cut_series() + hg.gate_series()
    _, lay = hg.lay_out(hg.in_tiles([c.frame for c in cg], "grid", rotations=(0,)))
    off, _, src, _ = lay[0]
    rows += [(cg[k].label, int(o), cg[k].frame) for k, o in zip(src, off)]
    ids = t.ids([r[2] for r in rows])
    st = t.expected(0)[3][ids]
    return [r + (int(v),) for r, v in zip(rows, st)]


def test_path_predicates_seen_both_ways():
    """The parse's path choices, computed from offsets and lengths as parse_tile / parse_frame compute
    them (sa = S & 3; off and end from the frame's own bytes), each seen true and false for every IHL at
    which both are possible."""
    seen = collections.defaultdict(set)
    for label, S, f, v in _placed_geometry():
        if len(f) < 34:
            continue
        ihl, sa, ln = label[1], S & 3, len(f)
        nib = f[14] & 0xF
        off = 14 + 4 * nib
        end = (14 + int.from_bytes(f[16:18], "big")) & 0xFFFF
        if nib == ihl:
            seen["hsum_global", ihl].add(sa + min(off, ln) > 64)
            if v == 0 or v >= 8:  # past the TotalLength gate: the L4 header dwords q .. q+5 are read
                last = ((sa + ln + 3) >> 2) - 1
                for i in range(6):
                    j = 3 + ihl + i
                    seen["l4_dword_from_memory", ihl].add(j + 1 >= 16)
                    if j + 1 >= 16:
                        seen["l4_dword_clamped", ihl].add(j + 1 > last)
        if end < ln:
            seen["pad_in_16_dwords", ihl].add(sa + ln <= 64)
            seen["pad_in_32_dwords", ihl].add(sa + ln <= 128)
    both = {True, False}
    for ihl in hg.IHLS:
        # sa + off > 64 needs off >= 62: IHL 12 with sa 3, IHL 13 and up at any sa; cut frames keep it false
        assert seen["hsum_global", ihl] == (both if ihl >= 12 else {False}), ihl
        # q + i + 1 >= 16 with q = 3 + IHL, i = 0..5: never below IHL 7, always from IHL 12
        assert seen["l4_dword_from_memory", ihl] == ({False} if ihl < 7 else both if ihl < 12 else {True}), ihl
        if ihl >= 7:
            assert seen["l4_dword_clamped", ihl] == both, ihl
        # padding behind a frame of at most 64 - sa bytes: the shortest frame with any is off + 8 + 1 bytes
        # long (UDP, no payload), so IHL 11 and up (off >= 58) never have it; the 1,400-byte frames are the
        # false side
        assert seen["pad_in_16_dwords", ihl] == (both if 14 + 4 * ihl + 9 <= 64 else {False}), ihl
        assert seen["pad_in_32_dwords", ihl] == both, ihl


def test_segment_kernel_ihl_12_boundary():
    """IHL 12 is where the 16-dword slot's header sum goes to memory for sa == 3 only: both sides are in
    the start-offset batch for every kind, with a frame long enough that min(off, len) = off."""
    sides = collections.defaultdict(set)
    for (c, _), o in zip(hg.start_cases(), hg.place([c.frame for c, _ in hg.start_cases()], [s for _, s in hg.start_cases()])[1]):
        if c.label[1] == 12:
            sides[c.label[2]].add((int(o) & 3) + 62 > 64)
    assert sides == {k: {True, False} for k in hg.GATE_KINDS}


def test_start_offsets_cover_every_residue():
    sc = hg.start_cases()
    assert len(sc) == 128 * 11 * 3 * 3 * 2
    buf, off, ln = hg.place([c.frame for c, _ in sc], [s for _, s in sc])
    assert len(buf) < 8 << 20
    got = collections.defaultdict(set)
    for (c, s), o, n in zip(sc, off, ln):
        assert int(o) % 128 == s and bytes(buf[o : o + n]) == c.frame
        got[c.label].add(int(o) % 128)
    want = {("valid", i, k, p, d) for i in hg.IHLS for k in hg.GATE_KINDS for p in hg.START_PAYLOADS for d in hg.START_PADS}
    assert set(got) == want and all(v == set(range(128)) for v in got.values())
    # frames do not overlap, and every byte outside them is non-zero noise
    mask = np.zeros(len(buf), dtype=np.int32)
    for o, n in zip(off, ln):
        mask[o : o + n] += 1
    assert mask.max() == 1 and (buf[mask == 0] != 0).all()


def test_place_leaves_room_and_shares_giant_fillers():
    big = hg.fillers()[131072][0]
    frames = [b"\x01" * 10, big, b"", b"\x02" * 7, big]
    buf, off, ln = hg.place(frames, [5, 127, 0, 64, 3], room=4, seed=1)
    assert [int(o) % 128 for o in off[:4]] == [5, 127, 0, 64] and off[4] == off[1] and list(ln) == [10, 131072, 0, 7, 131072]
    assert off[1] >= off[0] + 10 + 4 and off[3] >= off[2] + 4 and len(buf) >= off[3] + 7 + 4
    assert bytes(buf[off[1] : off[1] + 131072]) == big and (buf[off[0] + 10 : off[1]] != 0).all()


@pytest.mark.parametrize("context", hg.CONTEXTS)
def test_every_case_at_every_tile_position(context):
    cg = hg.context_cases(context)  # what the GPU tests run in this context
    assert {c.label[:3] for c in cg} == {c.label[:3] for c in hg.series_cases()}
    frames = [c.frame for c in cg]
    orders = hg.in_tiles(frames, context)
    assert len(orders) == 16
    at = collections.defaultdict(set)
    partial = set()
    for order in orders:
        for i, e in enumerate(order):
            if e.src >= 0:
                assert e.frame is frames[e.src]
                at[e.src].add(i % 16)
        lens = [[len(e.frame) for e in order[k : k + 16]] for k in range(0, len(order), 16)]
        src = [[e.src for e in order[k : k + 16]] for k in range(0, len(order), 16)]
        if context == "grid":
            assert len(order) % 16 == 0 and all(s >= 0 for t in src for s in t)
        elif context == "partial_tile":
            partial.add(len(order) % 16)
            assert all(s >= 0 for t in src for s in t)
        else:
            assert all(sum(s >= 0 for s in t) == 1 and len(t) == 16 for t in src)
            big = {"mtu_tile": 1500, "mixed_tile": 9000, "giant_tile": 131072}[context]
            small = 1500 if context == "mtu_tile" else 64
            for t, s in zip(lens, src):
                rest = sorted(n for n, k in zip(t, s) if k < 0)
                assert rest == [small] * (15 if context == "mtu_tile" else 14) + [big] * (context != "mtu_tile")
    assert set(at) == set(range(len(frames))) and all(v == set(range(16)) for v in at.values())
    if context == "partial_tile":
        assert partial == set(range(1, 16))
    # one buffer serves every rotation: each order reads back its own frames
    buf, lay = hg.lay_out(orders[:2])
    for off, ln, src, order in lay:
        for k in range(0, len(order), 97):
            assert bytes(buf[off[k] : off[k] + ln[k]]) == order[k].frame


def test_subsets_keep_every_label(series, table):
    cg = hg.cut_series() + hg.gate_series()
    t, _ = table
    st = t.expected(0)[3][t.ids([c.frame for c in cg])]
    labels = {c.label[:3] for c in cg}
    for pick in (hg.boundary_subset, hg.one_per_label):
        idx = pick(cg, st)
        assert {cg[i].label[:3] for i in idx} == labels
    assert len(hg.one_per_label(cg, st)) == len(labels)
    # the boundary subset keeps both sides of every change of verdict along a cut series
    kept = set(hg.boundary_subset(cg, st))
    groups = collections.defaultdict(list)
    for i, c in enumerate(cg):
        groups[c.label[:3]].append(i)
    changes = 0
    for key, idx in groups.items():
        if key[0] == "gate":
            assert set(idx) <= kept
            continue
        for a, b in zip(idx, idx[1:]):
            assert cg[b].label[3] == cg[a].label[3] + 1
            if st[a] != st[b]:
                changes += 1
                assert a in kept and b in kept, (cg[a].label, cg[b].label)
    assert changes > 3 * 44


def test_mtu_cases_sit_on_length_boundaries():
    for cases, trailer in ((hg.cut_series(), 0), (hg.gate_series(), 0), (hg.valid_grid(), 0), (hg.valid_grid(), 4)):
        lens = collections.Counter(len(c.frame) - trailer for c in cases)
        ms = hg.mtu_cases(cases, trailer)
        assert ms and all(lens[m] and lens[m + 1] for m in ms)
    assert hg.mtu_cases(hg.cut_series()) == list(range(139))
    assert 41 in hg.mtu_cases(hg.gate_series())
