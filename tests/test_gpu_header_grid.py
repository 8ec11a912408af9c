"""Every header geometry and every RecvEth gate boundary on every kernel (tests/headergrid.py's batches),
bit-exact against the C oracle.

The kernels share one header parse with four header-slot geometries; which path a frame takes depends
on its IHL and TCP data offset, its start offset (modulo 4 for the slot's byte alignment, modulo 16 and
64 for the small-frame kernel's chunks and the one-pass kernel's captured slot), its length, and the
other 15 frames of its tile (header_dma's ballot, mixed and giant tiles, a partial last tile). These
tests run IHL 5..15 x {UDP, TCP data offset 5..15} at every start offset 0..127, every truncation of a
frame per IHL, and both sides of every gate per IHL, at every tile position in five tile contexts,
through the digest, the FCS verify, the TX fill and the two coalesce calls, in every engine column.
tests/test_header_grid_builders.py shows on the CPU that the batches reach the paths they claim.

A digest depends only on the frame's bytes: the oracle runs once per distinct frame and MTU
(headergrid.Table) and every placed batch indexes that result."""
import functools

import numpy as np
import pytest

import engines
import headergrid as hg

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import coracle  # noqa: E402
from seqs_amd import FCS_APPEND, FILL_CSUM, FS_ERR_FCS, split_digests  # noqa: E402


@pytest.fixture(scope="module", params=engines.VARIANTS, ids=engines.IDS)
def engine(request):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = engines.engine_for(request.param)
    yield e
    e.close()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


class Batch:
    """A placed batch: the buffer, then any number of (offsets, lengths, ids, labels) listings of it."""

    def __init__(self, table, buf):
        self.table, self.buf, self.views = table, buf, []

    def add(self, off, ln, frames, labels, name=""):
        self.views.append((np.asarray(off, np.int64), np.asarray(ln, np.int32), self.table.ids(frames), labels, name))
        return self


def check_digests(engine, batch, mtus, fcs=False, views=None):
    """Every listing of the batch under every MTU: the three digest words and the verdict of every frame
    against the oracle's for that frame's bytes."""
    tb = _dev(batch.buf)
    call = engine.digest_fcs_device if fcs else engine.digest_device
    for off, ln, ids, labels, name in (batch.views if views is None else views):
        to, tl = _dev(off), _dev(ln)
        for mtu in mtus:
            out, st = call(tb, to, tl, mtu=mtu)
            torch.cuda.synchronize()
            crc, ipc, l4c = split_digests(out.cpu().numpy())
            st = st.cpu().numpy()
            ecrc, eipc, el4c, est = (x[ids] for x in batch.table.expected(mtu))
            bad = np.flatnonzero((crc != ecrc) | (ipc != eipc) | (l4c != el4c) | (st != est))
            if bad.size:
                i = int(bad[0])
                raise AssertionError(
                    f"{name} mtu {mtu}: {bad.size}/{len(ln)} mismatches; first: case {labels[i]} start offset "
                    f"{int(off[i])} (mod 128: {int(off[i]) % 128}) tile position {i % 16} (frame {i}) len {int(ln[i])}: "
                    f"gpu ({int(crc[i]):#010x}, {int(ipc[i]):#06x}, {int(l4c[i]):#06x}, {int(st[i])}) "
                    f"oracle ({int(ecrc[i]):#010x}, {int(eipc[i]):#06x}, {int(el4c[i]):#06x}, {int(est[i])})")


# ---- the batches (built once, shared by the engine columns) -------------------------------------------

TABLE = hg.Table()
FCS_TABLE = hg.Table(fcs=True)


def placed(table, pairs, name, room=0, seed=0):
    frames = [c.frame for c, _ in pairs]
    buf, off, ln = hg.place(frames, [s for _, s in pairs], room, seed)
    return Batch(table, buf).add(off, ln, frames, [c.label for c, _ in pairs], name)


@functools.lru_cache(maxsize=None)
def starts_batches():
    """(batch, its MTU values): the start-offset batch, and the whole valid grid at every alignment."""
    return tuple((placed(TABLE, pairs, name, seed=seed), [0] + hg.mtu_cases([c for c, _ in pairs]))
                 for seed, (name, pairs) in enumerate((("start offsets", hg.start_cases()),
                                                       ("grid at every alignment", hg.grid_at_every_alignment()))))


@functools.lru_cache(maxsize=None)
def context_batch(context):
    cases = hg.context_cases(context)
    assert {c.label[:3] for c in cases} == {c.label[:3] for c in hg.series_cases()}
    buf, lay = hg.lay_out(hg.in_tiles([c.frame for c in cases], context), starts_mod=64, seed=3)
    b = Batch(TABLE, buf)
    for r, (off, ln, src, order) in enumerate(lay):
        labels = [cases[k].label if k >= 0 else ("filler", len(e.frame)) for k, e in zip(src, order)]
        b.add(off, ln, [e.frame for e in order], labels, f"{context} rotation {r}")
    assert len(buf) < 60 << 20 and max(len(v[0]) for v in b.views) <= 65536
    return b


def series_mtus():
    return [0] + sorted(set(hg.mtu_cases(hg.cut_series()) + hg.mtu_cases(hg.gate_series())))


# ---- 1. the digest --------------------------------------------------------------------------------------

def test_digest_grid_starts(engine):
    """IHL x {udp, tcp5, tcp15} x payload {0, 3, 70} x padding {0, 3} at every start offset 0..127, and the
    whole valid grid at every start alignment; MTU 0 and every MTU on a length boundary."""
    for b, mtus in starts_batches():
        check_digests(engine, b, mtus)


@pytest.mark.parametrize("context", hg.CONTEXTS)
def test_digest_cut_and_gate_series(engine, context):
    """The cut and the gate series, starts cycling through 0..63. Tiles of nothing else: every MTU on a
    length boundary at rotation 0, MTU 0 at the other rotations. Among 1,500-byte frames, in mixed and
    giant tiles and before a partial last tile: every rotation, MTU 0 and 1514."""
    b = context_batch(context)
    if context == "grid":
        check_digests(engine, b, series_mtus(), views=b.views[:1])
        check_digests(engine, b, [0], views=b.views[1:])
    else:
        check_digests(engine, b, [0, 1514])


def test_digest_cut_and_gate_series_capped_grid(engine):
    """The same as context "grid" under fs_ctx_set_workgroups(1): one workgroup streams every tile of the
    series back to back."""
    b = context_batch("grid")
    engine.set_workgroups(1)
    try:
        check_digests(engine, b, series_mtus(), views=b.views[:1])
        check_digests(engine, b, [0], views=b.views[1:])
    finally:
        engine.set_workgroups(0)


# ---- 2. wire frames with their FCS ------------------------------------------------------------------------

def with_fcs(cases):
    """(case, wire frame): each frame with its FCS behind it, one in eight with a bit of it flipped."""
    out = []
    for k, c in enumerate(cases):
        fcs = bytearray(coracle.crc32_zlib(c.frame).to_bytes(4, "little"))
        if k % 8 == 5:
            fcs[k // 8 % 4] ^= 1 << (k // 32 % 8)
        out.append((hg.Case(c.label + ("fcs bad" if k % 8 == 5 else "fcs ok",), c.frame + bytes(fcs), None)))
    return out


@functools.lru_cache(maxsize=None)
def fcs_batch(series):
    if series == "valid":
        cases = with_fcs(hg.valid_grid())
    else:
        # (wire lengths 37 and 38, RecvEth's shortest frame with and without one byte, are cuts 33 and 34)
        cases = with_fcs(hg.cut_series())
        assert {37, 38} <= {len(c.frame) for c in cases}
        cases += [hg.Case(("wire", 5, "udp", n), cases[-1].frame[:n], None) for n in (0, 1, 2, 3)]  # shorter than an FCS
    b = placed(FCS_TABLE, [(c, k % 128) for k, c in enumerate(cases)], f"fcs {series}", seed=4)
    return b, [0] + hg.mtu_cases(cases, trailer=4)


@pytest.mark.parametrize("series", ["valid", "cut"])
def test_fcs_grid(engine, series):
    """fs_digest_batch_fcs on the valid grid and the cut series, the MTU at len - 4 and len - 5 of some frame."""
    b, mtus = fcs_batch(series)
    check_digests(engine, b, mtus, fcs=True)
    st = FCS_TABLE.expected(0)[3][b.views[0][2]]
    assert (st == FS_ERR_FCS).sum() >= len(st) // 8 and (st == 0).any()


# ---- 3. the TX fill ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fill_input():
    """The valid grid and series (b) with stale random bytes in both checksum fields, 4 spare bytes behind
    each frame, starts cycling through 0..127."""
    from test_tx_fcs import stale

    cases = [c for c in hg.valid_grid() + hg.cut_series() if c.label[0] in ("valid", "cut_b")]
    frames = stale([c.frame for c in cases], 7)
    buf, off, ln = hg.place(frames, [k % 128 for k in range(len(frames))], room=4, seed=5)
    return cases, buf, off, ln


@functools.lru_cache(maxsize=None)
def fill_expected(flags):
    cases, buf, off, ln = fill_input()
    ebuf = buf.copy()
    dig, st = coracle.fill_batch(ebuf, off, ln, 0, flags)
    return ebuf, dig, st


@pytest.mark.parametrize("flags", [FILL_CSUM, FCS_APPEND, FILL_CSUM | FCS_APPEND])
def test_fill_grid(engine, flags):
    """fs_fill_batch: the whole buffer byte for byte against the oracle's fill, the noise between the
    frames included: a rejected frame is not written, and the L4 checksum lands at off + 16 (TCP) or
    off + 6 (UDP) for every IHL. (Every engine column runs it, as in tests/test_tx_fcs.py: a column whose
    fill never reaches the small-frame kernel runs the kernel its choice falls back to.)"""
    cases, buf, off, ln = fill_input()
    ebuf, edig, est = fill_expected(flags)
    tb = _dev(buf)
    out, st = engine.fill_device(tb, _dev(off), _dev(ln), mtu=0, flags=flags)
    torch.cuda.synchronize()
    gbuf, st = tb.cpu().numpy(), st.cpu().numpy()
    crc, ipc, l4c = split_digests(out.cpu().numpy())
    diff = np.flatnonzero(gbuf != ebuf)
    if diff.size:
        i = int(np.searchsorted(off, diff[0], side="right")) - 1
        raise AssertionError(f"flags {flags}: {diff.size} bytes differ; first at {int(diff[0])}: case {cases[i].label} start "
                             f"offset {int(off[i])} tile position {i % 16}, byte {int(diff[0] - off[i])} of {int(ln[i])}")
    bad = np.flatnonzero((crc != edig["crc32"]) | (ipc != edig["ip_csum"]) | (l4c != edig["l4_csum"]) | (st != est))
    assert bad.size == 0, (f"flags {flags}: {bad.size} digests differ; first: case {cases[int(bad[0])].label} start offset "
                           f"{int(off[bad[0]])} tile position {int(bad[0]) % 16}")
    if flags & FILL_CSUM:  # what the oracle wrote is where the claim says, for every IHL
        where = {}
        for c, o, n, v in zip(cases, off, ln, est):
            changed = np.flatnonzero(ebuf[o : o + n] != buf[o : o + n])
            if v != 0:
                assert changed.size == 0, c.label
            else:
                l4 = 14 + 4 * c.label[1]
                field = l4 + (6 if c.label[2] == "udp" else 16)
                assert set(changed) <= {24, 25, field, field + 1}, c.label
                where.setdefault((c.label[1], c.label[2] == "udp"), set()).update(set(changed) - {24, 25})
        assert set(where) == {(i, u) for i in hg.IHLS for u in (True, False)}


# ---- 4. the coalesce calls --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def coalesce_input():
    cases = [c for c in hg.series_cases() if c.label[0] in ("gate", "cut_b")]
    frames = [c.frame for c in cases]
    buf, off, ln = hg.place(frames, [k % 64 for k in range(len(frames))], seed=6)
    return cases, buf, off.astype(np.uint64), ln.astype(np.uint32)


def _payload_claims(cases, e, NO_RUN):
    """What the issue claims of the expected result itself: a rejected frame at any IHL has no run and no
    payload; an accepted one contributes [14 + 4 IHL + L4 header, 14 + TotalLength)."""
    total = 0
    for k, (c, v) in enumerate(zip(cases, e["st"])):
        if v != 0:
            assert e["run_of"][k] == NO_RUN, c.label
            continue
        assert e["run_of"][k] != NO_RUN, c.label
        f = c.frame
        l4 = 14 + 4 * c.label[1]
        hdr = 8 if f[23] == 17 else 4 * (f[l4 + 12] >> 4)
        total += 14 + int.from_bytes(f[16:18], "big") - (l4 + hdr)
    assert e["payload_bytes"] == total
    return total


def test_coalesce_gate_series():
    """The gate series and series (b) through fs_coalesce_batch and fs_coalesce_flows_batch, everything
    compared (payload buffer byte for byte, runs, flows, order, run_of, totals, digests, verdicts)."""
    import coalesce_ref
    import flows_ref
    import test_gpu_coalesce
    import test_gpu_flows
    from seqs_amd import Engine

    assert torch.cuda.is_available(), "these tests need a GPU"
    cases, buf, off, ln = coalesce_input()
    eng = Engine(0)
    try:
        for mtu in (0, 1514):
            e = test_gpu_coalesce.check(eng, buf, off, ln, mtu=mtu, plead=3, seed=mtu)
            _payload_claims(cases, e, coalesce_ref.NO_RUN)
            assert {int(v) for v in e["st"]} >= set(range(3, 14)) - {2}
            e = test_gpu_flows.check(eng, buf, off, ln, mtu=mtu, plead=5, seed=mtu)
            _payload_claims(cases, e, flows_ref.NO_RUN)
            # the flow key follows the ports to 14 + 4 IHL: frames that differ in nothing else the key holds
            accepted = [c.frame for c, v in zip(cases, e["st"]) if v == 0]
            assert e["n_accepted"] == len(accepted)
            assert e["n_flows"] == len({flows_ref.flow_key(f) for f in accepted}) > 100
    finally:
        eng.close()
