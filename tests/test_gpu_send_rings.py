"""The ring send on the GPU (fs_send_rings_batch / fs_send_rings_batch_host) against tests/send_ref.py:
the per-socket rule in plain Python, the ring range unwrapped, and from there the pinned restatement
of the TX frame build and the C oracle. Every comparison is the WHOLE frames buffer byte for byte over
noise with a guard tail (a store outside a frame shows), plus offsets, lengths, digests, verdicts and
socks_out. The batches are tests/send_cases.py's."""
import numpy as np
import pytest

import deliver_ref as dref
import flows_ref as fref
import send_cases as cases
import send_ref as ref

pytestmark = pytest.mark.gpu

FCS = ref.FCS_APPEND
TAIL = 256  # noise past the layout's last byte


@pytest.fixture(scope="module")
def eng():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()  # (torch's runtime first, as in the other GPU suites)
    e = Engine(0)
    yield e
    e.close()


def compare(got, off, ln, out, st, outs, ebuf, eoff, eln, edig, est, eouts):
    from seqs_amd import split_digests

    assert np.array_equal(outs, eouts), f"socks_out differs at {np.flatnonzero(outs != eouts)[:8]}"
    assert np.array_equal(off.cpu().numpy().astype(np.uint64), eoff)
    assert np.array_equal(ln.cpu().numpy().astype(np.uint32), eln)
    bad = np.flatnonzero(got != ebuf)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8]} (frame starts {eoff[:4]}...)"
    crc, ipc, l4c = split_digests(out.cpu().numpy())
    assert np.array_equal(crc, edig["crc32"]) and np.array_equal(ipc, edig["ip_csum"])
    assert np.array_equal(l4c, edig["l4_csum"])
    assert np.array_equal(st.cpu().numpy(), est)


def check_device(eng, socks, rings, mtu=0, flags=0, align=1, lead=0, seed=9, dev_rings=None):
    """One fs_send_rings_batch into frames + lead of a noise-filled device buffer; everything compared,
    and `rings` shown untouched."""
    import torch

    from seqs_amd import send_rings_layout

    recs = ref.socks_of(socks)
    n, nbytes, _ = send_rings_layout(recs, flags, align)
    noise = np.random.default_rng(seed).integers(0, 256, lead + nbytes + TAIL, dtype=np.uint8)
    e = ref.expected(socks, rings, mtu, flags, align, noise[lead:])
    assert n == e[2].size
    dev = torch.device("cuda:0")
    buf = torch.from_numpy(noise).to(dev)
    rt = torch.from_numpy(rings).to(dev) if dev_rings is None else dev_rings
    _, off, ln, out, st, outs = eng.send_rings_device(recs, rt, mtu, flags, align, frames=buf[lead:])
    torch.cuda.synchronize()
    compare(buf.cpu().numpy(), off, ln, out, st, outs, np.concatenate([noise[:lead], e[0]]), *e[1:])
    if dev_rings is None:
        assert np.array_equal(rt.cpu().numpy(), rings), "the rings were written"
    return buf, off, ln, out, st, outs


def check_host(eng, socks, rings, mtu=0, flags=0, align=1, seed=9):
    from seqs_amd import send_rings_layout

    recs = ref.socks_of(socks)
    n, nbytes, _ = send_rings_layout(recs, flags, align)
    noise = np.random.default_rng(seed).integers(0, 256, nbytes + TAIL, dtype=np.uint8)
    ebuf, eoff, eln, edig, est, eouts = ref.expected(socks, rings, mtu, flags, align, noise)
    frames, before = noise.copy(), rings.copy()
    _, off, ln, dig, st, outs = eng.send_rings_host(recs, rings, mtu, flags, align, frames=frames)
    assert np.array_equal(outs, eouts) and np.array_equal(off, eoff) and np.array_equal(ln, eln)
    assert np.array_equal(frames, ebuf), np.flatnonzero(frames != ebuf)[:8]
    assert np.array_equal(dig, edig) and np.array_equal(st, est) and np.array_equal(rings, before)


# 1 ---- the wrap at every residue of a 16-byte piece
def test_wrap_at_every_position(eng):
    for rpos in cases.wrap_sweep_positions():
        socks, rings = cases.wrap_sweep(rpos)
        check_device(eng, socks, rings, 0, FCS, 1, lead=rpos % 5, seed=rpos)


# 2 ---- head pieces of every length, the lane stride, the two-piece loop
@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("flags", [0, FCS])
def test_chunk_lengths(eng, align, flags):
    socks, rings = cases.chunk_lengths()
    check_device(eng, socks, rings, 0, flags, align, lead=align == 1 and 5 or 64)


# 2b ---- the same bytes through both entry points: one frame body, so the same frames
@pytest.mark.parametrize("align,flags", [(1, FCS), (64, 0)])
def test_segment_batch_builds_the_same_frames(eng, align, flags):
    import torch

    import segment_ref as sref
    from seqs_amd import segment_layout, send_rings_layout

    dev = torch.device("cuda:0")
    for seed, (socks, rings) in enumerate(cases.both_entry_point_cases()):
        recs = ref.socks_of(socks)
        specs, payload = ref.segment_sends(socks, rings)  # (tests/test_send_host.py: these make the reference's frames)
        sends = sref.make_sends(specs)
        n, nbytes, _ = send_rings_layout(recs, flags, align)
        assert (n, nbytes) == segment_layout(sends, flags, align) and n >= 10
        noise = np.random.default_rng(seed).integers(0, 256, nbytes + TAIL, dtype=np.uint8)
        ring_buf, seg_buf = torch.from_numpy(noise).to(dev), torch.from_numpy(noise).to(dev)
        a = eng.send_rings_device(recs, torch.from_numpy(rings).to(dev), 0, flags, align, frames=ring_buf)
        b = eng.segment_device(sends, torch.from_numpy(payload).to(dev), 0, flags, align, frames=seg_buf)
        torch.cuda.synchronize()
        got, want = ring_buf.cpu().numpy(), seg_buf.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8]}"
        assert (got != noise).sum() > nbytes // 4  # (frames were built)
        for name, x, y in zip(("offsets", "lengths", "digests", "status"), a[1:5], b[1:5]):
            assert x.dtype == y.dtype and x.shape[0] == n and torch.equal(x, y), name


# 3 ---- rings smaller than a piece
def test_tiny_rings(eng):
    socks, rings = cases.tiny_rings()
    check_device(eng, socks, rings, 0, FCS, 1, lead=3)
    check_device(eng, socks, rings, 0, 0, 4)


# 4 ---- a ring that ends with the rings tensor
def test_ring_at_the_end_of_rings(eng):
    socks, rings = cases.ring_at_the_end()
    assert max(s["ring_off"] + s["ring_size"] for s in socks) == rings.size
    check_device(eng, socks, rings, 0, FCS, 1, lead=1)


# 5 ---- the window and the flags
def test_window_and_flags(eng):
    socks, rings = cases.window_and_flags()
    buf, off, ln, out, st, outs = check_device(eng, socks, rings, 0, FCS, 1, lead=2)
    got, off, ln = buf.cpu().numpy()[2:], off.cpu().numpy(), ln.cpu().numpy()
    frames = lambda i: [got[int(off[f]) : int(off[f]) + int(ln[f])].tobytes()  # noqa: E731
                        for f in range(int(outs["first_frame"][i]), int(outs["first_frame"][i]) + int(outs["n_frames"][i]))]
    # a few of them by hand, so that the reference and the kernel do not share a misreading
    assert [int(x) for x in outs["n_frames"][:8]] == [0, 1, 1, 1, 2, 10, 10, 10] and list(outs["bytes"][:3]) == [0, 1, 99]
    assert int(outs["n_frames"][8]) == 0 and int(outs["first_frame"][8]) == ref.NONE
    (ack,) = frames(10)
    assert len(ack) == 54 and ack[47] == 0x10 and int(outs["sent"][10]) == ref.TX_ACK
    assert int.from_bytes(ack[42:46], "big") == socks[10]["rcv_nxt"]
    assert [f[47] for f in frames(12)] == [0x10, 0x10, 0x11] and int(outs["sent"][12]) == ref.TX_FIN
    (fin,) = frames(13)
    assert len(fin) == 54 and fin[47] == 0x11 and int(outs["snd_nxt"][13]) == (socks[13]["snd_nxt"] + 1) & ref.M32
    assert all(f[47] == 0x10 for f in frames(14)) and int(outs["sent"][14]) == 0 and int(outs["bytes"][14]) == 300
    assert [f[47] for f in frames(16)] == [0x10, 0x10, 0x18]
    assert frames(19)[0][48:50] == frames(20)[0][48:50] == b"\xff\xff" and frames(21)[0][48:50] == b"\0\0"
    assert int(outs["n_frames"][22]) == 1 and [f[47] for f in frames(23)] == [0x10, 0x10, 0x18]
    seqs = [int.from_bytes(f[38:42], "big") for f in frames(24)]
    assert seqs[:3] == [0xFFFFFF00, 0xFFFFFF64, 0xFFFFFFC8] and seqs[3] == 0x2C and int(outs["snd_nxt"][24]) == 0x2E8
    assert int(outs["snd_nxt"][26]) == 1


# 6 ---- many sockets, a long socket, a one-workgroup grid
def test_mixed_sockets(eng):
    socks, rings = cases.mixed()
    check_device(eng, socks, rings, 0, FCS, 4, lead=4)
    check_device(eng, socks, rings, 0, 0, 1, lead=1)


def test_long_socket(eng):
    socks, rings = cases.long_socket()
    *_, outs = check_device(eng, socks, rings, 0, FCS, 1, lead=3)
    assert int(outs["n_frames"][0]) == 4096 and int(outs["sent"][0]) == ref.TX_FIN


def test_grid_cap(eng):
    from seqs_amd import Engine

    e = Engine(0)
    try:
        e.set_workgroups(1)  # one workgroup loops over many tiles
        check_device(e, *cases.mixed(), 0, FCS, 1, lead=7)
        check_device(e, *cases.chunk_lengths(), 0, 0, 64, lead=64)
    finally:
        e.close()


def test_nothing_to_send(eng):
    import torch

    from seqs_amd.framesum import TX_SOCK_DTYPE

    socks, rings = cases.mixed()
    quiet = [s for s in socks if ref.rule(s)["S"] == 0]
    *_, st, outs = check_device(eng, quiet, rings, 0, FCS, 1)
    assert st.numel() == 0 and (outs["first_frame"] == ref.NONE).all() and len(outs) == len(quiet)
    res = eng.send_rings_device(np.zeros(0, dtype=TX_SOCK_DTYPE), torch.zeros(1, dtype=torch.uint8, device="cuda:0"))
    assert res[0].numel() == 0 and res[5].size == 0


# 7 ---- the verdict gates
def test_verdicts_of_built_frames(eng):
    socks, rings = cases.rejected_frames()
    *_, st, _ = check_device(eng, socks, rings, 1514, FCS, 1, lead=1)
    assert list(st.cpu().numpy()) == [0, 0, 0, 2, 2, 0, 10, 10, 10, 2]


# 8 ---- two calls in flight, the second from the first's socks_out
def test_back_to_back_calls_equal_one(eng):
    import torch

    from seqs_amd import send_rings_layout

    socks, rings = cases.mixed()
    for s in socks:  # (no PSH: the first call's last segment is not the last of the two)
        s["max_frames"], s["flags"] = 2, s["flags"] & ~ref.TX_PSH
    twice = [dict(s, max_frames=4) for s in socks]
    dev = torch.device("cuda:0")
    rt = torch.from_numpy(rings).to(dev)
    a_recs = ref.socks_of(socks)
    bufs = [torch.zeros(send_rings_layout(a_recs, FCS, 1)[1] * 2 + TAIL, dtype=torch.uint8, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev)
    a = eng.send_rings_device(a_recs, rt, 0, FCS, 1, stream=stream, frames=bufs[0])
    b_recs = a_recs.copy()
    for k in ("snd_nxt", "ring_rpos", "ring_buffered"):
        b_recs[k] = a[5][k]
    b_recs["hdr"][:, 18], b_recs["hdr"][:, 19] = a[5]["ip_id"] >> 8, a[5]["ip_id"] & 0xFF
    # as a stack does it: a FIN that went out is not asked for again, and any frame carried the ACK
    b_recs["flags"] &= ~np.where(a[5]["sent"] == ref.TX_FIN, ref.TX_FIN, 0).astype(np.uint32)
    b_recs["flags"] &= ~np.where(a[5]["n_frames"] > 0, ref.TX_ACK, 0).astype(np.uint32)
    a_recs.view(np.uint8)[:] = 0xA5  # garbage where the first call read its sockets
    b = eng.send_rings_device(b_recs, rt, 0, FCS, 1, stream=stream, frames=bufs[1])
    torch.cuda.synchronize()
    c = check_device(eng, twice, rings, 0, FCS, 1)

    def frames_of(res, i, buf):
        off, ln, out, outs = res[1].cpu().numpy(), res[2].cpu().numpy(), res[3].cpu().numpy(), res[5]
        f0, n = int(outs["first_frame"][i]), int(outs["n_frames"][i])
        return [(buf[int(off[f]) : int(off[f]) + int(ln[f]) + 4].tobytes(), tuple(out[f])) for f in range(f0, f0 + n)]

    ha, hb, hc = bufs[0].cpu().numpy(), bufs[1].cpu().numpy(), c[0].cpu().numpy()
    for i in range(len(socks)):
        assert frames_of(a, i, ha) + frames_of(b, i, hb) == frames_of(c, i, hc), i
    for k in ("snd_nxt", "ring_rpos", "ring_buffered", "ip_id"):
        assert np.array_equal(b[5][k], c[5][k]), k
    assert np.array_equal(a[5]["bytes"] + b[5]["bytes"], c[5]["bytes"])
    assert (b[5]["n_frames"] > 0).sum() > 20 and ((c[5]["sent"] == ref.TX_FIN) & (a[5]["sent"] == 0)).any()


# 9 ---- the host form
def test_host_form_wrap_sweep(eng):
    for rpos in cases.wrap_sweep_positions():
        check_host(eng, *cases.wrap_sweep(rpos), 0, FCS, 1, seed=rpos)


@pytest.mark.parametrize("align,flags", [(1, FCS), (64, 0)])
def test_host_form_mixed(eng, align, flags):
    check_host(eng, *cases.mixed(), 0, flags, align)
    quiet = [s for s in cases.mixed()[0] if ref.rule(s)["S"] == 0]
    check_host(eng, quiet, cases.mixed()[1], 0, flags, align)


# 10 ---- send, deliver, acknowledge
def test_round_trip_through_the_delivery(eng):
    import torch

    from seqs_amd import split_socks, tx_sock_from

    rng = np.random.default_rng(31)
    dev = torch.device("cuda:0")
    tx = [ref.sock(cases.hdr(rng), 1000, 10, 5000, 4000, 3000, snd_una=0xFFFFFA00, snd_nxt=0xFFFFFA00, rcv_nxt=77,
                   flags=ref.TX_PSH),
          ref.sock(cases.hdr(rng), 536, 6000, 4096, 4095, 2500, snd_una=5, snd_nxt=5, rcv_nxt=1 << 31)]
    tx_rings = ref.filled_rings(rng, tx)
    frames, off, ln, out, st, sent = check_device(eng, tx, tx_rings, 0, 0, 4)
    assert list(sent["n_frames"]) == [3, 5] and (st.cpu().numpy() == 0).all()
    perm = torch.tensor([3, 0, 4, 1, 5, 6, 2, 7], device=dev)  # the two flows interleaved, each in order
    # the receivers: the peers of the two senders, their RX rings wrapped
    rx = dref.socks_of(*(dref.sock(fref.flow_key(s["hdr"]), s["snd_nxt"], 100 + 5000 * i, 4000 + i, snd_nxt=s["rcv_nxt"],
                                   ring_wpos=3000 - i) for i, s in enumerate(tx)))
    rx_rings = torch.zeros(100 + 2 * 5000, dtype=torch.uint8, device=dev)
    socks_out, marks, *_, st2 = eng.deliver_flows_device(frames, off[perm].contiguous(), ln[perm].contiguous(), rx,
                                                         rx_rings, payload=False)
    torch.cuda.synchronize()
    got = split_socks(socks_out)
    assert (st2.cpu().numpy() == 0).all() and (marks.cpu().numpy() == 1).all()
    host_rings = rx_rings.cpu().numpy()
    for i, s in enumerate(tx):
        assert int(got["rcv_nxt"][i]) == int(sent["snd_nxt"][i]) and int(got["bytes"][i]) == int(sent["bytes"][i])
        size, wpos = int(rx["ring_size"][i]), int(rx["ring_wpos"][i])
        at = (wpos + np.arange(int(sent["bytes"][i]))) % size + int(rx["ring_off"][i])
        assert host_rings[at].tobytes() == ref.ring_bytes(tx_rings, s, int(sent["bytes"][i]))
    # the ACKs that answer the delivery
    back = ref.socks_of([ref.sock(cases.hdr(rng), 1460, 0, 64, 0, 0, snd_una=s["rcv_nxt"], snd_nxt=s["rcv_nxt"]) for s in tx])
    acks = tx_sock_from(got, back, flags=ref.TX_ACK)
    af, aoff, aln, aout, ast, aouts = eng.send_rings_device(acks, torch.zeros(64, dtype=torch.uint8, device=dev), align=64)
    o3, s3 = eng.digest_device(af, aoff, aln)
    torch.cuda.synchronize()
    host = af.cpu().numpy()
    assert list(aln.cpu().numpy()) == [54, 54] and list(aouts["sent"]) == [ref.TX_ACK] * 2
    for i in range(2):
        f = host[64 * i : 64 * i + 54].tobytes()
        assert int.from_bytes(f[42:46], "big") == int(got["rcv_nxt"][i]) == int(sent["snd_nxt"][i]) and f[47] == 0x10
        assert int.from_bytes(f[48:50], "big") == min(int(got["ring_free"][i]), 65535)
    assert (s3.cpu().numpy() == 0).all() and (ast.cpu().numpy() == 0).all() and torch.equal(o3, aout)


# 11 ---- ring offsets beyond 4 GiB
def test_ring_across_4_gib(eng):
    import torch

    dev = torch.device("cuda:0")
    total = (1 << 32) + (1 << 20)
    if torch.cuda.mem_get_info(dev)[0] < 6 << 30:
        pytest.skip("less than 6 GiB of device memory free")
    rng = np.random.default_rng(32)
    lo = (1 << 32) - 8192
    local = rng.integers(0, 256, total - lo, dtype=np.uint8)
    rings = torch.empty(total, dtype=torch.uint8, device=dev)
    rings[lo:] = torch.from_numpy(local).to(dev)
    # a wrapped ring that spans offset 2^32, one wholly beyond it that ends with the tensor, one below
    socks = [ref.sock(cases.hdr(rng), 1446, (1 << 32) - 3000, 8192, 7000, 6000),
             ref.sock(cases.hdr(rng), 100, total - 5000, 5000, 4990, 777),
             ref.sock(cases.hdr(rng), 999, lo + 1, 4000, 3999, 4000)]
    shifted = [dict(s, ring_off=s["ring_off"] - lo) for s in socks]
    from seqs_amd import send_rings_layout

    recs = ref.socks_of(socks)
    n, nbytes, _ = send_rings_layout(recs, FCS, 1)
    noise = rng.integers(0, 256, nbytes + TAIL, dtype=np.uint8)
    e = ref.expected(shifted, local, 0, FCS, 1, noise)
    buf = torch.from_numpy(noise).to(dev)
    _, off, ln, out, st, outs = eng.send_rings_device(recs, rings, 0, FCS, 1, frames=buf)
    torch.cuda.synchronize()
    compare(buf.cpu().numpy(), off, ln, out, st, outs, *e)
    assert np.array_equal(rings[lo:].cpu().numpy(), local)
    del rings


# ---- rejected calls (a context is needed to tell them from a null context) ---------------------------
def test_rejected_calls(eng):
    import torch

    from seqs_amd import TX_SOCK_OUT_DTYPE, FramesumError

    socks, rings = cases.ring_at_the_end()
    recs = ref.socks_of(socks)
    rt = torch.from_numpy(rings).to("cuda:0")
    with pytest.raises(FramesumError, match="ring outside rings_bytes"):
        eng.send_rings_device(recs, rt[:-1])
    with pytest.raises(FramesumError, match="frames_bytes"):
        eng.send_rings_device(recs, rt, frames=torch.zeros(100, dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(FramesumError, match="ring outside rings_bytes"):
        eng.send_rings_host(recs, rings[:-1])
    bad = recs.copy()
    bad["mss"][1] = 0
    with pytest.raises(FramesumError, match="socket 1: mss"):
        eng.send_rings_device(bad, rt)
    # null rings or frames while there is something to build; neither is needed when there is not
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    sp, outs = recs.ctypes.data, np.zeros(recs.size, dtype=TX_SOCK_OUT_DTYPE)

    def call(socks, n, rings_ptr, frames_ptr):
        return eng.lib.fs_send_rings_batch(eng._ctx, socks, n, rings_ptr, rings.size, 0, 0, 1, frames_ptr, buf.numel(), None,
                                           None, None, None, outs.ctypes.data, None)

    assert call(sp, recs.size, None, buf.data_ptr()) == -1 and b"null rings" in eng.lib.fs_last_error(eng._ctx)
    assert call(sp, recs.size, rt.data_ptr(), None) == -1 and call(None, recs.size, rt.data_ptr(), buf.data_ptr()) == -1
    quiet = recs.copy()
    quiet["ring_buffered"] = 0
    assert call(quiet.ctypes.data, quiet.size, None, None) == 0 and call(None, 0, None, None) == 0
    torch.cuda.synchronize()
    assert int(buf.max()) == 0
