"""The in-order TCP delivery on the GPU (fs_deliver_flows_batch / fs_deliver_flows_batch_host) against
the sequential restatement of tests/deliver_ref.py, bit for bit: socks_out, delivered, the WHOLE rings
buffer (filled with a sentinel pattern first: a stray or a missing byte shows) and every output of the
flow-aware coalesce (tests/test_gpu_flows.py's comparison)."""
import ctypes

import numpy as np
import pytest

import deliver_ref as ref
import engines
import flows_ref as fref
import segment_ref as sref

pytestmark = pytest.mark.gpu

ACK, FIN, PSH, SYN, RST = fref.ACK, fref.FIN, fref.PSH, ref.SYN, ref.RST
TAIL = 96


@pytest.fixture(scope="module")
def eng():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()
    e = Engine(0)
    yield e
    e.close()


def to_device(buf, off, ln):
    import torch

    dev = torch.device("cuda:0")
    return (torch.from_numpy(buf).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
            torch.from_numpy(ln.astype(np.int32)).to(dev))


def sentinel(nbytes, seed=0):
    return np.random.default_rng(500 + seed).integers(0, 256, nbytes, dtype=np.uint8)


def compare_delivery(e, socks_out, delivered, rings):
    from seqs_amd import split_socks

    got = split_socks(socks_out)
    assert got.tobytes() == e["socks_out"].tobytes(), (got, e["socks_out"])
    if delivered is not None:
        assert np.array_equal(delivered.cpu().numpy(), e["delivered"]), (delivered.cpu().numpy()[:32], e["delivered"][:32])
    bad = np.flatnonzero(rings.cpu().numpy() != e["rings"])
    assert bad.size == 0, f"{bad.size} ring bytes differ, first at {bad[:8]}"


def check(eng, frames, socks, rings_bytes, mtu=0, flags=0, cap=None, payload=True, delivered=True, lead=1, seed=0,
          e=None, batch=None):
    """One fs_deliver_flows_batch of the frames (a list of bytes, or `batch` = (buf, off, ln)) with the
    sockets `socks` over a sentinel-filled rings buffer; everything compared. `e`: the expected dict of
    an earlier check of the same case. Returns the expected dict."""
    import torch

    from test_gpu_flows import compare

    buf, off, ln = batch if batch is not None else fref.pack(frames, lead=lead, seed=seed)
    room = 0 if not payload else (int(ln.sum()) if cap is None else cap)
    noise = np.random.default_rng(77 + seed).integers(0, 256, 3 + room + TAIL, dtype=np.uint8)
    rings = sentinel(rings_bytes, seed)
    if e is None:
        e = ref.expected(buf, off, ln, mtu, flags, noise, 3, room, socks, rings)
    dev = torch.device("cuda:0")
    pt, rt = torch.from_numpy(noise).to(dev), torch.from_numpy(rings).to(dev)
    res = eng.deliver_flows_device(*to_device(buf, off, ln), socks, rt, mtu, flags,
                                   payload=pt[3 : 3 + room] if payload else False, delivered=delivered)
    torch.cuda.synchronize()
    compare_delivery(e, res[0], res[1], rt)
    compare(e, pt.cpu().numpy(), *res[3:])
    return e


def snd_of(hdr):
    """The Ack the flow's frames carry: a socket with this snd_nxt passes rule (c)."""
    return int.from_bytes(hdr[42:46], "big")


def with_ack(hdr, ack):
    h = bytearray(hdr)
    h[42:46] = (ack % (1 << 32)).to_bytes(4, "big")
    return bytes(h)


def sock_for(hdr, rcv_nxt, ring_off, ring_size, **kw):
    kw.setdefault("snd_nxt", snd_of(hdr))
    return ref.sock(ref.key_of_header(hdr), rcv_nxt, ring_off, ring_size, **kw)


def marks(e):
    return [int(x) for x in e["delivered"]]


def out_of(e, s=0):
    o = e["socks_out"][s]
    return {k: int(o[k]) for k in o.dtype.names}


# ---- 1. interleaved flows, with and without sockets ----------------------------------------------

def three_flows(rng):
    hdrs = [fref.flow_header(rng, 0x1000 + f) for f in range(3)]
    segs = [fref.segments(rng, h, 1000 * (f + 1), [100] * 5) for f, h in enumerate(hdrs)]
    frames = [segs[g][k] for g, k in fref.interleave([range(5)] * 3)]
    frames.insert(4, fref.udp_frame(rng, b"a udp datagram"))
    return hdrs, fref.finish(frames)


@pytest.mark.parametrize("variant", engines.VARIANTS, ids=engines.IDS)
def test_three_interleaved_flows_two_sockets(variant):
    import torch

    assert torch.cuda.is_available()
    rng = np.random.default_rng(11)
    hdrs, frames = three_flows(rng)
    socks = ref.socks_of(sock_for(hdrs[2], 3000, 7, 600), sock_for(hdrs[0], 1000, 700, 500))
    e2 = engines.engine_for(variant)
    try:
        e = check(e2, frames, socks, 1300)
    finally:
        e2.close()
    assert [out_of(e, s)["bytes"] for s in (0, 1)] == [500, 500] and sum(marks(e)) == 10
    assert [out_of(e, s)["flow"] for s in (0, 1)] == [2, 0]
    assert [out_of(e, s)["stop"] for s in (0, 1)] == [15, 5]
    assert out_of(e, 0)["rcv_nxt"] == 3500 and out_of(e, 1)["ring_wpos"] == 0 and out_of(e, 1)["ring_free"] == 0


def test_no_sockets_equals_coalesce_flows(eng):
    import torch

    rng = np.random.default_rng(12)
    _, frames = three_flows(rng)
    buf, off, ln = fref.pack(frames, lead=2)
    e = check(eng, frames, ref.socks_of(), 64, batch=(buf, off, ln))
    assert marks(e) == [0] * len(frames)
    tb, to, tl = to_device(buf, off, ln)
    a = eng.coalesce_flows_device(tb, to, tl, payload=torch.zeros(int(ln.sum()), dtype=torch.uint8, device=tb.device))
    b = eng.deliver_flows_device(tb, to, tl, ref.socks_of(), torch.zeros(8, dtype=torch.uint8, device=tb.device),
                                 payload=torch.zeros(int(ln.sum()), dtype=torch.uint8, device=tb.device))
    torch.cuda.synchronize()
    n_runs, n_flows, n_acc = e["n_runs"], e["n_flows"], e["n_accepted"]
    for x, y, cut in zip(a, b[2:], (None, n_runs, n_flows, n_acc, None, None, None, None)):
        assert torch.equal(x[:cut], y[:cut])
    assert b[0].numel() == 0 and not bool(b[1].any())


def test_socket_without_frames_and_empty_batch(eng):
    import torch

    from seqs_amd import split_flows, split_socks

    rng = np.random.default_rng(13)
    hdrs, frames = three_flows(rng)
    stranger = fref.flow_header(rng, 0x7777)
    socks = ref.socks_of(sock_for(stranger, 5, 0, 64, ring_wpos=9, ring_free=30), sock_for(hdrs[1], 2000, 64, 512))
    e = check(eng, frames, socks, 600)
    assert out_of(e, 0) == dict(rcv_nxt=5, ring_wpos=9, ring_free=30, bytes=0, n_delivered=0, n_dropped=0,
                                flow=ref.NONE, stop=ref.NONE)
    assert out_of(e, 1)["bytes"] == 500
    # n of 0: zero totals, the input state
    buf, off, ln = fref.pack(frames)
    tb, to, tl = to_device(buf, off, ln)
    rings = torch.from_numpy(sentinel(600)).to(tb.device)
    res = eng.deliver_flows_device(tb, to[:0], tl[:0], socks, rings)
    torch.cuda.synchronize()
    assert bytes(split_flows(*res[3:6], res[7])[3].tobytes()) == bytes(24)
    so = split_socks(res[0])
    for s in range(2):
        assert (int(so[s]["rcv_nxt"]), int(so[s]["ring_wpos"]), int(so[s]["ring_free"])) == \
            (int(socks[s]["rcv_nxt"]), int(socks[s]["ring_wpos"]), int(socks[s]["ring_free"]))
        assert [int(so[s][k]) for k in ("bytes", "n_delivered", "n_dropped", "flow", "stop")] == [0, 0, 0, ref.NONE, ref.NONE]
    assert np.array_equal(rings.cpu().numpy(), sentinel(600))


# ---- 2. the ring ---------------------------------------------------------------------------------

def one_flow(seed, sizes, seq=1000, **kw):
    rng = np.random.default_rng(seed)
    hdr = fref.flow_header(rng, 0x2000 + seed)
    return hdr, fref.finish(fref.segments(rng, hdr, seq, sizes, **kw))


def test_ring_wrap(eng):
    hdr, frames = one_flow(21, [100, 100, 100])
    e = check(eng, frames, ref.socks_of(sock_for(hdr, 1000, 13, 4096, ring_wpos=4000)), 4200)
    assert out_of(e)["ring_wpos"] == 204 and out_of(e)["bytes"] == 300 and marks(e) == [1, 1, 1]
    want = b"".join(f[54:] for f in frames)
    assert e["rings"][13 + 4000 : 13 + 4096].tobytes() == want[:96] and e["rings"][13 : 13 + 204].tobytes() == want[96:]


def test_frame_ends_at_the_rings_end_and_ring_of_one_byte(eng):
    hdr, frames = one_flow(22, [96, 100])
    e = check(eng, frames, ref.socks_of(sock_for(hdr, 1000, 5, 4096, ring_wpos=4000)), 4200)
    assert out_of(e)["ring_wpos"] == 100 and marks(e) == [1, 1]
    hdr, frames = one_flow(23, [1, 1, 2])
    e = check(eng, frames, ref.socks_of(sock_for(hdr, 1000, 33, 1)), 70)
    assert marks(e) == [1, 2, 2] and out_of(e) | dict(flow=0) == dict(
        rcv_nxt=1001, ring_wpos=0, ring_free=0, bytes=1, n_delivered=1, n_dropped=2, flow=0, stop=3)


def test_ring_full_in_a_run_then_the_retransmission(eng):
    rng = np.random.default_rng(24)
    hdr = fref.flow_header(rng, 0x2424)
    first = fref.segments(rng, hdr, 1000, [100] * 4)
    again = fref.segments(rng, hdr, 1250, [30, 20])  # nxt stays at 1200: this run is not the next either
    retransmitted = fref.segments(rng, hdr, 1200, [40, 10])
    frames = fref.finish(first + again + retransmitted)
    e = check(eng, frames, ref.socks_of(sock_for(hdr, 1000, 0, 1024, ring_wpos=1000, ring_free=250)), 1024)
    assert marks(e) == [1, 1, 2, 2, 2, 2, 1, 1]
    assert out_of(e) == dict(rcv_nxt=1250, ring_wpos=226, ring_free=0, bytes=250, n_delivered=4, n_dropped=4, flow=0, stop=8)


# ---- 3. the window, Seq and Ack ------------------------------------------------------------------

@pytest.mark.parametrize("wnd,want", [(99, [2, 2]), (100, [1, 1]), (101, [1, 1]), (0, [2, 2])])
def test_window(eng, wnd, want):
    hdr, frames = one_flow(31, [100, 100])
    e = check(eng, frames, ref.socks_of(sock_for(hdr, 1000, 0, 512, rcv_wnd=wnd)), 512, seed=wnd)
    assert marks(e) == want


def test_fin_counts_against_the_window(eng):
    hdr, frames = one_flow(32, [50, 100], last_flags=ACK | FIN)
    e = check(eng, frames, ref.socks_of(sock_for(hdr, 1000, 0, 512, rcv_wnd=100)), 512)  # len + 1 = wnd + 1
    assert marks(e) == [1, 2] and out_of(e)["stop"] == 2
    e = check(eng, frames, ref.socks_of(sock_for(hdr, 1000, 0, 512, rcv_wnd=101)), 512)
    assert marks(e) == [1, 1] and out_of(e)["rcv_nxt"] == 1151


def test_out_of_order_duplicate_and_off_by_one(eng):
    rng = np.random.default_rng(33)
    hdr = fref.flow_header(rng, 0x3333)
    a = fref.segments(rng, hdr, 1000, [10, 20])
    later = fref.segments(rng, hdr, 1100, [10, 10])     # out of order
    dup = fref.segments(rng, hdr, 1000, [10, 20])       # a duplicate of the first run
    plus1 = fref.segments(rng, hdr, 1031, [5])          # starts at nxt + 1
    nxt = fref.segments(rng, hdr, 1030, [7])
    frames = fref.finish(a + later + dup + plus1 + nxt)
    e = check(eng, frames, ref.socks_of(sock_for(hdr, 1000, 3, 256)), 300)
    assert marks(e) == [1, 1, 2, 2, 2, 2, 2, 1] and out_of(e)["rcv_nxt"] == 1037


def test_run_across_2_pow_32(eng):
    hdr, frames = one_flow(34, [60, 60, 60], seq=0xFFFFFF9C)
    e = check(eng, frames, ref.socks_of(sock_for(hdr, 0xFFFFFF9C, 0, 256)), 256)
    assert marks(e) == [1, 1, 1] and out_of(e)["rcv_nxt"] == (0xFFFFFF9C + 180) % (1 << 32) == 80


@pytest.mark.parametrize("snd", [5000, 0x7FFFFFFF, 0xFFFFFFFF])
def test_ack_of_unsent_data_is_dropped_inside_a_run(eng, snd):
    rng = np.random.default_rng(35)
    hdr = with_ack(fref.flow_header(rng, 0x3535), snd)  # Ack == snd_nxt
    segs = fref.segments(rng, hdr, 1000, [10, 10, 10, 10])
    bad = fref.tcp_frame(with_ack(hdr, snd + 1), 1010, segs[1][54:])
    noack = fref.tcp_frame(with_ack(hdr, snd + 77), 1000, segs[0][54:], flags=PSH)  # no ACK flag: (c) does not apply
    frames = fref.finish([noack, bad] + segs[2:])
    e = check(eng, frames, ref.socks_of(sock_for(hdr, 1000, 0, 128, snd_nxt=snd)), 128, seed=snd & 0xFF)
    assert marks(e) == [1, 2, 2, 2]
    # ... and an Ack below snd_nxt passes
    frames = fref.finish([fref.tcp_frame(with_ack(hdr, snd - 1), 1000, segs[0][54:])])
    assert marks(check(eng, frames, ref.socks_of(sock_for(hdr, 1000, 0, 128, snd_nxt=snd)), 128)) == [1]


# ---- 4. SYN, RST, FIN, pure ACKs -----------------------------------------------------------------

@pytest.mark.parametrize("flag", [SYN, RST, SYN | ACK])
def test_syn_and_rst_end_the_walk(eng, flag):
    rng = np.random.default_rng(41)
    hdr = fref.flow_header(rng, 0x4141)
    segs = fref.segments(rng, hdr, 1000, [10, 10, 10, 10])
    segs[2] = fref.tcp_frame(hdr, 1020, segs[2][54:], flags=flag)
    other = fref.segments(rng, fref.flow_header(rng, 0x4242), 7, [9])
    frames = fref.finish(segs[:1] + other + segs[1:])
    e = check(eng, frames, ref.socks_of(sock_for(hdr, 1000, 0, 128)), 128, seed=flag)
    assert marks(e) == [1, 0, 1, 0, 0] and out_of(e)["stop"] == 2 and out_of(e)["rcv_nxt"] == 1020


def test_fin_ends_the_walk(eng):
    rng = np.random.default_rng(42)
    hdr = fref.flow_header(rng, 0x4242)
    segs = fref.segments(rng, hdr, 1000, [10, 10], last_flags=ACK | FIN) + fref.segments(rng, hdr, 1021, [5, 5])
    e = check(eng, fref.finish(segs), ref.socks_of(sock_for(hdr, 1000, 0, 128)), 128)
    assert marks(e) == [1, 1, 0, 0] and out_of(e)["stop"] == 2 and out_of(e)["rcv_nxt"] == 1021
    # FIN with an empty payload, pure ACKs between the data frames
    segs = [fref.tcp_frame(hdr, 1000, b"0123456789"), fref.tcp_frame(hdr, 1010, b""), fref.tcp_frame(hdr, 1010, b""),
            fref.tcp_frame(hdr, 1010, b"abcde"), fref.tcp_frame(hdr, 1015, b"", flags=ACK | FIN),
            fref.tcp_frame(hdr, 1016, b"late")]
    e = check(eng, fref.finish(segs), ref.socks_of(sock_for(hdr, 1000, 0, 128)), 128, seed=1)
    assert marks(e) == [1, 0, 0, 1, 1, 0]
    assert out_of(e) == dict(rcv_nxt=1016, ring_wpos=15, ring_free=113, bytes=15, n_delivered=3, n_dropped=0, flow=0, stop=5)


# ---- 5. header geometries, rejected frames, FCS --------------------------------------------------

def test_ip_and_tcp_options_are_data_frames(eng):
    rng = np.random.default_rng(51)
    hdr = fref.flow_header(rng, 0x5151)
    pay = [rng.integers(0, 256, 20 + k, dtype=np.uint8).tobytes() for k in range(5)]
    seqs = np.concatenate([[1000], 1000 + np.cumsum([len(p) for p in pay])])
    frames = fref.finish([
        fref.tcp_frame(hdr, int(seqs[0]), pay[0]),
        fref.tcp_frame(hdr, int(seqs[1]), pay[1], ip_options=b"\x01" * 4),
        fref.tcp_frame(hdr, int(seqs[2]), pay[2], ip_options=b"\x01" * 40),
        fref.tcp_frame(hdr, int(seqs[3]), pay[3], options=b"\x01" * 4),
        fref.tcp_frame(hdr, int(seqs[4]), pay[4], options=b"\x01" * 40, ip_options=b"\x01" * 8),
    ])
    e = check(eng, frames, ref.socks_of(sock_for(hdr, 1000, 1, 128, ring_wpos=50)), 140)
    assert list(e["st"]) == [0] * 5 and marks(e) == [1] * 5 and out_of(e)["bytes"] == 110 > 128 - 50


@pytest.mark.parametrize("fcs", [False, True])
def test_checksum_failed_frame_inside_a_run(eng, fcs):
    rng = np.random.default_rng(52)
    hdr = fref.flow_header(rng, 0x5252)
    frames = fref.finish(fref.segments(rng, hdr, 1000, [30, 30, 30]) + fref.segments(rng, hdr, 1030, [30]), fcs=fcs)
    f = bytearray(frames[1])
    f[60] ^= 0x40
    frames[1] = bytes(f)
    e = check(eng, frames, ref.socks_of(sock_for(hdr, 1000, 0, 128)), 128, flags=fref.RX_FCS if fcs else 0)
    # the damaged frame is in no flow; the run behind it fails (a) until the retransmission comes
    assert e["st"][1] in (13, 14) and marks(e) == [1, 0, 2, 1] and out_of(e)["rcv_nxt"] == 1060


# ---- 6. the packed payload is optional -----------------------------------------------------------

def test_payload_null_and_payload_cap_short(eng):
    rng = np.random.default_rng(61)
    hdrs, frames = three_flows(rng)
    socks = ref.socks_of(sock_for(hdrs[0], 1000, 0, 512), sock_for(hdrs[1], 2000, 512, 512))
    full = check(eng, frames, socks, 1024)
    for kw in (dict(payload=False), dict(cap=700), dict(delivered=False)):
        e = check(eng, frames, socks, 1024, **kw)
        assert e["socks_out"].tobytes() == full["socks_out"].tobytes() and np.array_equal(e["rings"], full["rings"])
        assert np.array_equal(e["delivered"], full["delivered"]) and e["payload_bytes"] == full["payload_bytes"]


# ---- 7. sizes ------------------------------------------------------------------------------------

def long_flow(n, seed, size=10):
    """One flow of n frames of `size` bytes each, in order, built with numpy (tests/test_gpu_flows.py)."""
    from test_gpu_flows import big_batch

    assert size == 10
    return big_batch(np.zeros(n, dtype=np.int64), seed)


@pytest.mark.parametrize("n", [65, 257, 1100])
def test_one_long_flow(eng, n):
    buf, off, ln = long_flow(n, 70 + n)
    f0 = buf[int(off[0]) : int(off[0]) + 54].tobytes()
    seq0 = int.from_bytes(f0[38:42], "big")
    # the ring is short by one frame: every frame but the last is admitted, wrapping once
    size = 10 * (n - 1)
    socks = ref.socks_of(sock_for(f0, seq0, 11, size, ring_wpos=size - 25))
    e = check(eng, None, socks, size + 40, batch=(buf, off, ln), seed=n)
    assert marks(e) == [1] * (n - 1) + [2]
    assert out_of(e) == dict(rcv_nxt=(seq0 + size) % (1 << 32), ring_wpos=size - 25, ring_free=0, bytes=size,
                             n_delivered=n - 1, n_dropped=1, flow=0, stop=n)


def many_flows(n_flows=300, per=3, seed=75):
    from test_gpu_flows import big_batch

    flow_of = np.tile(np.arange(n_flows, dtype=np.int64), per)  # interleaved
    buf, off, ln = big_batch(flow_of, seed)
    socks = []
    for f in range(n_flows):
        h = buf[int(off[f]) : int(off[f]) + 54].tobytes()
        socks.append(sock_for(h, int.from_bytes(h[38:42], "big"), 40 * (n_flows - 1 - f) + 3, 32, ring_wpos=f % 32))
    return (buf, off, ln), ref.socks_of(*socks)


def test_300_flows_300_sockets(eng):
    batch, socks = many_flows()
    e = check(eng, None, socks, 40 * 300 + 8, batch=batch)
    assert int(e["socks_out"]["bytes"].sum()) == 9000 and (e["delivered"] == 1).all()
    assert sorted(int(x) for x in e["socks_out"]["flow"]) == list(range(300))


def test_hash_mask_and_one_workgroup(eng):
    from seqs_amd import Engine
    from seqs_amd.framesum import TEST_LIB_PATH

    batch, socks = many_flows(seed=76)
    e = check(eng, None, socks, 40 * 300 + 8, batch=batch)
    te = Engine(0, lib_path=TEST_LIB_PATH)
    try:
        for mask in (0, 0xF, 0xFFFFFFFF):
            assert te.lib.fs_test_set_flow_hash_mask(te._ctx, mask) == 0
            check(te, None, socks, 40 * 300 + 8, batch=batch, e=e)
        te.set_workgroups(1)
        check(te, None, socks, 40 * 300 + 8, batch=batch, e=e)
        buf, off, ln = long_flow(1100, 77)
        f0 = buf[int(off[0]) : int(off[0]) + 54].tobytes()
        check(te, None, ref.socks_of(sock_for(f0, int.from_bytes(f0[38:42], "big"), 0, 16384)), 16384, batch=(buf, off, ln))
    finally:
        te.close()


def mixed_flow(seed, n, free):
    """One flow of n frames around a receiver that starts at Seq 5000 with `free` ring bytes: in-order
    segments, duplicates, segments ahead, pure ACKs, segments above the window, ACKs of unsent data,
    in random order, so that the walk restarts inside and across its chunks of 64 lanes."""
    rng = np.random.default_rng(seed)
    hdr = with_ack(fref.flow_header(rng, 0x7A00 + seed), 9000)
    nxt, left, frames, last = 5000, free, [], 8
    for _ in range(n):
        kind = rng.choice(["next", "next", "next", "next", "dup", "ahead", "ack", "wide", "unsent"])
        size = int(rng.integers(1, 40))
        data = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
        if kind == "next":
            frames.append(fref.tcp_frame(hdr, nxt, data))
            if size <= left:
                nxt, left, last = nxt + size, left - size, size
        elif kind == "dup":
            frames.append(fref.tcp_frame(hdr, nxt - last, data[:last]))
        elif kind == "ahead":
            frames.append(fref.tcp_frame(hdr, nxt + int(rng.integers(1, 9)), data))
        elif kind == "ack":
            frames.append(fref.tcp_frame(hdr, nxt, b""))
        elif kind == "wide":
            frames.append(fref.tcp_frame(hdr, nxt, bytes(301)))  # above the window of 300
        else:
            frames.append(fref.tcp_frame(with_ack(hdr, 9001), nxt, data))
    return hdr, fref.finish(frames)


@pytest.mark.parametrize("seed,n,free", [(1, 64, 4000), (2, 200, 2500), (3, 333, 1 << 20), (4, 129, 900)])
def test_mixed_flow_restarts_the_walk(eng, seed, n, free):
    hdr, frames = mixed_flow(seed, n, free)
    size = max(free, 1024)
    socks = ref.socks_of(sock_for(hdr, 5000, 9, size, rcv_wnd=300, snd_nxt=9000, ring_wpos=size - 100, ring_free=free))
    e = check(eng, frames, socks, size + 32, seed=seed)
    o = out_of(e)
    assert o["n_delivered"] > n // 5 and o["n_dropped"] > n // 8 and o["n_delivered"] + o["n_dropped"] < n
    assert set(marks(e)) == {0, 1, 2} and o["stop"] == n


def test_back_to_back_calls_need_no_synchronization(eng):
    import torch

    from test_gpu_flows import compare

    cases = []
    for seed, n, free in ((5, 150, 3000), (6, 40, 500), (7, 260, 1 << 16)):
        hdr, frames = mixed_flow(seed, n, free)
        size = max(free, 1024)
        socks = ref.socks_of(sock_for(hdr, 5000, 0, size, rcv_wnd=300, snd_nxt=9000, ring_free=free))
        buf, off, ln = fref.pack(frames, lead=seed)
        noise = np.random.default_rng(seed).integers(0, 256, int(ln.sum()) + TAIL, dtype=np.uint8)
        rings = sentinel(size, seed)
        e = ref.expected(buf, off, ln, 0, 0, noise, 0, int(ln.sum()), socks, rings)
        dev = torch.device("cuda:0")
        cases.append((e, to_device(buf, off, ln), socks, torch.from_numpy(noise).to(dev), torch.from_numpy(rings).to(dev),
                      int(ln.sum())))
    torch.cuda.synchronize()
    res = [eng.deliver_flows_device(*batch, socks, rt, payload=pt[:room]) for _, batch, socks, pt, rt, room in cases]
    torch.cuda.synchronize()
    for (e, _, _, pt, rt, _), r in zip(cases, res):
        compare_delivery(e, r[0], r[1], rt)
        compare(e, pt.cpu().numpy(), *r[3:])


# ---- 8. the host form ----------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["three flows", "wrap"])
def test_host_form(eng, case):
    if case == "three flows":
        hdrs, frames = three_flows(np.random.default_rng(81))
        socks = ref.socks_of(sock_for(hdrs[1], 2000, 100, 600, ring_wpos=550), sock_for(hdrs[0], 1000, 900, 500))
        nbytes = 1500  # bytes 0..99, 700..899 and 1400.. belong to no ring
    else:
        hdr, frames = one_flow(82, [100, 100, 100])
        socks = ref.socks_of(sock_for(hdr, 1000, 64, 4096, ring_wpos=4000))
        nbytes = 4300
    buf, off, ln = fref.pack(frames, lead=9)
    room = int(ln.sum())
    noise = np.random.default_rng(61).integers(0, 256, room + TAIL, dtype=np.uint8)
    rings = sentinel(nbytes, 8)
    e = ref.expected(buf, off, ln, 0, 0, noise, 0, room, socks, rings)
    mine = noise.copy()
    so, dl, pay, runs, flows, order, run_of, totals, dig, st = eng.deliver_flows_host(buf, off, ln, socks, rings, payload=mine[:room])
    assert so.tobytes() == e["socks_out"].tobytes() and np.array_equal(dl, e["delivered"])
    assert np.array_equal(rings, e["rings"])  # in place, the bytes between the rings the caller's
    assert np.array_equal(mine, e["payload"]) and runs.tobytes() == e["runs"].tobytes()
    assert flows.tobytes() == e["flows"].tobytes() and np.array_equal(order, e["order"])
    assert np.array_equal(run_of, e["run_of"]) and np.array_equal(dig, e["dig"]) and np.array_equal(st, e["st"])
    assert int(totals["n_accepted"]) == e["n_accepted"] and int(totals["payload_bytes"]) == e["payload_bytes"]
    # n of 0 on the host: the input state
    so = eng.deliver_flows_host(buf, off[:0], ln[:0], socks, rings, payload=False)[0]
    assert [int(x) for x in so["rcv_nxt"]] == [int(x) for x in socks["rcv_nxt"]] and (so["flow"] == ref.NONE).all()


# ---- 9. the round trip through fs_segment_batch --------------------------------------------------

def test_segmented_sends_arrive_in_their_rings(eng):
    import torch

    from seqs_amd import split_socks

    rng = np.random.default_rng(91)
    payload = rng.integers(0, 256, 5000, dtype=np.uint8)
    hdrs = [fref.flow_header(rng, 0x9100 + k, flags=ACK | PSH) for k in range(2)]
    specs = [(hdrs[0], 0, 3001, 536), (hdrs[1], 3001, 1999, 100)]
    dev = torch.device("cuda:0")
    frames, off, ln, _, st = eng.segment_device(sref.make_sends(specs), torch.from_numpy(payload).to(dev), 0, 0, 4)
    counts = [sref.n_frames(mss, n) for _, _, n, mss in specs]
    perm = np.array([sum(counts[:g]) + k for g, k in fref.interleave([range(c) for c in counts])], dtype=np.int64)
    pt = torch.from_numpy(perm).to(dev)
    socks = ref.socks_of(*[sock_for(h, int.from_bytes(h[38:42], "big"), at, n, ring_wpos=0) for h, at, n, _ in specs])
    rings = torch.zeros(5000, dtype=torch.uint8, device=dev)
    res = eng.deliver_flows_device(frames, off[pt].contiguous(), ln[pt].contiguous(), socks, rings, payload=False)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all() and res[2] is None
    assert np.array_equal(rings.cpu().numpy(), payload)
    so = split_socks(res[0])
    assert [int(x) for x in so["bytes"]] == [3001, 1999] and [int(x) for x in so["ring_free"]] == [0, 0]
    assert [int(x) for x in so["n_delivered"]] == counts and bool((res[1] == 1).all())


# ---- the call's own checks -----------------------------------------------------------------------

def test_rejected_calls(eng):
    import torch

    from seqs_amd import FramesumError

    hdr, frames = one_flow(95, [10])
    tb, to, tl = to_device(*fref.pack(frames))
    rings = torch.zeros(256, dtype=torch.uint8, device=tb.device)
    good = sock_for(hdr, 1000, 0, 128)
    other = sock_for(fref.flow_header(np.random.default_rng(1), 0x9595), 1, 128, 128)

    def bad(field, value, base=good):
        s = base.copy()
        s[field] = value
        return s

    for socks in (ref.socks_of(good, good), ref.socks_of(good, bad("ring_off", 127, other)),
                  ref.socks_of(bad("ring_size", 0)), ref.socks_of(bad("ring_wpos", 128)),
                  ref.socks_of(bad("ring_free", 129)), ref.socks_of(bad("ring_off", 129)),
                  ref.socks_of(bad("reserved", [0, 1, 0])), ref.socks_of(bad("key", [17] + [0] * 12))):
        with pytest.raises(FramesumError, match="socket"):
            eng.deliver_flows_device(tb, to, tl, socks, rings)
    with pytest.raises(FramesumError):
        eng.deliver_flows_device(tb, to, tl, ref.socks_of(good), rings, flags=2)
    lib, vp = eng.lib, ctypes.c_void_p
    some = vp(tb.data_ptr())
    s1 = ref.socks_of(good)
    for socks_p, rings_p, out_p in ((None, some, some), (vp(s1.ctypes.data), None, some), (vp(s1.ctypes.data), some, None)):
        assert lib.fs_deliver_flows_batch(eng._ctx, some, some, some, 1, 0, 0, socks_p, 1, rings_p, 256, out_p, None, None, 0,
                                          some, some, some, None, some, None, None, None) == -1
    assert lib.fs_deliver_flows_batch(eng._ctx, some, some, some, 1, 0, 0, vp(s1.ctypes.data), 65537, some, 256, some, None,
                                      None, 0, some, some, some, None, some, None, None, None) == -1
    torch.cuda.synchronize()
    assert not bool(rings.any())
