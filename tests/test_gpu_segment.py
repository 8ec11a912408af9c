"""The TX frame build on the GPU (fs_segment_batch / fs_segment_batch_host) against the Python
restatement + C oracle of tests/segment_ref.py. Every comparison is the WHOLE frames buffer byte for
byte (gaps, leading and trailing noise included: a store outside a frame shows), plus offsets,
lengths, digests and verdicts."""
import numpy as np
import pytest

import segment_ref as ref

pytestmark = pytest.mark.gpu

FCS = 2
MSS = [1, 2, 63, 64, 65, 127, 536, 1446, 1460]
TAIL = 192  # noise past the layout's last byte


@pytest.fixture(scope="module")
def eng():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()  # (torch's runtime first, as in the other GPU suites)
    e = Engine(0)
    yield e
    e.close()


def edge_specs(seed=2):
    """Case 2's batch: TCP sends over every mss and L in {0, 1, mss-1, mss, mss+1, 3 mss + 7}, UDP
    sends of L in {0, 1, 5, 63, 64, 65, 1472} interleaved, payload ranges at odd offsets."""
    rng = np.random.default_rng(seed)
    udp = [0, 1, 5, 63, 64, 65, 1472]
    specs, at = [], 3
    for mss in MSS:
        for ln in (0, 1, mss - 1, mss, mss + 1, 3 * mss + 7):
            specs.append((ref.tcp_header(rng, seq=int(rng.integers(0, 1 << 32))), at, ln, mss))
            at += ln + int(rng.integers(0, 3))
            if len(specs) % 4 == 0:
                u = udp[(len(specs) // 4) % len(udp)]
                specs.append((ref.udp_header(rng), at, u, 0))
                at += u
    payload = rng.integers(0, 256, at + 7, dtype=np.uint8)
    return specs, payload


def check_device(eng, specs, payload, mtu=0, flags=0, align=4, lead=0, seed=9):
    """One fs_segment_batch into frames + lead of a noise-filled device buffer; everything compared."""
    import torch

    from seqs_amd import segment_layout

    sends = ref.make_sends(specs)
    n, nbytes = segment_layout(sends, flags, align)
    noise = np.random.default_rng(seed).integers(0, 256, lead + nbytes + TAIL, dtype=np.uint8)
    ebuf, eoff, eln, edig, est = ref.expected(specs, payload, mtu, flags, align, noise[lead:])
    assert n == eln.size
    dev = torch.device("cuda:0")
    buf = torch.from_numpy(noise).to(dev)
    pay = torch.from_numpy(payload).to(dev)
    _, off, ln, out, st = eng.segment_device(sends, pay, mtu, flags, align, frames=buf[lead:])
    torch.cuda.synchronize()
    compare(buf.cpu().numpy(), off, ln, out, st, np.concatenate([noise[:lead], ebuf]), eoff, eln, edig, est)
    return buf, off, ln, out, st


def compare(got, off, ln, out, st, ebuf, eoff, eln, edig, est):
    from seqs_amd import split_digests

    assert np.array_equal(off.cpu().numpy().astype(np.uint64), eoff)
    assert np.array_equal(ln.cpu().numpy().astype(np.uint32), eln)
    bad = np.flatnonzero(got != ebuf)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8]} (frame starts {eoff[:4]}...)"
    crc, ipc, l4c = split_digests(out.cpu().numpy())
    assert np.array_equal(crc, edig["crc32"]) and np.array_equal(ipc, edig["ip_csum"])
    assert np.array_equal(l4c, edig["l4_csum"])
    assert np.array_equal(st.cpu().numpy(), est)


def test_kat_round_trip(eng):
    frames, specs, payload = ref.kat_sends()
    for flags in (0, FCS):
        buf, off, ln, _, st = check_device(eng, specs, payload, 0, flags, 1)
        got = buf.cpu().numpy()
        for f, o, n in zip(frames, off.cpu().numpy(), ln.cpu().numpy()):
            assert got[int(o) : int(o) + int(n)].tobytes() == f
        assert (st.cpu().numpy() == 0).all()


@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("flags", [0, FCS])
def test_chunk_length_edges(eng, align, flags):
    specs, payload = edge_specs()
    check_device(eng, specs, payload, 0, flags, align, lead=align == 1 and 5 or 64)


def test_verdicts_of_built_frames(eng):
    # frames RecvEth rejects before its checksum compare: above the MTU, a zero port, and a
    # TotalLength that wraps the reference's uint16 `end`; beside frames that pass
    rng = np.random.default_rng(4)
    zero_port = bytearray(ref.tcp_header(rng))
    zero_port[34:36] = b"\0\0"
    specs = [(ref.tcp_header(rng), 0, 4000, 1460), (ref.tcp_header(rng), 5, 3000, 0), (bytes(zero_port), 9, 100, 40),
             (ref.udp_header(rng), 1, 1472, 0), (ref.udp_header(rng), 2, 1473, 0)]
    payload = rng.integers(0, 256, 70000, dtype=np.uint8)
    *_, st = check_device(eng, specs, payload, 1514, FCS, 1, lead=1)
    assert list(st.cpu().numpy()) == [0, 0, 0, 2, 10, 10, 10, 0, 2]
    check_device(eng, [(ref.tcp_header(rng), 7, 65495, 0), (ref.udp_header(rng), 11, 65507, 0)], payload, 0, FCS, 4)


def test_relative_alignment_sweep(eng):
    # every source phase x destination phase of a 64-byte row: send i reads payload + i, and its
    # first frame lands at d + 1290 i, which takes every residue mod 64 as d runs over 0..63
    rng = np.random.default_rng(6)
    payload = rng.integers(0, 256, 64 + 1000 + 8, dtype=np.uint8)
    specs = [(ref.tcp_header(rng), i, 1000, 200) for i in range(64)]
    for d in range(64):
        check_device(eng, specs, payload, 0, FCS, 1, lead=d, seed=d)


def test_long_send(eng):
    # 4,096 frames of one send: the ID chain prand16^k at large k, Seq wrapping 2^32
    rng = np.random.default_rng(8)
    payload = rng.integers(0, 256, 4096 * 16 + 3, dtype=np.uint8)
    specs = [(ref.tcp_header(rng, seq=0xFFFFF000, ident=1), 3, 4096 * 16, 16),
             (ref.tcp_header(rng, seq=0xFFFFFFFF, ident=0xBEEF), 0, 4095 * 7 + 1, 7)]
    check_device(eng, specs, payload, 0, FCS, 1, lead=3)
    check_device(eng, specs, payload, 0, 0, 4)


def test_grid_cap(eng):
    from seqs_amd import Engine

    e = Engine(0)
    try:
        e.set_workgroups(1)  # one workgroup loops over many tiles
        specs, payload = edge_specs()
        for align, flags in ((1, FCS), (64, 0)):
            check_device(e, specs, payload, 0, flags, align, lead=64 + 7)
    finally:
        e.close()


def test_round_trips_through_digest_entry_points(eng):
    import torch

    specs, payload = edge_specs(seed=5)
    buf, off, ln, out, st = check_device(eng, specs, payload, 0, FCS, 4)
    o2, s2 = eng.digest_fcs_device(buf, off, ln + 4)
    torch.cuda.synchronize()
    assert (s2.cpu().numpy() == 0).all() and torch.equal(o2, out)
    buf, off, ln, out, st = check_device(eng, specs, payload, 0, 0, 4)
    o2, s2 = eng.digest_device(buf, off, ln)
    torch.cuda.synchronize()
    assert (s2.cpu().numpy() == 0).all() and torch.equal(o2, out)


@pytest.mark.parametrize("streams", [1, 2])
def test_in_flight_reuse_of_sends(eng, streams):
    # two calls, the caller's sends array overwritten between them, no synchronization
    import torch

    from seqs_amd import segment_layout

    rng = np.random.default_rng(12)
    dev = torch.device("cuda:0")
    payload = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
    batches = []
    for _ in range(2):
        specs = [(ref.tcp_header(rng), int(rng.integers(0, 1 << 19)), int(rng.integers(2000, 12000)), 1446)
                 for _ in range(256)]
        batches.append((specs, ref.make_sends(specs)))
    pay = torch.from_numpy(payload).to(dev)
    noises = [rng.integers(0, 256, segment_layout(s, FCS, 1)[1] + TAIL, dtype=np.uint8) for _, s in batches]
    bufs = [torch.from_numpy(x).to(dev) for x in noises]
    torch.cuda.synchronize()
    ss = [torch.cuda.Stream(dev) for _ in range(streams)]
    sends = batches[0][1].copy()
    res = []
    for i in range(2):
        sends[:] = batches[i][1]
        res.append(eng.segment_device(sends, pay, 0, FCS, 1, stream=ss[i % streams], frames=bufs[i]))
        sends.view(np.uint8)[:] = 0xA5  # garbage where the call read its sends
    torch.cuda.synchronize()
    for i in range(2):
        e = ref.expected(batches[i][0], payload, 0, FCS, 1, noises[i])
        compare(bufs[i].cpu().numpy(), *res[i][1:], *e)


@pytest.mark.parametrize("pinned", [False, True])
def test_host_form(eng, pinned):
    from seqs_amd import segment_layout

    specs, payload = edge_specs()
    sends = ref.make_sends(specs)
    for align, flags in ((1, FCS), (64, 0), (64, FCS), (1, 0)):
        n, nbytes = segment_layout(sends, flags, align)
        noise = np.random.default_rng(align + flags).integers(0, 256, nbytes + TAIL, dtype=np.uint8)
        if pinned:
            frames, pay = eng.host_empty(noise.size), eng.host_empty(payload.size)
            frames[:], pay[:] = noise, payload
        else:
            frames, pay = noise.copy(), payload
        _, off, ln, dig, st = eng.segment_host(sends, pay, 0, flags, align, frames=frames)
        ebuf, eoff, eln, edig, est = ref.expected(specs, payload, 0, flags, align, noise)
        assert np.array_equal(frames, ebuf) and np.array_equal(off, eoff) and np.array_equal(ln, eln)
        assert np.array_equal(dig, edig) and np.array_equal(st, est)


def test_segment_batch_lists(eng):
    rng = np.random.default_rng(13)
    hdrs = [ref.tcp_header(rng), ref.udp_header(rng), ref.tcp_header(rng)]
    pays = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (3000, 700, 0)]
    got = eng.segment_batch(hdrs, pays, 1460, append_fcs=True)
    specs, at = [], 0
    for h, p in zip(hdrs, pays):
        specs.append((h, at, len(p), 0 if len(h) == 42 else 1460))
        at += len(p)
    payload = np.frombuffer(b"".join(pays), dtype=np.uint8)
    ebuf, eoff, eln, _, _ = ref.expected(specs, payload, 0, FCS, 1, np.zeros(8192, dtype=np.uint8))
    want = [ebuf[int(o) : int(o) + int(n) + 4].tobytes() for o, n in zip(eoff, eln)]
    assert [len(g) for g in got] == [3, 1, 1] and [f for g in got for f in g] == want


def test_sanity_of_rejected_calls(eng):
    import torch

    from seqs_amd import FramesumError

    rng = np.random.default_rng(14)
    sends = ref.make_sends([(ref.tcp_header(rng), 0, 1000, 100)])
    pay = torch.zeros(999, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(FramesumError):  # the payload range ends past payload_bytes
        eng.segment_device(sends, pay)
    pay = torch.zeros(1000, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(FramesumError):  # frames_bytes below the layout's
        eng.segment_device(sends, pay, frames=torch.zeros(1559, dtype=torch.uint8, device="cuda:0"))
    assert eng.segment_device(sends[:0], pay)[1].numel() == 0  # no sends: success, nothing written


def test_workload_shape_once(eng):
    # 1,024 sends x 64 frames of 1500 bytes (the C2 shape), align 4, with FCS
    rng = np.random.default_rng(15)
    per = 64 * 1446
    payload = rng.integers(0, 256, 1024 * per, dtype=np.uint8)
    specs = [(ref.tcp_header(rng), i * per, per, 1446) for i in range(1024)]
    *_, st = check_device(eng, specs, payload, 0, FCS, 4)
    assert st.numel() == 65536
