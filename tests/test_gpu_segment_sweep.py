"""The TX frame build on the GPU at the shapes tests/test_gpu_segment.py leaves out: every chunk
length up to three whole turns of the chunk loop and a piece (so every C mod 16, every lane for the
short first piece, J = 1..4 turns), segmentation with an mss above 2048, and the kernel's own
frame -> send search at 63 / 64 / 65 sends and with a third level (above 4,096 sends). Same method as
there: the WHOLE frames buffer byte for byte, offsets, lengths, digests and verdicts against
tests/segment_ref.py + the C oracle; the every-length frames then go through fs_coalesce_batch and
must give their payload slices back. The builders (no GPU needed) are also run by
tests/test_edge_case_builders.py."""
import numpy as np
import pytest

import coalesce_ref as cref
import segment_ref as ref
from test_gpu_coalesce import TAIL as CO_TAIL
from test_gpu_coalesce import compare as co_compare
from test_gpu_segment import FCS, check_device

pytestmark = pytest.mark.gpu

SWEEP_MAX = 3 * 1024 + 80
LARGE_MSS = (2047, 2048, 2049, 4101, 8946)
SEARCH_SENDS = (1, 2, 63, 64, 65, 4095, 4096, 4097)


@pytest.fixture(scope="module")
def eng():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "these tests need a GPU"
    torch.cuda.init()  # (torch's runtime first, as in the other GPU suites)
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng1():
    from seqs_amd import Engine

    e = Engine(0)
    e.set_workgroups(1)  # one workgroup: its 12 waves loop over the tiles, each with a search of its own
    yield e
    e.close()


def turns(C):
    """The turns J of build_frame's chunk loop for a chunk of C bytes: 64 pieces of 16 bytes a turn."""
    return -(-(-(-C // 16)) // 64)


def sweep_specs(seed=16):
    """One single-frame send (mss 0) per chunk length C = 0 .. SWEEP_MAX, TCP for even C and UDP for
    odd, its payload at payload + C % 61."""
    rng = np.random.default_rng(seed)
    specs = [(ref.tcp_header(rng, seq=int(rng.integers(0, 1 << 32))) if C % 2 == 0 else ref.udp_header(rng), C % 61, C, 0)
             for C in range(SWEEP_MAX + 1)]
    return specs, rng.integers(0, 256, 60 + SWEEP_MAX + 5, dtype=np.uint8)


def large_mss_specs(seed=17):
    rng = np.random.default_rng(seed)
    specs, at = [], 1
    for mss in LARGE_MSS:
        for L in (2 * mss + 1, 2 * mss + 15, 3 * mss - 1, 3 * mss):
            specs.append((ref.tcp_header(rng, seq=int(rng.integers(0, 1 << 32))), at, L, mss))
            at += L + int(rng.integers(0, 3))
    return specs, rng.integers(0, 256, at + 7, dtype=np.uint8)


def search_specs(n_sends, long_first, seed=18):
    """n_sends one-frame UDP sends of 1..9 bytes; `long_first`: send 0 is a TCP send of 70 frames
    (mss 3) instead, which makes the prefix of frame counts irregular and crosses the stride of the
    staged IPv4 ID powers."""
    rng = np.random.default_rng(seed + n_sends)
    specs = [(ref.udp_header(rng), 3 * i % 50, 1 + i % 9, 0) for i in range(n_sends)]
    if long_first:
        specs[0] = (ref.tcp_header(rng, seq=0xFFFFFF80), 2, 208, 3)
    return specs, rng.integers(0, 256, 256, dtype=np.uint8)


# ---- 1. every chunk length -----------------------------------------------------------------------

def test_every_chunk_length_and_back_through_the_coalesce(eng):
    import torch

    from seqs_amd import split_runs

    specs, payload = sweep_specs()
    lead = 3
    buf, off, ln, _, st = check_device(eng, specs, payload, 0, FCS, 1, lead=lead)
    assert (st.cpu().numpy() == 0).all()
    # the frames as they lie on the device, with their FCS, through fs_coalesce_batch
    hb = buf.cpu().numpy()
    ho, hl = (off + lead).cpu().numpy().astype(np.uint64), (ln + 4).cpu().numpy().astype(np.uint32)
    room = int(hl.sum())
    noise = np.random.default_rng(19).integers(0, 256, 5 + room + CO_TAIL, dtype=np.uint8)
    e = cref.expected(hb, ho, hl, 0, cref.RX_FCS, noise, 5, room)
    pt = torch.from_numpy(noise).to(buf.device)
    res = eng.coalesce_device(buf, off + lead, ln + 4, 0, cref.RX_FCS, payload=pt[5 : 5 + room])
    torch.cuda.synchronize()
    co_compare(e, pt.cpu().numpy(), *res[1:])
    runs, total, n_runs = split_runs(res[1], res[3])
    assert n_runs == len(specs) == SWEEP_MAX + 1 and total == sum(C for _, _, C, _ in specs)
    got, at = pt.cpu().numpy()[5:], 0
    for (_, start, C, _), r in zip(specs, runs):  # one run per send, its bytes the send's payload slice
        assert (int(r["payload_off"]), int(r["payload_len"]), int(r["n_frames"])) == (at, C, 1)
        assert got[at : at + C].tobytes() == payload[start : start + C].tobytes()
        at += C


def test_every_chunk_length_without_fcs_in_64_byte_slots(eng):
    specs, payload = sweep_specs()
    *_, st = check_device(eng, specs, payload, 0, 0, 64, lead=64)
    assert (st.cpu().numpy() == 0).all()


# ---- 2. large mss --------------------------------------------------------------------------------

@pytest.mark.parametrize("align,flags", [(1, FCS), (64, 0)])
def test_large_mss(eng, align, flags):
    specs, payload = large_mss_specs()
    *_, ln, _, st = check_device(eng, specs, payload, 0, flags, align, lead=align == 1 and 7 or 64)
    assert ln.numel() == 3 * len(specs) and (st.cpu().numpy() == 0).all()


# ---- 3. the frame -> send search -----------------------------------------------------------------

@pytest.mark.parametrize("n_sends", SEARCH_SENDS)
def test_send_search(eng, eng1, n_sends):
    for long_first in (False, True):
        specs, payload = search_specs(n_sends, long_first)
        for e in (eng, eng1):  # uncapped (a tile of one frame per wave while they last), and one workgroup
            for flags, align in ((FCS, 1), (0, 4)):
                *_, ln, _, _ = check_device(e, specs, payload, 0, flags, align, lead=align == 1 and 1 or 0, seed=n_sends)
                assert ln.numel() == n_sends + (69 if long_first else 0)
