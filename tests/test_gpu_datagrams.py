"""tests/datagrams.py's exchange on the GPU: the frames are fs_segment_batch's UDP build, every call is
fs_udp_flows_batch over sentinel-filled result tensors, and every call's whole output (ports_out, port_of,
cell_of, every byte of cells) is what tests/udp_ref.py gives for the same frames, with the CPU oracle's
verdicts; the whole exchange ends as the model's does."""
import numpy as np
import pytest

import datagrams as dg
import flows_ref as fref
import udp_ref as ref
from test_gpu_close import SentinelEmpty
from test_gpu_deliver import to_device
from test_gpu_udp import Lists, oracle_status

pytestmark = pytest.mark.gpu


def test_two_endpoints_exchange_datagrams():
    import torch

    from seqs_amd import Engine
    from seqs_amd.framesum import UDP_PORT_OUT_DTYPE

    assert torch.cuda.is_available(), "these tests need a GPU"
    eng = Engine(0)
    dev = torch.device("cuda:0")
    lists = Lists()
    calls = []

    def build(headers, payloads):
        frames = [f[0] for f in eng.segment_batch(headers, payloads, 0)]
        for f, h, p in zip(frames, headers, payloads):  # the build's frame carries the template's addresses and the payload
            assert f[:12] == h[:12] and f[26:38] == h[26:38] and f[42:] == p and len(f) == 42 + len(p)
        return frames

    def call(frames, ports, cells):
        if not frames:
            return dg.model_call(frames, ports, cells)
        buf, off, ln = fref.pack(frames, lead=len(calls) % 8)
        ct = torch.from_numpy(cells).to(dev)
        with SentinelEmpty(len(calls)):
            res = eng.udp_flows_device(*to_device(buf, off, ln), lists.socks, lists.snd, torch.zeros(8, dtype=torch.uint8, device=dev),
                                       lists.listeners, lists.slots, lists.closers, lists.openers, ports, ct, payload=False)
        torch.cuda.synchronize()
        got = (res[0].cpu().numpy().reshape(-1).view(UDP_PORT_OUT_DTYPE).copy(), res[1].cpu().numpy().view(np.uint32),
               res[2].cpu().numpy().view(np.uint32), ct.cpu().numpy())
        want = ref.expected(frames, oracle_status(buf, off, ln), ports, cells)
        assert got[0].tobytes() == want[0].tobytes(), (got[0], want[0])
        assert all(np.array_equal(x, y) for x, y in zip(got[1:], want[1:]))
        calls.append(len(frames))
        return got

    try:
        log = dg.run(build, call)
    finally:
        eng.close()
    model = dg.run()
    assert len(calls) == len(log) == len(model) == 2 * dg.ROUNDS
    for (who, frames, ports, out), (mwho, mframes, mports, mout) in zip(log, model):
        assert who == mwho and ports.tobytes() == mports.tobytes() and len(frames) == len(mframes)
        assert out[0].tobytes() == mout[0].tobytes() and all(np.array_equal(x, y) for x, y in zip(out[1:], mout[1:]))
