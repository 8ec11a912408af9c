"""The conversation of tests/conversation.py on the GPU: every ring send is fs_send_rings_batch, every
receive fs_recv_flows_batch, the rings stay device tensors from round to round, and each call's output
is the next call's input. After every call its WHOLE output is compared with the model's for the same
inputs (a send as tests/test_gpu_send_rings.py's compare: the frames buffer over noise with a guard
tail, offsets, lengths, digests, verdicts, socks_out, the rings untouched; a receive as
tests/test_gpu_recv.py's check: snd_out, code, socks_out, delivered, the whole rings buffer, the flows
arrays), and at the end the conversation must show what tests/test_conversation_model.py asserts."""
import numpy as np
import pytest

import conversation as conv
from test_gpu_deliver import compare_delivery, to_device
from test_gpu_recv import compare_recv

pytestmark = pytest.mark.gpu


class Device:
    """The calls on cuda:0; rings are uint8 device tensors."""

    def __init__(self, eng):
        import torch

        self.eng, self.dev, self.calls = eng, torch.device("cuda:0"), 0

    def rings(self, initial):
        import torch

        return torch.from_numpy(initial.copy()).to(self.dev)

    def put(self, rings, at, data):
        import torch

        rings[at : at + len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(self.dev)

    def get(self, rings, at, n):
        return rings[at : at + n].cpu().numpy().tobytes()

    def send(self, tx, rings, seed):
        import torch

        from test_gpu_send_rings import compare

        before = rings.cpu().numpy()
        noise, *e = conv.model_send(tx, before, seed)
        buf = torch.from_numpy(noise).to(self.dev)
        _, off, ln, out, st, outs = self.eng.send_rings_device(tx, rings, 0, 0, conv.ALIGN, frames=buf)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        compare(got, off, ln, out, st, outs, *e)
        assert np.array_equal(rings.cpu().numpy(), before), "the send wrote into the rings"
        self.calls += 1
        return conv.frames_of_buffer(got, off.cpu().numpy(), ln.cpu().numpy()), outs

    def recv(self, frames, socks, snd, rings, seed):
        import torch

        from seqs_amd import split_snd, split_socks
        from test_gpu_flows import compare

        batch, noise, e = conv.model_recv(frames, socks, snd, rings.cpu().numpy(), seed)
        room = int(batch[2].sum())
        pt = torch.from_numpy(noise).to(self.dev)
        res = self.eng.recv_flows_device(*to_device(*batch), socks, snd, rings, payload=pt[3 : 3 + room])
        torch.cuda.synchronize()
        compare_recv(e, res[0], res[1])
        compare_delivery(e, res[2], res[3], rings)
        compare(e, pt.cpu().numpy(), *res[5:])
        self.calls += 1
        return split_snd(res[0]), split_socks(res[2]), res[1].cpu().numpy(), res[-1].cpu().numpy()


def test_the_conversation_on_the_gpu():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "this test needs a GPU"
    torch.cuda.init()
    eng = Engine(0)
    try:
        be = Device(eng)
        A, B, stats = conv.run(be)
    finally:
        eng.close()
    conv.check_end(A, B, stats)
    assert be.calls == stats["calls"] == 4 * stats["rounds"]
    assert stats["codes"][3] == stats["codes"][5] == stats["codes"][6] == 0 and stats["window_closed"]["B"] == 0
