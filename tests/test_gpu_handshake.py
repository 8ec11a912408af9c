"""The handshake of tests/handshake.py on the GPU: the SYNs are fs_segment_batch's, the accept calls
fs_accept_flows_batch's, the clients' and the server's segments fs_send_rings_batch's; the rings stay
device tensors from call to call. After every call its WHOLE output is compared with the model's for the
same inputs, and at the end the handshake must show what tests/test_handshake_model.py asserts."""
import numpy as np
import pytest

import handshake as hs
from test_gpu_accept import compare_accept
from test_gpu_conversation import Device as ConversationDevice
from test_gpu_deliver import compare_delivery, to_device
from test_gpu_recv import compare_recv

pytestmark = pytest.mark.gpu


class Device(ConversationDevice):
    def segment(self, specs, seed):
        import torch

        import segment_ref as sref

        noise, buf, off, ln, dig, st = hs.model_segment(specs, seed)
        frames = torch.from_numpy(noise).to(self.dev)
        payload = torch.zeros(1, dtype=torch.uint8, device=self.dev)
        res = self.eng.segment_device(sref.make_sends(specs), payload, 0, 0, 1, frames=frames)
        torch.cuda.synchronize()
        got = frames.cpu().numpy()
        assert np.array_equal(got, buf), "the SYNs differ from the model's"
        self.calls += 1
        return hs.conv.frames_of_buffer(got, off, ln)

    def accept(self, frames, socks, snd, rings, listeners, slots, seed):
        import torch

        from seqs_amd import split_accept, split_flows, split_snd, split_socks
        from test_gpu_flows import compare

        batch, noise, syn0, e = hs.model_accept(frames, socks, snd, rings.cpu().numpy(), listeners, slots, seed)
        room, n = int(batch[2].sum()), int(batch[2].size)
        pt, st = torch.from_numpy(noise).to(self.dev), torch.from_numpy(syn0).to(self.dev)
        out0, st0 = np.full((len(slots), 2), -7, dtype=np.int32), np.full(len(slots), 0xA5, dtype=np.uint8)
        res = self.eng.accept_flows_device(*to_device(*batch), socks, snd, rings, listeners, slots, payload=pt[3 : 3 + room],
                                           synacks=st, synack_results=(torch.from_numpy(out0).to(self.dev),
                                                                       torch.from_numpy(st0).to(self.dev)))
        torch.cuda.synchronize()
        compare_accept(e, res, out0, st0, n)
        compare_recv(e, res[6], res[7])
        compare_delivery(e, res[8], res[9], rings)
        compare(e, pt.cpu().numpy(), *res[11:])
        self.calls += 1
        # the next step reads the device's own results
        conns, lout, of = split_accept(*res[:3])
        _, flows, _, _ = split_flows(*res[11:14], res[15])
        return dict(e, conns=conns, listeners_out=lout, accept_of=of, synacks=st.cpu().numpy(), snd_out=split_snd(res[6]),
                    socks_out=split_socks(res[8]), code=res[7].cpu().numpy(), flows=flows)


def test_the_handshake_on_the_gpu():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "this test needs a GPU"
    torch.cuda.init()
    eng = Engine(0)
    try:
        be = Device(eng)
        r = hs.run(be)
        hs.check_end(r)
    finally:
        eng.close()
    assert be.calls == 6  # two segment builds, two accept calls, two ring sends
