"""The lifecycles of tests/lifecycle.py on the GPU: the SYNs are fs_segment_batch's, every RX call is
fs_close_flows_batch, the peers' and the server's segments fs_send_rings_batch's; the rings stay device
tensors from call to call. After every call its WHOLE output is compared with the model's for the same
inputs, and at the end the lifecycles must show what tests/test_lifecycle_model.py asserts."""
import numpy as np
import pytest

import lifecycle as lc
from test_gpu_accept import compare_accept
from test_gpu_close import compare_close
from test_gpu_deliver import compare_delivery, to_device
from test_gpu_handshake import Device as HandshakeDevice
from test_gpu_recv import compare_recv

pytestmark = pytest.mark.gpu


class Device(HandshakeDevice):
    def close(self, frames, socks, snd, rings, listeners, slots, closers, seed):
        import torch

        from seqs_amd import split_accept, split_close, split_flows, split_snd, split_socks
        from test_gpu_flows import compare

        batch, noise, syn0, e = lc.model_close(frames, socks, snd, rings.cpu().numpy(), listeners, slots, closers, seed)
        room, n = int(batch[2].sum()), int(batch[2].size)
        pt, st = torch.from_numpy(noise).to(self.dev), torch.from_numpy(syn0).to(self.dev)
        out0, st0 = np.full((len(slots), 2), -7, dtype=np.int32), np.full(len(slots), 0xA5, dtype=np.uint8)
        res = self.eng.close_flows_device(*to_device(*batch), socks, snd, rings, listeners, slots, closers, payload=pt[3 : 3 + room],
                                          synacks=st, synack_results=(torch.from_numpy(out0).to(self.dev),
                                                                      torch.from_numpy(st0).to(self.dev)))
        torch.cuda.synchronize()
        compare_close(e, res)
        acc = res[3:]
        compare_accept(e, acc, out0, st0, n)
        compare_recv(e, acc[6], acc[7])
        compare_delivery(e, acc[8], acc[9], rings)
        compare(e, pt.cpu().numpy(), *acc[11:])
        self.calls += 1
        # the next step reads the device's own results
        cout, sclose, ctl = split_close(*res[:3])
        conns, lout, of = split_accept(*acc[:3])
        _, flows, _, _ = split_flows(*acc[11:14], acc[15])
        return dict(e, closers_out=cout, socks_close=sclose, ctl_code=ctl, conns=conns, listeners_out=lout, accept_of=of,
                    synacks=st.cpu().numpy(), snd_out=split_snd(acc[6]), socks_out=split_socks(acc[8]), code=acc[7].cpu().numpy(),
                    flows=flows)


def test_the_lifecycles_on_the_gpu():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "this test needs a GPU"
    torch.cuda.init()
    eng = Engine(0)
    try:
        be = Device(eng)
        r = lc.run(be)
        lc.check_end(r)
    finally:
        eng.close()
    assert be.calls == 10  # one segment build, five close calls, four ring sends
