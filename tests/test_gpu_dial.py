"""The handshake of tests/dial.py on the GPU, the library on both ends of the link: the connect calls are
fs_connect_flows_batch's, the accept calls fs_accept_flows_batch's, the clients' segments
fs_send_rings_batch's; the rings stay device tensors from call to call. After every call its WHOLE output is
compared with the model's for the same inputs, and at the end the handshake must show what
tests/test_dial_model.py asserts. The pair whose SYNs cross comes back SynRcvd; completing that open is host
work (a SYN at a listed socket is the delivery's `stop`)."""
import numpy as np
import pytest

import close_ref
import dial
from test_gpu_connect import compare_connect
from test_gpu_deliver import to_device
from test_gpu_handshake import Device as HandshakeDevice

pytestmark = pytest.mark.gpu


class Device(HandshakeDevice):
    def connect(self, frames, openers, seed):
        import torch

        from seqs_amd import split_close, split_connect, split_flows
        from test_gpu_flows import compare

        batch, noise, rep0, e = dial.model_connect(frames, openers, seed)
        none = (dial.dref.socks_of(), dial.rref.snd_of(), torch.zeros(64, dtype=torch.uint8, device=self.dev),
                dial.aref.listeners_of(), dial.aref.slots_of(), close_ref.closers_of())
        rp = torch.from_numpy(rep0).to(self.dev)
        if batch is None:
            tb = to_device(np.zeros(8, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
            res = self.eng.connect_flows_device(*tb, *none, openers, replies=rp, payload=False)
        else:
            room = int(batch[2].sum())
            pt = torch.from_numpy(noise).to(self.dev)
            res = self.eng.connect_flows_device(*to_device(*batch), *none, openers, replies=rp, payload=pt[3 : 3 + room])
        torch.cuda.synchronize()
        compare_connect(e, res)
        if batch is not None:
            assert np.array_equal(split_close(*res[4:7])[2], e["ctl_code"])
            compare(e, pt.cpu().numpy(), *res[4 + 3 + 11 :])
        self.calls += 1
        # the next step reads the device's own results
        out, dig, st = split_connect(res[0], res[2], res[3])
        got = dict(e, openers_out=out, replies=rp.cpu().numpy(), reply_out=dig, reply_status=st)
        if batch is not None:
            got["ctl_code"] = res[6].cpu().numpy()
            got["flows"] = split_flows(*res[18:21], res[22])[1]
        return got


def test_the_dial_on_the_gpu():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "this test needs a GPU"
    torch.cuda.init()
    eng = Engine(0)
    try:
        be = Device(eng)
        r = dial.run(be)
        dial.check_end(r)
    finally:
        eng.close()
    assert be.calls == 5  # two connect calls, two accept calls, one ring send
