"""tests/neighbours.py's exchange on the GPU, the library on both ends of the link: every ARP call is
fs_arp_flows_batch over sentinel-filled result tensors, the handshake's calls are tests/test_gpu_dial.py's; after
every call its WHOLE output is compared with the model's for the same inputs (the CPU oracle's verdicts), and the
exchange ends as tests/test_neighbours_model.py asserts."""
import numpy as np
import pytest

import arp_ref as ref
import flows_ref as fref
import neighbours as nb
from test_gpu_arp import NO_PORTS, differences
from test_gpu_close import SentinelEmpty
from test_gpu_deliver import to_device
from test_gpu_dial import Device
from test_gpu_udp import Lists, oracle_status

pytestmark = pytest.mark.gpu


def test_two_endpoints_start_from_ip_addresses_alone():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "this test needs a GPU"
    torch.cuda.init()
    eng = Engine(0)
    dev = torch.device("cuda:0")
    lists = Lists()
    calls = []

    def arp(frames, hosts, queries, n_reply, flags, seed):
        slots = n_reply + len(queries)
        frames0, out0, st0 = nb.prefill(slots, seed)
        if frames:
            buf, off, ln = fref.pack(frames, lead=len(calls) % 8)
            status = oracle_status(buf, off, ln)
        else:
            buf, off, ln, status = np.zeros(64, dtype=np.uint8), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32), []
        want = ref.expected(frames, status, hosts, queries, n_reply, flags, frames0, out0, st0)
        ft = torch.from_numpy(frames0).to(dev)
        pair = (torch.from_numpy(out0.view(np.int32).reshape(-1, 2).copy()).to(dev), torch.from_numpy(st0).to(dev))
        with SentinelEmpty(len(calls)):
            res = eng.arp_flows_device(*to_device(buf, off, ln), lists.socks, lists.snd, torch.zeros(8, dtype=torch.uint8, device=dev),
                                       lists.listeners, lists.slots, lists.closers, lists.openers, NO_PORTS[0],
                                       torch.zeros(8, dtype=torch.uint8, device=dev), hosts, queries, n_reply_slots=n_reply,
                                       arp_flags=flags, arp_frames=ft, arp_results=pair, payload=False)
        torch.cuda.synchronize()
        got = (res[0], res[1], ft, res[3], res[4], res[5], res[6])
        bad = differences(got, want)
        assert not bad, "\n".join(bad)
        calls.append(len(frames))
        # the next step reads the device's own results
        return (res[0].cpu().numpy().reshape(-1).view(ref.HOST_OUT_DTYPE).copy(), res[1].cpu().numpy().reshape(-1).view(ref.QUERY_OUT_DTYPE).copy(),
                ft.cpu().numpy(), res[3].cpu().numpy().reshape(-1).view(ref.DIGEST_DTYPE).copy(), res[4].cpu().numpy(), res[5].cpu().numpy(),
                res[6].cpu().numpy().view(np.uint32))

    try:
        be = Device(eng)
        r = nb.run(be, arp)
        nb.check_end(r)
    finally:
        eng.close()
    assert calls == [0, 3, 1, 2 * nb.SWEEP] and be.calls == 3  # four ARP calls; two connect calls and one accept call
    import dial

    model = nb.run(dial.Model())
    for (who, frames, hosts, queries, n_reply, flags, seed, out), m in zip(r["log"], model["log"]):
        assert who == m[0] and frames == m[1] and hosts.tobytes() == m[2].tobytes() and ref.same(out, m[7]) == []
