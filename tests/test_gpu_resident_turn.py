"""The resident conversation of tests/resident_turn.py on the GPU: every send is fs_send_rings_resident on a
TX socket table that stays a device tensor from the first round to the last, with the receive call's
socks_out and snd_out TENSORS handed off as they are and FS_TX_WRITEBACK set; every receive is
fs_recv_flows_batch. After every send its whole output (the frames buffer over noise with a guard tail, the
four arrays with their untouched tails, socks_out, totals, the table) is compared with the model's for the
same inputs, the receives as tests/test_gpu_conversation.py compares them, and the endpoint asserts after
every send that the table equals the host chain."""
import numpy as np
import pytest

import conversation as conv
import resident_turn as rt
from test_gpu_conversation import Device

pytestmark = pytest.mark.gpu


class ResidentDevice(Device):
    """The calls on cuda:0; tables and rings are device tensors."""

    def table(self, recs):
        from seqs_amd import tx_socks_tensor

        return tx_socks_tensor(recs, self.dev)

    def read_table(self, table):
        from seqs_amd.framesum import TX_SOCK_DTYPE, _records

        return _records(table, TX_SOCK_DTYPE).copy()

    def edit(self, table, c, ring_buffered, set_flags):
        import torch

        row = self.read_table(table[c : c + 1])  # the application raises ring_buffered and sets flags, nothing else
        row["ring_buffered"], row["flags"] = ring_buffered, row["flags"] | np.uint32(set_flags)
        table[c] = torch.from_numpy(row.view(np.uint8).copy()).to(self.dev)

    def send_resident(self, table, rings, rx_out, seed):
        import torch

        from seqs_amd import split_snd, split_socks, split_tx
        from seqs_amd.framesum import DIGEST_DTYPE, _records
        from test_gpu_send_resident import sentinels

        before = rings.cpu().numpy()
        host_rx = None if rx_out is None else (split_socks(rx_out[0]), split_snd(rx_out[1]))  # (for the model alone)
        noise, cap, e = rt.model_send_resident(self.read_table(table), before, host_rx, seed)
        sent = sentinels(cap, seed + 1)
        buf = torch.from_numpy(noise).to(self.dev)
        arrays = [torch.from_numpy(a.view(np.uint8).copy()).to(self.dev).view(t) for a, t in
                  zip(sent, (torch.int64, torch.int32, torch.int32, torch.uint8))]
        arrays[2] = arrays[2].view(-1, 2)
        rx = (None, None) if rx_out is None else rx_out
        res = self.eng.send_rings_resident(table, rings, cap, frames=buf, rx_socks_out=rx[0], rx_snd_out=rx[1], writeback=True,
                                           align=conv.ALIGN, offsets=arrays[0], lengths=arrays[1], out=arrays[2], status=arrays[3])
        torch.cuda.synchronize()
        outs, totals, after = split_tx(res[5], res[6], table)
        k = int(totals["n_frames"])
        got = buf.cpu().numpy()
        bad = np.flatnonzero(got != e[0])
        assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8]}"
        for a, d, want, whole in zip(arrays, (np.uint64, np.uint32, DIGEST_DTYPE, np.uint8), e[1:5], sent):
            mine = _records(a, d)
            assert np.array_equal(mine[:k], want) and np.array_equal(mine[k:], whole[k:])
        assert np.array_equal(outs, e[5]) and totals == e[6] and (e[4] == 0).all()
        assert np.array_equal(after, conv.send_ref.socks_of(e[7]["after"])), "the table differs from the model's"
        assert np.array_equal(rings.cpu().numpy(), before), "the send wrote into the rings"
        self.calls += 1
        return conv.frames_of_buffer(got, e[1], e[2]), outs

    def recv_resident(self, frames, socks, snd, rings, seed):
        import torch

        from seqs_amd import split_snd, split_socks
        from test_gpu_deliver import compare_delivery, to_device
        from test_gpu_flows import compare
        from test_gpu_recv import compare_recv

        batch, noise, e = conv.model_recv(frames, socks, snd, rings.cpu().numpy(), seed)
        room = int(batch[2].sum())
        pt = torch.from_numpy(noise).to(self.dev)
        res = self.eng.recv_flows_device(*to_device(*batch), socks, snd, rings, payload=pt[3 : 3 + room])
        torch.cuda.synchronize()
        compare_recv(e, res[0], res[1])
        compare_delivery(e, res[2], res[3], rings)
        compare(e, pt.cpu().numpy(), *res[5:])
        self.calls += 1
        # the tensors themselves go to the next send: (socks_out, snd_out)
        return split_snd(res[0]), split_socks(res[2]), res[1].cpu().numpy(), res[-1].cpu().numpy(), (res[2], res[0])


def test_the_resident_conversation_on_the_gpu():
    import torch

    from seqs_amd import Engine

    assert torch.cuda.is_available(), "this test needs a GPU"
    torch.cuda.init()
    eng = Engine(0)
    try:
        be = ResidentDevice(eng)
        A, B, stats = rt.run(be)
        conv.check_end(A, B, stats)
        assert be.calls == stats["calls"] == 4 * stats["rounds"]
        assert stats["codes"][3] == stats["codes"][5] == stats["codes"][6] == 0 and stats["window_closed"]["B"] == 0
        for e in (A, B):
            assert e.table.is_cuda and np.array_equal(be.read_table(e.table)["snd_nxt"], e.tx["snd_nxt"])
    finally:
        eng.close()
