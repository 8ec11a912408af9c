#!/usr/bin/env python3
"""The ring send from device-resident sockets (fs_send_rings_resident) against the host-socket call
(fs_send_rings_batch), in one process on one GPU, in interleaved rounds. Three shapes:

  (a) DESIGN.md §3.19's shape, 64 sockets x 1,024 frames of 1,500 B: the frame kernel is the same body in
      both calls, so the difference is the cost of the plan kernels. With --parent-lib the host-socket call
      of another build of the library (the parent commit's) is timed in the same rounds.
  (b) many small sockets: 65,536 sockets x one 1,446-byte segment, and 65,536 bare ACKs. Per call the device
      time between two HIP events, and the host wall time the call takes to return.
  (c) the turn: fs_recv_flows_batch, synchronise, copy socks_out and snd_out to the host, tx_sock_from,
      fs_send_rings_batch -- against fs_recv_flows_batch and fs_send_rings_resident back to back on one
      stream. Wall time from the first enqueue until the frames are complete, for 1,000 and 65,536 sockets.

Every pair of calls is first shown to build the same frames. Prints per-round medians, the medians over the
rounds with the rounds' range, and one JSON line per shape.

    python tools/send_resident_bench.py [--shapes abc] [--rounds 5] [--launches 60] [--parent-lib PATH] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
vp = ctypes.c_void_p
ALIGN = 4


def headers(rng, n):
    hdr = rng.integers(0, 256, (n, 54), dtype=np.uint8)
    hdr[:, 12], hdr[:, 13], hdr[:, 14], hdr[:, 23], hdr[:, 46] = 0x08, 0x00, 0x45, 6, 0x50
    hdr[:, 26:30] = (np.arange(n, dtype=np.uint32) + 0x0A000001).astype(">u4").view(np.uint8).reshape(-1, 4)  # distinct flows
    hdr[:, 34:38] = [0x12, 0x34, 0x00, 0x50]
    return hdr


def sockets(rng, n, frames, mss, buffered=None, flags=0):
    """n TX sockets of `frames` frames of mss bytes: full rings read from their middle."""
    from seqs_amd import TX_SOCK_DTYPE

    size = max(1, frames * mss)
    s = np.zeros(n, dtype=TX_SOCK_DTYPE)
    s["hdr"], s["mss"], s["ring_size"], s["ring_rpos"] = headers(rng, n), mss, size, size // 2
    s["ring_buffered"] = size if buffered is None else buffered
    s["ring_off"] = np.arange(n, dtype=np.uint64) * np.uint64(size)
    s["snd_una"] = s["snd_nxt"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    s["snd_wnd"], s["rcv_wnd"], s["max_frames"], s["flags"] = 0xFFFFFFFF, 65535, max(frames, 1), flags
    s["rcv_nxt"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return s, n * size


class Parent:
    """fs_send_rings_batch of another build of the library, with a context of its own."""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.fs_ctx_create.argtypes, self.lib.fs_ctx_create.restype = [ctypes.c_int, ctypes.POINTER(vp)], ctypes.c_int32
        self.lib.fs_send_rings_batch.restype, self.lib.fs_last_error.restype = ctypes.c_int32, ctypes.c_char_p
        self.lib.fs_send_rings_batch.argtypes = [vp, vp, ctypes.c_uint32, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                                 ctypes.c_uint32, vp, ctypes.c_uint64, vp, vp, vp, vp, vp, vp]
        self.lib.fs_last_error.argtypes, self.lib.fs_ctx_destroy.argtypes = [vp], [vp]
        self._ctx = vp()
        assert self.lib.fs_ctx_create(0, ctypes.byref(self._ctx)) == 0, self.lib.fs_last_error(None)

    def close(self):
        self.lib.fs_ctx_destroy(self._ctx)


class Tx:
    """One shape's buffers and the two calls over them."""

    def __init__(self, eng, torch, stream, socks, ring_bytes, buffers, parent=None):
        from seqs_amd import TX_SOCK_OUT_DTYPE, send_rings_layout, tx_socks_tensor

        dev = torch.device("cuda:0")
        self.eng, self.torch, self.stream, self.socks, self.n, self.parent = eng, torch, stream, socks, len(socks), parent
        self.n_frames, self.frames_bytes, self.expect = send_rings_layout(socks, 0, ALIGN)
        rng = np.random.default_rng(2)
        self.rings = [torch.from_numpy(rng.integers(0, 256, max(ring_bytes, 1), dtype=np.uint8)).to(dev) for _ in range(buffers)]
        self.frames = [torch.empty(self.frames_bytes, dtype=torch.uint8, device=dev) for _ in range(buffers)]
        k = self.n_frames
        self.arrays = (torch.empty((k,), dtype=torch.int64, device=dev), torch.empty((k,), dtype=torch.int32, device=dev),
                       torch.empty((k, 2), dtype=torch.int32, device=dev), torch.empty((k,), dtype=torch.uint8, device=dev))
        self.results = tuple(vp(t.data_ptr()) for t in self.arrays)
        self.table = tx_socks_tensor(socks, dev)
        self.socks_out = np.zeros(self.n, dtype=TX_SOCK_OUT_DTYPE)
        self.d_socks_out = torch.empty((self.n, 32), dtype=torch.uint8, device=dev)
        self.d_totals = torch.empty((40,), dtype=torch.uint8, device=dev)
        self.ring_bytes = max(ring_bytes, 1)

    def batch(self, b, who=None):
        who = who or self.eng
        st = who.lib.fs_send_rings_batch(who._ctx, vp(self.socks.ctypes.data), self.n, vp(self.rings[b].data_ptr()), self.ring_bytes,
                                         0, 0, ALIGN, vp(self.frames[b].data_ptr()), self.frames_bytes, *self.results,
                                         vp(self.socks_out.ctypes.data), vp(self.stream.cuda_stream))
        assert st == 0, who.lib.fs_last_error(who._ctx)

    def batch_parent(self, b):
        self.batch(b, self.parent)

    def resident(self, b, rx=(None, None)):
        st = self.eng.lib.fs_send_rings_resident(
            self.eng._ctx, vp(self.table.data_ptr()), self.n, rx[0], rx[1], None, self.n if rx[0] else 0,
            vp(self.rings[b].data_ptr()), self.ring_bytes, 0, 0, ALIGN, vp(self.frames[b].data_ptr()), self.frames_bytes,
            self.n_frames, *self.results, vp(self.d_socks_out.data_ptr()), vp(self.d_totals.data_ptr()), vp(self.stream.cuda_stream))
        assert st == 0, self.eng.lib.fs_last_error(self.eng._ctx)

    def same_frames(self):
        from seqs_amd import split_tx

        torch = self.torch
        with torch.cuda.stream(self.stream):
            self.frames[0].fill_(0x5A)  # (the bytes between the slots' frames are written by neither call)
            self.batch(0)
            self.stream.synchronize()
            want = (self.frames[0].clone(), *(t.clone() for t in self.arrays))
            self.frames[0].fill_(0x5A)
            self.resident(0)
            self.stream.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(want, (self.frames[0], *self.arrays))), "the frames differ"
        outs, tot = split_tx(self.d_socks_out, self.d_totals)
        assert np.array_equal(outs, self.expect) and int(tot["n_frames"]) == self.n_frames and int(tot["n_deferred"]) == 0


def timed(torch, stream, fn, launches, buffers):
    """(device us between two events, host us until the call returned) per launch."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    host = []
    with torch.cuda.stream(stream):
        for i, (e0, e1) in enumerate(ev):
            e0.record(stream)
            t0 = time.perf_counter()
            fn(i % buffers)
            host.append((time.perf_counter() - t0) * 1e6)
            e1.record(stream)
            if i % 8 == 7:
                stream.synchronize()  # (the host-socket call has 32 staging blocks: neither call queues behind them)
    stream.synchronize()
    return [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev], host


def rounds_of(torch, stream, kinds, rounds, launches, buffers, lines, label):
    for _, fn in kinds:
        timed(torch, stream, fn, 16, buffers)
    dev_us, host_us = {k: [] for k, _ in kinds}, {k: [] for k, _ in kinds}
    for rd in range(rounds):
        order = kinds if rd % 2 == 0 else kinds[::-1]  # alternate who goes first
        for name, fn in order:
            d, h = timed(torch, stream, fn, launches, buffers)
            dev_us[name].append(statistics.median(d))
            host_us[name].append(statistics.median(h))
        lines.append(f"{label} round {rd}: " + "  ".join(f"{k} {dev_us[k][-1]:9.2f} us (host {host_us[k][-1]:8.2f})" for k, _ in kinds))
    return {k: {"device_us": round(statistics.median(dev_us[k]), 2), "device_range": [round(min(dev_us[k]), 2), round(max(dev_us[k]), 2)],
                "host_us": round(statistics.median(host_us[k]), 2), "host_range": [round(min(host_us[k]), 2), round(max(host_us[k]), 2)]}
            for k, _ in kinds}


def shape_a(a, eng, torch, stream, parent, lines):
    rng = np.random.default_rng(1)
    socks, ring_bytes = sockets(rng, 64, 1024, 1446)
    tx = Tx(eng, torch, stream, socks, ring_bytes, 4, parent)
    tx.same_frames()
    kinds = [("resident", tx.resident), ("batch", tx.batch)] + ([("batch_parent", tx.batch_parent)] if parent else [])
    r = rounds_of(torch, stream, kinds, a.rounds, a.launches, 4, lines, "(a)")
    ref = r["batch_parent" if parent else "batch"]
    cost = round(r["resident"]["device_us"] - ref["device_us"], 2)
    noise = round(ref["device_range"][1] - ref["device_range"][0], 2)
    res = {"shape": "a: 64 sockets x 1024 frames of 1500 B", "frames": tx.n_frames, **{k: v for k, v in r.items()},
           "against": "parent library" if parent else "this library", "plan_cost_us": cost, "yardstick_range_us": noise,
           "inside_noise": bool(abs(cost) <= noise)}
    lines.append(f"(a) resident {r['resident']['device_us']} us, host-socket call {ref['device_us']} us {ref['device_range']}: "
                 f"the plan kernels cost {cost} us; the yardstick's own range of per-round medians is {noise} us")
    return res


def shape_b(a, eng, torch, stream, lines):
    out = []
    for label, frames, mss, flags in (("65536 sockets x one 1446-byte segment", 1, 1446, 0), ("65536 bare ACKs", 0, 1446, 1)):
        rng = np.random.default_rng(3)
        socks, ring_bytes = sockets(rng, 65536, frames, mss, buffered=None if frames else 0, flags=flags)
        tx = Tx(eng, torch, stream, socks, ring_bytes if frames else 65536, 3)
        tx.same_frames()
        r = rounds_of(torch, stream, [("resident", tx.resident), ("batch", tx.batch)], a.rounds, max(10, a.launches // 3), 3, lines,
                      "(b) " + label)
        lines.append(f"(b) {label}: device us resident {r['resident']['device_us']} {r['resident']['device_range']} / batch "
                     f"{r['batch']['device_us']} {r['batch']['device_range']}; host us of the call resident {r['resident']['host_us']} "
                     f"{r['resident']['host_range']} / batch {r['batch']['host_us']} {r['batch']['host_range']}")
        out.append({"shape": "b: " + label, "frames": tx.n_frames, **r})
    return out


def shape_c(a, eng, torch, stream, lines):
    from seqs_amd import SND_DTYPE, SOCK_DTYPE, split_snd, split_socks, tx_sock_from

    out = []
    dev = torch.device("cuda:0")
    for n in (1000, 65536):
        rng = np.random.default_rng(4)
        # the peers' frames: one 64-byte segment to each of our sockets (built by the host-socket call)
        peers, peer_bytes = sockets(rng, n, 1, 64)
        peers["rcv_nxt"] = rng.integers(0, 1 << 30, n).astype(np.uint32)
        ptx = Tx(eng, torch, stream, peers, peer_bytes, 1)
        with torch.cuda.stream(stream):
            ptx.batch(0)
        stream.synchronize()
        in_frames, in_off, in_len = ptx.frames[0], ptx.arrays[0], ptx.arrays[1]
        rx = np.zeros(n, dtype=SOCK_DTYPE)
        rx["key"][:, 0], rx["key"][:, 1:9], rx["key"][:, 9:13] = 6, peers["hdr"][:, 26:34], peers["hdr"][:, 34:38]
        rx["rcv_nxt"], rx["rcv_wnd"], rx["snd_nxt"] = peers["snd_nxt"], 65535, peers["rcv_nxt"]
        rx["ring_size"], rx["ring_free"], rx["ring_off"] = 4096, 4096, np.arange(n, dtype=np.uint64) * np.uint64(4096)
        snd = np.zeros(n, dtype=SND_DTYPE)
        snd["snd_una"], snd["snd_wnd"] = peers["rcv_nxt"], 65535
        rx_rings = torch.zeros(n * 4096, dtype=torch.uint8, device=dev)
        # our answer: the owed ACK on one 1,446-byte segment per socket
        mine, ring_bytes = sockets(rng, n, 1, 1446)
        mine["snd_una"] = mine["snd_nxt"] = peers["rcv_nxt"]
        tx = Tx(eng, torch, stream, mine, ring_bytes, 1)

        def recv():
            r = eng.recv_flows_device(in_frames, in_off, in_len, rx, snd, rx_rings, payload=False, delivered=False, code=False,
                                      stream=stream)
            return r[0], r[2]  # snd_out, socks_out

        def host_turn():
            snd_out, socks_out = recv()
            stream.synchronize()
            tx.socks = tx_sock_from(split_socks(socks_out), mine, snd_out=split_snd(snd_out))
            tx.batch(0)
            stream.synchronize()

        def resident_turn():
            snd_out, socks_out = recv()
            tx.resident(0, (vp(socks_out.data_ptr()), vp(snd_out.data_ptr())))
            stream.synchronize()

        with torch.cuda.stream(stream):
            tx.frames[0].fill_(0x5A)
            host_turn()
            want = (tx.frames[0].clone(), *(t.clone() for t in tx.arrays))
            tx.frames[0].fill_(0x5A)
            resident_turn()
            assert all(torch.equal(x, y) for x, y in zip(want, (tx.frames[0], *tx.arrays))), "the turns' frames differ"
            assert int(tx.arrays[3].max()) == 0
            kinds, wall = [("host_turn", host_turn), ("resident_turn", resident_turn)], {"host_turn": [], "resident_turn": []}
            for rd in range(a.rounds):
                for name, fn in (kinds if rd % 2 == 0 else kinds[::-1]):
                    ts = []
                    for _ in range(max(5, a.launches // 6)):
                        t0 = time.perf_counter()
                        fn()
                        ts.append((time.perf_counter() - t0) * 1e6)
                    wall[name].append(statistics.median(ts))
                lines.append(f"(c) {n} sockets round {rd}: " + "  ".join(f"{k} {wall[k][-1]:10.2f} us" for k, _ in kinds))
        med = {k: round(statistics.median(v), 2) for k, v in wall.items()}
        rng_ = {k: [round(min(v), 2), round(max(v), 2)] for k, v in wall.items()}
        lines.append(f"(c) {n} sockets: wall us first enqueue to frames complete: host turn {med['host_turn']} {rng_['host_turn']}, "
                     f"resident turn {med['resident_turn']} {rng_['resident_turn']}")
        out.append({"shape": f"c: the turn, {n} sockets", "wall_us": med, "wall_range_us": rng_})
    return out


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="abc")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--launches", type=int, default=60)
    p.add_argument("--parent-lib", default=None, help="another build of libframesum.so whose fs_send_rings_batch shape (a) times too")
    p.add_argument("--out", default=None, help="also write the report to this file")
    a = p.parse_args()

    import torch

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    from seqs_amd import Engine

    eng = Engine(0)
    parent = Parent(a.parent_lib) if a.parent_lib else None
    stream = torch.cuda.Stream(torch.device("cuda:0"))
    lines, results = [], []
    if "a" in a.shapes:
        results.append(shape_a(a, eng, torch, stream, parent, lines))
    if "b" in a.shapes:
        results += shape_b(a, eng, torch, stream, lines)
    if "c" in a.shapes:
        results += shape_c(a, eng, torch, stream, lines)
    for r in results:
        r.update(device=torch.cuda.get_device_name(0), hip=torch.version.hip)
        lines.append(json.dumps(r))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("command: python " + " ".join(sys.argv) + "\n" + text + "\n")
    if parent:
        parent.close()
    eng.close()


if __name__ == "__main__":
    main()
