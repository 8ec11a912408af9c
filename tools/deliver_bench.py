#!/usr/bin/env python3
"""In-order TCP delivery into socket rings against the flow-aware coalesce it builds on, in one
process on one GPU.

Shape (that of tools/coalesce_bench.py --flows 64): 65,536 TCP frames of 1500 B, device-resident,
built by fs_segment_batch as F flows of 65,536 / F frames each (a flow of more than 4,096 frames is
several sends with one header whose Seq continue), listed round-robin across the flows (A0 B0 ... A1
B1 ...), with F sockets whose rings hold the whole flow. Four things are timed with HIP events, one
event pair per call, over interleaved rounds of calls that rotate over distinct frame, payload and
rings buffers (more than the 256 MiB Infinity Cache holds in total):
  (a) fs_deliver_flows_batch with the packed payload;
  (b) fs_deliver_flows_batch with payload NULL (delivery only, no packed copy);
  (c) fs_coalesce_flows_batch of the same library on the same frames;
  (d) fs_deliver_flows_batch with n_socks 0 (the same launches as (c) plus the zeroing of `delivered`).
--flows 1 is the walk's worst case: one wave walks all 65,536 frames alone.
Prints the per-round medians, the medians over rounds with the rounds' spread, and one JSON line.

    python tools/deliver_bench.py [--flows 64] [--rounds 3] [--launches 100] [--buffers 4] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_SEND = 4096  # frames one send may produce


def tcp_template(rng, sport: int) -> bytearray:
    h = bytearray(rng.integers(0, 256, 54, dtype=np.uint8).tobytes())
    h[12:14], h[14], h[23], h[46], h[47] = b"\x08\x00", 0x45, 6, 0x50, 0x10
    h[34:36], h[36:38] = (1024 + sport % 60000).to_bytes(2, "big"), b"\x00\x50"
    return h


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--launches", type=int, default=100)
    p.add_argument("--buffers", type=int, default=4)
    p.add_argument("--frames", type=int, default=65536)
    p.add_argument("--mss", type=int, default=1446)
    p.add_argument("--flows", type=int, default=64, help="F flows, their frames interleaved round-robin, F sockets")
    p.add_argument("--out", default=None, help="also write the report to this file")
    a = p.parse_args()

    import torch

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    from seqs_amd import (FLOW_DTYPE, FLOW_TOTALS_DTYPE, RUN_DTYPE, SEND_DTYPE, SOCK_DTYPE, SOCK_OUT_DTYPE, Engine,
                          segment_layout, split_flows, split_socks)

    assert a.frames % a.flows == 0, "--flows must divide --frames"
    per_flow = a.frames // a.flows
    per_send = min(per_flow, MAX_SEND)
    assert per_flow % per_send == 0
    sends_per_flow = per_flow // per_send
    ring_size = per_flow * a.mss
    assert ring_size <= 1 << 31

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    n_sends = a.flows * sends_per_flow
    sends = np.zeros(n_sends, dtype=SEND_DTYPE)
    socks = np.zeros(a.flows, dtype=SOCK_DTYPE)
    for f in range(a.flows):
        h = tcp_template(rng, f)
        seq0 = int.from_bytes(h[38:42], "big")
        socks["key"][f] = np.frombuffer(bytes([6]) + bytes(h[26:38]), dtype=np.uint8)
        socks["rcv_nxt"][f], socks["snd_nxt"][f] = seq0, int.from_bytes(h[42:46], "big")
        for s in range(sends_per_flow):
            h[38:42] = ((seq0 + s * per_send * a.mss) % (1 << 32)).to_bytes(4, "big")
            sends["hdr"][f * sends_per_flow + s] = np.frombuffer(bytes(h), dtype=np.uint8)
    socks["rcv_wnd"], socks["ring_size"], socks["ring_free"] = 65535, ring_size, ring_size
    socks["ring_off"] = np.arange(a.flows, dtype=np.uint64) * np.uint64(ring_size)
    sends["mss"] = a.mss
    sends["payload_len"] = per_send * a.mss
    sends["payload_off"] = np.arange(n_sends, dtype=np.uint64) * np.uint64(per_send * a.mss)
    align = 4
    n_frames, frames_bytes = segment_layout(sends, 0, align)
    payload_bytes = a.frames * a.mss
    assert n_frames == a.frames

    eng = Engine(0)
    stream = torch.cuda.Stream(dev)
    src = torch.from_numpy(rng.integers(0, 256, payload_bytes, dtype=np.uint8)).to(dev)
    frames = [torch.empty(frames_bytes, dtype=torch.uint8, device=dev) for _ in range(a.buffers)]
    gathered = [torch.empty(payload_bytes, dtype=torch.uint8, device=dev) for _ in range(a.buffers)]
    rings = [torch.zeros(payload_bytes, dtype=torch.uint8, device=dev) for _ in range(a.buffers)]
    built = []
    with torch.cuda.stream(stream):
        for b in range(a.buffers):
            built.append(eng.segment_device(sends, src, 0, 0, align, stream=stream, frames=frames[b]))
    stream.synchronize()
    assert all(int(r[4].max()) == 0 for r in built), "a built frame is not FS_OK"
    # the interleaved descriptors: frame k of the batch is frame k // F of flow k % F
    k = torch.arange(n_frames, device=dev)
    perm = (k % a.flows) * per_flow + k // a.flows
    inter = [(built[b][1][perm].contiguous(), built[b][2][perm].contiguous()) for b in range(a.buffers)]

    runs = torch.empty((n_frames, RUN_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    flows_t = torch.empty((n_frames, FLOW_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    order_t = torch.empty((n_frames,), dtype=torch.int32, device=dev)
    run_of = torch.empty((n_frames,), dtype=torch.int32, device=dev)
    ftotals = torch.empty((FLOW_TOTALS_DTYPE.itemsize,), dtype=torch.uint8, device=dev)
    out = torch.empty((n_frames, 2), dtype=torch.int32, device=dev)
    status = torch.empty((n_frames,), dtype=torch.uint8, device=dev)
    socks_out = torch.empty((a.flows, SOCK_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    delivered = torch.empty((n_frames,), dtype=torch.uint8, device=dev)
    vp = ctypes.c_void_p

    def head(b):
        return (eng._ctx, vp(frames[b].data_ptr()), vp(inter[b][0].data_ptr()), vp(inter[b][1].data_ptr()), n_frames, 0, 0)

    def tail(b, packed):
        return ((vp(gathered[b].data_ptr()), payload_bytes) if packed else (None, 0)) + \
            (vp(runs.data_ptr()), vp(flows_t.data_ptr()), vp(order_t.data_ptr()), vp(run_of.data_ptr()),
             vp(ftotals.data_ptr()), vp(out.data_ptr()), vp(status.data_ptr()), vp(stream.cuda_stream))

    def sock_args(b, n_socks):
        return (vp(socks.ctypes.data), n_socks, vp(rings[b].data_ptr()), payload_bytes, vp(socks_out.data_ptr()),
                vp(delivered.data_ptr()))

    def deliver(n_socks, packed):
        args = [head(b) + sock_args(b, n_socks) + tail(b, packed) for b in range(a.buffers)]

        def run(b):
            st = eng.lib.fs_deliver_flows_batch(*args[b])
            assert st == 0, eng.lib.fs_last_error(eng._ctx)
        return run

    fl_args = [head(b) + tail(b, True) for b in range(a.buffers)]

    def run_flows(b):
        st = eng.lib.fs_coalesce_flows_batch(*fl_args[b])
        assert st == 0, eng.lib.fs_last_error(eng._ctx)

    kinds = [("deliver", deliver(a.flows, True)), ("deliver_nopayload", deliver(a.flows, False)), ("flows", run_flows),
             ("deliver_nosocks", deliver(0, True))]

    # every flow arrives whole in its ring, and the packed payload is what the flow call gives: checked once
    with torch.cuda.stream(stream):
        kinds[1][1](0)
    stream.synchronize()
    so = split_socks(socks_out)
    assert torch.equal(rings[0], src) and int(delivered.min()) == 1
    assert (so["bytes"] == ring_size).all() and (so["n_delivered"] == per_flow).all() and (so["ring_free"] == 0).all()
    gathered[0].zero_()
    with torch.cuda.stream(stream):
        kinds[0][1](0)
    stream.synchronize()
    _, _, _, ft = split_flows(runs, flows_t, order_t, ftotals)
    assert (int(ft["payload_bytes"]), int(ft["n_flows"]), int(ft["n_accepted"])) == (payload_bytes, a.flows, n_frames)
    assert torch.equal(gathered[0], src)

    def timed(fn, launches):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        with torch.cuda.stream(stream):
            for i, (e0, e1) in enumerate(ev):
                e0.record(stream)
                fn(i % a.buffers)
                e1.record(stream)
        stream.synchronize()
        return [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]  # us

    for _, fn in kinds:  # warm-up (also past the digest's automatic kernel choice window)
        timed(fn, 40)
    rounds = {name: [] for name, _ in kinds}
    lines = []
    for rd in range(a.rounds):
        for name, fn in kinds:
            rounds[name].append(statistics.median(timed(fn, a.launches)))
        lines.append(f"round {rd}: " + "  ".join(f"{name} {rounds[name][-1]:9.2f} us" for name, _ in kinds))
    med = {name: statistics.median(v) for name, v in rounds.items()}
    spread = {name: [round(min(v), 2), round(max(v), 2)] for name, v in rounds.items()}
    inside = spread["flows"][0] <= med["deliver_nosocks"] <= spread["flows"][1]
    res = {
        "shape": f"{n_frames} frames of {54 + a.mss} B in {a.flows} interleaved flows of {per_flow}, {a.flows} sockets, "
                 f"rings of {ring_size} B",
        "frames": n_frames, "flows": a.flows, "payload_bytes": payload_bytes, "buffers": a.buffers, "rounds": a.rounds,
        "launches_per_round": a.launches,
        "deliver_us": round(med["deliver"], 2), "deliver_nopayload_us": round(med["deliver_nopayload"], 2),
        "flows_us": round(med["flows"], 2), "deliver_nosocks_us": round(med["deliver_nosocks"], 2),
        "round_min_max_us": spread, "deliver_over_flows": round(med["deliver"] / med["flows"], 3),
        "nosocks_inside_flows_spread": bool(inside),
        "last_kernel": eng.last_kernel(), "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
    }
    lines.append(f"median of rounds [min, max]: (a) deliver {med['deliver']:.2f} us {spread['deliver']}  "
                 f"(b) deliver, payload NULL {med['deliver_nopayload']:.2f} us {spread['deliver_nopayload']}  "
                 f"(c) coalesce_flows {med['flows']:.2f} us {spread['flows']}  "
                 f"(d) deliver, n_socks 0 {med['deliver_nosocks']:.2f} us {spread['deliver_nosocks']}  "
                 f"(a) / (c) = {med['deliver'] / med['flows']:.3f}  (d) inside (c)'s rounds: {'yes' if inside else 'NO'}")
    lines.append(json.dumps(res))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("command: python " + " ".join(sys.argv) + "\n" + text + "\n")
    eng.close()


if __name__ == "__main__":
    main()
