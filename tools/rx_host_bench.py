#!/usr/bin/env python3
"""Wall clock per call of the four RX host forms (fs_coalesce_batch_host, fs_coalesce_flows_batch_host,
fs_deliver_flows_batch_host, fs_recv_flows_batch_host) in one process on one GPU, from and to pageable
numpy arrays: what a caller without device memory pays, the staging, the launches, the copies back
and the waits together.

Shape: 4,096 TCP frames of 1500 B built by fs_segment_batch_host as F flows of 4,096 / F frames,
listed round-robin across the flows, F sockets whose rings hold the whole flow. Every call goes
through the raw prototype with arrays allocated once. Prints, per call, the median of --calls calls
behind --warmup calls, and one JSON line.

    python tools/rx_host_bench.py [--flows 64] [--calls 100] [--warmup 5] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from deliver_bench import tcp_template  # noqa: E402


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=100)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--frames", type=int, default=4096)
    p.add_argument("--mss", type=int, default=1446)
    p.add_argument("--flows", type=int, default=64, help="F flows, their frames interleaved round-robin, F sockets")
    p.add_argument("--out", default=None, help="also write the report to this file")
    a = p.parse_args()

    import torch

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    from seqs_amd import (DIGEST_DTYPE, FLOW_DTYPE, FLOW_TOTALS_DTYPE, RUN_DTYPE, SEND_DTYPE, SND_DTYPE, SND_OUT_DTYPE,
                          SOCK_DTYPE, SOCK_OUT_DTYPE, TOTALS_DTYPE, Engine)

    assert a.frames % a.flows == 0 and a.frames // a.flows <= 4096, "--flows must divide --frames, one send per flow"
    n, per_flow = a.frames, a.frames // a.flows
    ring_size = per_flow * a.mss
    rng = np.random.default_rng(1)
    sends = np.zeros(a.flows, dtype=SEND_DTYPE)
    socks = np.zeros(a.flows, dtype=SOCK_DTYPE)
    snd = np.zeros(a.flows, dtype=SND_DTYPE)
    for f in range(a.flows):
        h = tcp_template(rng, f)
        socks["key"][f] = np.frombuffer(bytes([6]) + bytes(h[26:38]), dtype=np.uint8)
        socks["rcv_nxt"][f], socks["snd_nxt"][f] = int.from_bytes(h[38:42], "big"), int.from_bytes(h[42:46], "big")
        snd["snd_una"][f], snd["snd_wnd"][f] = (int(socks["snd_nxt"][f]) - 100) % (1 << 32), 1000
        sends["hdr"][f] = np.frombuffer(bytes(h), dtype=np.uint8)
    socks["rcv_wnd"], socks["ring_size"], socks["ring_free"] = 65535, ring_size, ring_size
    socks["ring_off"] = np.arange(a.flows, dtype=np.uint64) * np.uint64(ring_size)
    sends["mss"], sends["payload_len"] = a.mss, ring_size
    sends["payload_off"] = np.arange(a.flows, dtype=np.uint64) * np.uint64(ring_size)
    payload_bytes = n * a.mss
    src = rng.integers(0, 256, payload_bytes, dtype=np.uint8)

    eng = Engine(0)
    frames, off, ln, _, st = eng.segment_host(sends, src, 0, 0, 4)
    assert off.size == n and int(st.max()) == 0, "a built frame is not FS_OK"
    k = np.arange(n)
    perm = (k % a.flows) * per_flow + k // a.flows  # frame k of the batch is frame k // F of flow k % F
    off, ln = np.ascontiguousarray(off[perm], dtype=np.uint64), np.ascontiguousarray(ln[perm], dtype=np.uint32)

    gathered = np.zeros(payload_bytes, dtype=np.uint8)
    rings = np.zeros(payload_bytes, dtype=np.uint8)
    runs, flows_a = np.zeros(n, dtype=RUN_DTYPE), np.zeros(n, dtype=FLOW_DTYPE)
    order, run_of = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    totals, ftotals = np.zeros(1, dtype=TOTALS_DTYPE), np.zeros(1, dtype=FLOW_TOTALS_DTYPE)
    out, status = np.zeros(n, dtype=DIGEST_DTYPE), np.zeros(n, dtype=np.uint8)
    socks_out, snd_out = np.zeros(a.flows, dtype=SOCK_OUT_DTYPE), np.zeros(a.flows, dtype=SND_OUT_DTYPE)
    delivered, code = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    at = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    head = (eng._ctx, at(frames), frames.nbytes, at(off), at(ln), n, 0, 0)
    sock_args = (at(socks), a.flows, at(rings), rings.nbytes, at(socks_out), at(delivered))
    packed = (at(gathered), gathered.nbytes, at(runs))
    flow_tail = (at(flows_a), at(order), at(run_of), at(ftotals), at(out), at(status))
    calls = [
        ("fs_coalesce_batch_host", head + packed + (at(run_of), at(totals), at(out), at(status))),
        ("fs_coalesce_flows_batch_host", head + packed + flow_tail),
        ("fs_deliver_flows_batch_host", head + sock_args + packed + flow_tail),
        ("fs_recv_flows_batch_host", head + sock_args + (at(snd), at(snd_out), at(code)) + packed + flow_tail),
    ]
    med, lines = {}, []
    for name, args in calls:
        fn = getattr(eng.lib, name)
        times = []
        for i in range(a.warmup + a.calls):
            t0 = time.perf_counter_ns()
            rc = fn(*args)
            t1 = time.perf_counter_ns()
            assert rc == 0, eng.lib.fs_last_error(eng._ctx)
            if i >= a.warmup:
                times.append((t1 - t0) / 1e3)
        med[name] = statistics.median(times)
        lines.append(f"{name:30s} {med[name]:9.2f} us  (min {min(times):.2f}, max {max(times):.2f})")
    # checked once: the last call delivered every flow whole into its ring
    assert np.array_equal(rings, src) and (socks_out["n_delivered"] == per_flow).all() and int(code.min()) == 1
    assert int(ftotals["n_accepted"][0]) == n and int(ftotals["n_flows"][0]) == a.flows
    res = {"shape": f"{n} frames of {54 + a.mss} B in {a.flows} interleaved flows, {a.flows} sockets, pageable arrays",
           "calls": a.calls, "warmup": a.warmup, **{name + "_us": round(v, 2) for name, v in med.items()},
           "device": torch.cuda.get_device_name(0), "hip": torch.version.hip}
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
