#!/usr/bin/env python3
"""The connect call against the close call it builds on, in one process on one GPU, from the same library on
the same frames, payload NULL in both, no listeners and no sockets in either.

Shapes:
  a  nobody dialing: 64 closers in CloseWait with 1,024 pure ACKs of 54 bytes each (tools/close_bench.py's
     shape c) and n_openers 0: the call adds no launch.
  b  64 openers whose flows are 1,024 rejected frames (Seq 5 under rcv.NXT 0) and one SYN-ACK, interleaved:
     65,600 frames, 64 walks of 17 chunks, 64 ACKs built.
  c  65,536 one-frame openers, each with its SYN-ACK: 65,536 walks of one frame, 65,536 ACKs built.
Timed with HIP events, one event pair per call, over interleaved rounds of calls that rotate over distinct
frame buffers (the method of tools/close_bench.py). Prints the per-round medians, the medians over rounds
with the rounds' spread, and one JSON line.

    python tools/connect_bench.py --shape a|b|c [--rounds 3] [--launches 100] [--buffers 4] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from deliver_bench import tcp_template  # noqa: E402

FLOWS = 64
LOCAL_IP = bytes([10, 0, 0, 1])
ISS = 4999


def control_frames(rng, n, n_flows, seq, flags):
    """n frames of 54 bytes without payload, 64 apart, in n_flows flows (frame k belongs to flow k % n_flows
    and carries Seq seq[k], Ack ISS + 1, flags[k]): (buffer, offsets, lengths, the flows' keys)."""
    from oracle import coracle

    h = bytearray(tcp_template(rng, 0))
    h[16:18], h[30:34], h[42:46], h[46] = (40).to_bytes(2, "big"), LOCAL_IP, (ISS + 1).to_bytes(4, "big"), 0x50
    rows = np.zeros((n, 64), dtype=np.uint8)
    rows[:, :54] = np.frombuffer(bytes(h), dtype=np.uint8)
    k = np.arange(n, dtype=np.int64)
    f = k % n_flows
    rows[:, 28], rows[:, 29] = 1 + f // 60000, 1 + f % 250
    rows[:, 34], rows[:, 35] = (f % 60000 + 1) >> 8, (f % 60000 + 1) & 0xFF
    rows[:, 38:42] = np.asarray(seq, dtype=">u4").reshape(n, 1).view(np.uint8)
    rows[:, 47] = flags
    off, ln = (k * 64).astype(np.uint64), np.full(n, 54, dtype=np.uint32)
    flat = rows.reshape(-1)
    _, st = coracle.fill_batch(flat, off, ln, 0, coracle.FILL_CSUM)
    assert not st.any()
    keys = np.concatenate([np.full((n_flows, 1), 6, dtype=np.uint8), rows[:n_flows, 26:38]], axis=1)
    return flat, off, ln, keys


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--shape", choices=("a", "b", "c"), required=True)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--launches", type=int, default=100)
    p.add_argument("--buffers", type=int, default=4)
    p.add_argument("--out", default=None, help="also write the report to this file")
    a = p.parse_args()

    import torch

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    from seqs_amd import (CLOSE_OUT_DTYPE, CLOSER_DTYPE, CONNECT_OUT_DTYPE, FLOW_DTYPE, FLOW_TOTALS_DTYPE, OPENER_DTYPE, RUN_DTYPE,
                          SND_DTYPE, SND_OUT_DTYPE, SOCK_DTYPE, SOCK_OUT_DTYPE, Engine, split_close, split_connect)

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    eng = Engine(0)
    stream = torch.cuda.Stream(dev)

    closers, openers = np.zeros(0, dtype=CLOSER_DTYPE), np.zeros(0, dtype=OPENER_DTYPE)
    if a.shape == "a":
        N = 65536
        buf, off, ln, keys = control_frames(rng, N, FLOWS, np.full(N, 77), 0x10)
        closers = np.zeros(FLOWS, dtype=CLOSER_DTYPE)
        closers["key"], closers["state"], closers["rcv_nxt"], closers["rcv_wnd"] = keys, 9, 77, 65535
        closers["snd_una"], closers["snd_nxt"], closers["snd_wnd"] = ISS - 100, ISS + 1, 1000
    else:
        per = 1025 if a.shape == "b" else 1
        n_flows = FLOWS if a.shape == "b" else 65536
        N = n_flows * per
        last = np.arange(N) // n_flows == per - 1
        buf, off, ln, keys = control_frames(rng, N, n_flows, np.where(last, 77, 5), np.where(last, 0x12, 0x10))
        openers = np.zeros(n_flows, dtype=OPENER_DTYPE)
        openers["key"], openers["iss"], openers["rcv_wnd"], openers["ip_id"] = keys, ISS, 65535, np.arange(n_flows) & 0xFFFF
        openers["local_mac"], openers["remote_mac"] = (2, 0, 0, 0, 0, 1), (2, 0, 0, 0, 0, 2)
    n_closers, n_openers = int(closers.size), int(openers.size)
    frames = [torch.from_numpy(buf).to(dev) for _ in range(a.buffers)]
    d_off, d_len = torch.from_numpy(off.astype(np.int64)).to(dev), torch.from_numpy(ln.astype(np.int32)).to(dev)
    rings = torch.zeros(64, dtype=torch.uint8, device=dev)

    def empty(shape, dtype=torch.uint8):
        return torch.empty(shape, dtype=dtype, device=dev)

    runs, flows_t = empty((N, RUN_DTYPE.itemsize)), empty((N, FLOW_DTYPE.itemsize))
    order_t, run_of = empty((N,), torch.int32), empty((N,), torch.int32)
    ftotals, out, status = empty((FLOW_TOTALS_DTYPE.itemsize,)), empty((N, 2), torch.int32), empty((N,))
    socks, snd = np.zeros(0, dtype=SOCK_DTYPE), np.zeros(0, dtype=SND_DTYPE)
    socks_out, snd_out = empty((1, SOCK_OUT_DTYPE.itemsize)), empty((1, SND_OUT_DTYPE.itemsize))
    delivered, code, accept_of = empty((N,)), empty((N,)), empty((N,), torch.int32)
    closers_out, socks_close = empty((max(n_closers, 1), CLOSE_OUT_DTYPE.itemsize)), empty((1, CLOSE_OUT_DTYPE.itemsize))
    ctl_code = empty((N,))
    openers_out = empty((max(n_openers, 1), CONNECT_OUT_DTYPE.itemsize))
    replies = torch.zeros((max(n_openers, 1) * 64,), dtype=torch.uint8, device=dev)
    reply_out, reply_status = empty((max(n_openers, 1), 2), torch.int32), empty((max(n_openers, 1),))
    vp = ctypes.c_void_p

    def args_of(b, connect):
        head = (eng._ctx, vp(frames[b].data_ptr()), vp(d_off.data_ptr()), vp(d_len.data_ptr()), N, 0, 0,
                vp(socks.ctypes.data), 0, vp(rings.data_ptr()), 64, vp(socks_out.data_ptr()), vp(delivered.data_ptr()),
                vp(snd.ctypes.data), vp(snd_out.data_ptr()), vp(code.data_ptr()))
        listen = (None, 0, None, 0, 0, None, None, vp(accept_of.data_ptr()), None, None, None)
        mid = (vp(closers.ctypes.data) if n_closers else None, n_closers, vp(closers_out.data_ptr()), vp(socks_close.data_ptr()),
               vp(ctl_code.data_ptr()))
        more = (vp(openers.ctypes.data) if n_openers else None, n_openers, 0, vp(openers_out.data_ptr()), vp(replies.data_ptr()),
                vp(reply_out.data_ptr()), vp(reply_status.data_ptr())) if connect else ()
        tail = (None, 0, vp(runs.data_ptr()), vp(flows_t.data_ptr()), vp(order_t.data_ptr()), vp(run_of.data_ptr()),
                vp(ftotals.data_ptr()), vp(out.data_ptr()), vp(status.data_ptr()), vp(stream.cuda_stream))
        return head + listen + mid + more + tail

    def kind(connect):
        fn = eng.lib.fs_connect_flows_batch if connect else eng.lib.fs_close_flows_batch
        args = [args_of(b, connect) for b in range(a.buffers)]

        def run(b):
            st = fn(*args[b])
            assert st == 0, eng.lib.fs_last_error(eng._ctx)
        return run

    kinds = [("connect", kind(True)), ("close", kind(False))]

    # checked once: the shape does what it says
    with torch.cuda.stream(stream):
        kinds[0][1](0)
    stream.synchronize()
    assert int(status.max()) == 0
    ctl = ctl_code.cpu().numpy()
    if a.shape == "a":
        co, _, _ = split_close(closers_out[:n_closers], socks_close[:0], ctl_code)
        assert (co["state"] == 9).all() and (co["n_taken"] == N // FLOWS).all() and (ctl == 1).all()
    else:
        oo, dig, rst = split_connect(openers_out, reply_out, reply_status)
        assert (oo["state"] == 4).all() and (oo["reply"] == 1).all() and (oo["n_rejected"] == (1024 if a.shape == "b" else 0)).all()
        assert not rst.any() and int((ctl == 1).sum()) == n_openers and int((ctl == 4).sum()) == N - n_openers
        got = replies.cpu().numpy().reshape(-1, 64)
        assert (got[:, 47] == 0x10).all() and (got[:, 38:42].copy().view(">u4")[:, 0] == ISS + 1).all()

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
    res = {
        "shape": a.shape, "frames": N, "n_closers": n_closers, "n_openers": n_openers,
        "buffers": a.buffers, "rounds": a.rounds, "launches_per_round": a.launches,
        **{name + "_us": round(v, 2) for name, v in med.items()}, "round_min_max_us": spread,
        "connect_minus_close_us": round(med["connect"] - med["close"], 2),
        "connect_over_close": round(med["connect"] / med["close"], 3),
        "last_kernel": eng.last_kernel(), "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
    }
    lines.append("median of rounds [min, max]: " + "  ".join(f"{name} {med[name]:.2f} us {spread[name]}" for name, _ in kinds) +
                 f"  connect - close = {med['connect'] - med['close']:.2f} us")
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
