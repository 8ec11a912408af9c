#!/usr/bin/env python3
"""The UDP call against the connect call it builds on, in one process on one GPU, from the same library on the
same frames, payload NULL in both, no sockets, listeners, closers or openers in either.

Shapes:
  a    the reference's benchmark (stacks/benchmark_test.go:12-46): 65,536 frames of 47 bytes (5 payload bytes)
       from random sources to port 67 of one address, one port with 65,536 cells of 40 bytes: the 4-lane copy.
  a16  shape a's frames into cells of 104 bytes, which is the smallest cell the 16-lane copy serves: the same
       bytes written by the other copy kernel, to compare the two group widths.
  b    65,536 frames of 1,500 bytes to 64 ports of 1,024 cells of 1,504 bytes (1,458 payload bytes each).
  c    shape b's frames with n_ports 0: the call adds the fills of port_of and cell_of alone.
Timed with HIP events, one event pair per call, over interleaved rounds of calls that rotate over distinct
frame buffers (the method of tools/connect_bench.py). Prints the per-round medians, the medians over rounds
with the rounds' spread, and one JSON line. For shape c it also says whether udp - connect lies within the
spread of the connect call's own rounds plus the two fills, which it times on their own.

    python tools/udp_bench.py --shape a|a16|b|c [--rounds 3] [--launches 100] [--buffers 4] [--out FILE]
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

N = 65536
LOCAL_IP = (10, 0, 0, 1)


def datagrams(rng, frame_len, n_ports):
    """N valid UDP frames of frame_len bytes from random sources to LOCAL_IP, frame k to port 67 + k % n_ports,
    at a stride of frame_len rounded up to 4 bytes: (buffer, offsets, lengths)."""
    from oracle import coracle
    from seqs_amd import synth

    stride = (frame_len + 3) & ~3
    rows = np.zeros((N, stride), dtype=np.uint8)
    rows[:, :frame_len] = synth.make_frames(N, frame_len, 17, rng)
    port = 67 + np.arange(N) % max(n_ports, 1)
    rows[:, 30:34] = LOCAL_IP
    rows[:, 36], rows[:, 37] = port >> 8, port & 0xFF
    flat = np.concatenate([rows.reshape(-1), np.zeros(64, dtype=np.uint8)])
    off, ln = (np.arange(N, dtype=np.uint64) * stride), np.full(N, frame_len, dtype=np.uint32)
    _, st = coracle.fill_batch(flat, off, ln, 0, coracle.FILL_CSUM)
    assert not st.any()
    return flat, off, ln


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--shape", choices=("a", "a16", "b", "c"), required=True)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--launches", type=int, default=100)
    p.add_argument("--buffers", type=int, default=4)
    p.add_argument("--out", default=None, help="also write the report to this file")
    a = p.parse_args()

    import torch

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    from seqs_amd import (CLOSE_OUT_DTYPE, CLOSER_DTYPE, CONNECT_OUT_DTYPE, FLOW_DTYPE, FLOW_TOTALS_DTYPE, OPENER_DTYPE, RUN_DTYPE,
                          SND_DTYPE, SND_OUT_DTYPE, SOCK_DTYPE, SOCK_OUT_DTYPE, UDP_PORT_DTYPE, UDP_PORT_OUT_DTYPE, Engine, udp_port)

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    eng = Engine(0)
    stream = torch.cuda.Stream(dev)

    if a.shape in ("a", "a16"):
        frame_len, listed, n_cells, cell_size = 47, 1, N, 40 if a.shape == "a" else 104
    else:
        frame_len, listed, n_cells, cell_size = 1500, 64, 1024, 1504
    buf, off, ln = datagrams(rng, frame_len, listed)
    n_ports = 0 if a.shape == "c" else listed
    ports = np.concatenate([udp_port(bytes(LOCAL_IP), 67 + k, n_cells, cell_size, k * n_cells * cell_size) for k in range(listed)])[:n_ports]
    ports = np.ascontiguousarray(ports, dtype=UDP_PORT_DTYPE)
    cells_bytes = max(8, listed * n_cells * cell_size)
    frames = [torch.from_numpy(buf).to(dev) for _ in range(a.buffers)]
    d_off, d_len = torch.from_numpy(off.astype(np.int64)).to(dev), torch.from_numpy(ln.astype(np.int32)).to(dev)
    rings = torch.zeros(64, dtype=torch.uint8, device=dev)

    def empty(shape, dtype=torch.uint8):
        return torch.empty(shape, dtype=dtype, device=dev)

    runs, flows_t = empty((N, RUN_DTYPE.itemsize)), empty((N, FLOW_DTYPE.itemsize))
    order_t, run_of = empty((N,), torch.int32), empty((N,), torch.int32)
    ftotals, out, status = empty((FLOW_TOTALS_DTYPE.itemsize,)), empty((N, 2), torch.int32), empty((N,))
    socks, snd = np.zeros(0, dtype=SOCK_DTYPE), np.zeros(0, dtype=SND_DTYPE)
    closers, openers = np.zeros(0, dtype=CLOSER_DTYPE), np.zeros(0, dtype=OPENER_DTYPE)
    socks_out, snd_out = empty((1, SOCK_OUT_DTYPE.itemsize)), empty((1, SND_OUT_DTYPE.itemsize))
    delivered, code, accept_of = empty((N,)), empty((N,)), empty((N,), torch.int32)
    closers_out, socks_close = empty((1, CLOSE_OUT_DTYPE.itemsize)), empty((1, CLOSE_OUT_DTYPE.itemsize))
    ctl_code = empty((N,))
    openers_out = empty((1, CONNECT_OUT_DTYPE.itemsize))
    replies = torch.zeros((64,), dtype=torch.uint8, device=dev)
    reply_out, reply_status = empty((1, 2), torch.int32), empty((1,))
    cells = torch.zeros((cells_bytes,), dtype=torch.uint8, device=dev)
    ports_out = empty((max(n_ports, 1), UDP_PORT_OUT_DTYPE.itemsize))
    port_of, cell_of = empty((N,), torch.int32), empty((N,), torch.int32)
    vp = ctypes.c_void_p

    def args_of(b, udp):
        head = (eng._ctx, vp(frames[b].data_ptr()), vp(d_off.data_ptr()), vp(d_len.data_ptr()), N, 0, 0,
                vp(socks.ctypes.data), 0, vp(rings.data_ptr()), 64, vp(socks_out.data_ptr()), vp(delivered.data_ptr()),
                vp(snd.ctypes.data), vp(snd_out.data_ptr()), vp(code.data_ptr()))
        listen = (None, 0, None, 0, 0, None, None, vp(accept_of.data_ptr()), None, None, None)
        mid = (None, 0, vp(closers_out.data_ptr()), vp(socks_close.data_ptr()), vp(ctl_code.data_ptr()))
        opening = (None, 0, 0, vp(openers_out.data_ptr()), vp(replies.data_ptr()), vp(reply_out.data_ptr()), vp(reply_status.data_ptr()))
        more = (vp(ports.ctypes.data) if n_ports else None, n_ports, vp(cells.data_ptr()), cells_bytes, vp(ports_out.data_ptr()),
                vp(port_of.data_ptr()), vp(cell_of.data_ptr())) if udp else ()
        tail = (None, 0, vp(runs.data_ptr()), vp(flows_t.data_ptr()), vp(order_t.data_ptr()), vp(run_of.data_ptr()),
                vp(ftotals.data_ptr()), vp(out.data_ptr()), vp(status.data_ptr()), vp(stream.cuda_stream))
        return head + listen + mid + opening + more + tail

    def kind(udp):
        fn = eng.lib.fs_udp_flows_batch if udp else eng.lib.fs_connect_flows_batch
        args = [args_of(b, udp) for b in range(a.buffers)]

        def run(b):
            st = fn(*args[b])
            assert st == 0, eng.lib.fs_last_error(eng._ctx)
        return run

    def fills(b):  # what shape c adds, on its own: the two fills of n 32-bit entries
        port_of.fill_(-1)
        cell_of.fill_(-1)

    kinds = [("udp", kind(True)), ("connect", kind(False))] + ([("fills", fills)] if a.shape == "c" else [])

    # checked once: the shape does what it says
    with torch.cuda.stream(stream):
        kinds[0][1](0)
    stream.synchronize()
    assert int(status.max()) == 0
    po, co = port_of.cpu().numpy(), cell_of.cpu().numpy()
    if n_ports == 0:
        assert (po == -1).all() and (co == -1).all()
    else:
        want_port = np.arange(N) % n_ports
        assert (po == want_port).all() and (co == np.arange(N) // n_ports).all()
        o = ports_out.cpu().numpy().reshape(-1).view(UDP_PORT_OUT_DTYPE)
        assert (o["n_admitted"] == N // n_ports).all() and (o["n_truncated"] == 0).all()
        assert int(o["bytes"].sum()) == N * (frame_len - 42)
        got = cells.cpu().numpy()
        k = N - 1  # the last frame's cell: its header's batch index and its payload
        at = int(ports[k % n_ports]["cells_off"]) + (k // n_ports) * cell_size
        assert int(got[at : at + 4].view("<u4")[0]) == k
        assert (got[at + 32 : at + 32 + frame_len - 42] == buf[int(off[k]) + 42 : int(off[k]) + frame_len]).all()

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
    diff = med["udp"] - med["connect"]
    res = {
        "shape": a.shape, "frames": N, "frame_len": frame_len, "n_ports": n_ports, "cell_size": cell_size,
        "buffers": a.buffers, "rounds": a.rounds, "launches_per_round": a.launches,
        **{name + "_us": round(v, 2) for name, v in med.items()}, "round_min_max_us": spread,
        "udp_minus_connect_us": round(diff, 2), "udp_over_connect": round(med["udp"] / med["connect"], 3),
        "last_kernel": eng.last_kernel(), "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
    }
    lines.append("median of rounds [min, max]: " + "  ".join(f"{name} {med[name]:.2f} us {spread[name]}" for name, _ in kinds) +
                 f"  udp - connect = {diff:.2f} us")
    if a.shape == "c":
        bound = (spread["connect"][1] - spread["connect"][0]) + spread["fills"][1]
        res["bound_us"], res["within_bound"] = round(bound, 2), bool(diff <= bound)
        lines.append(f"bound: the connect rounds' spread {spread['connect'][1] - spread['connect'][0]:.2f} us + the two fills "
                     f"{spread['fills'][1]:.2f} us = {bound:.2f} us; udp - connect = {diff:.2f} us: "
                     f"{'within' if diff <= bound else 'OUTSIDE'} the bound")
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
