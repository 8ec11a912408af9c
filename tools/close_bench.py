#!/usr/bin/env python3
"""The close call against the accept call it builds on, in one process on one GPU, from the same library on
the same frames, payload NULL in both, no listeners in either.

Shapes:
  a  65,536 one-frame flows, each a FIN | ACK of 54 bytes to a closer in FinWait1 that it takes to
     TimeWait: 65,536 closers, one walk of one frame each.
  b  the 64-flow shape of tools/recv_bench.py (65,536 data frames of 1500 B in 64 interleaved flows, 64
     sockets whose rings hold the whole flow) with n_closers 0 and no FIN or RST in the batch: what the
     call costs when nobody closes (64 continuations that find nothing to do).
  c  64 closers in CloseWait with 1,024 pure ACKs of 54 bytes each, interleaved: 64 walks of 16 chunks.
Timed with HIP events, one event pair per call, over interleaved rounds of calls that rotate over distinct
frame and rings buffers (the method of tools/accept_bench.py). Prints the per-round medians, the medians
over rounds with the rounds' spread, and one JSON line.

    python tools/close_bench.py --shape a|b|c [--rounds 3] [--launches 100] [--buffers 4] [--out FILE]
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

from deliver_bench import MAX_SEND, tcp_template  # noqa: E402

N, FLOWS, MSS = 65536, 64, 1446
LOCAL_IP = bytes([10, 0, 0, 1])
SND_NXT = 5000


def control_frames(rng, n_flows, flags):
    """N frames of 54 bytes without payload, 64 apart, in n_flows flows (frame k belongs to flow k % n_flows
    and carries Seq 77, Ack SND_NXT, `flags`): (buffer, offsets, lengths, the flows' keys)."""
    from oracle import coracle

    h = bytearray(tcp_template(rng, 0))
    h[16:18], h[30:34], h[42:46], h[46], h[47] = (40).to_bytes(2, "big"), LOCAL_IP, SND_NXT.to_bytes(4, "big"), 0x50, flags
    rows = np.zeros((N, 64), dtype=np.uint8)
    rows[:, :54] = np.frombuffer(bytes(h), dtype=np.uint8)
    k = np.arange(N, dtype=np.int64)
    f = k % n_flows
    rows[:, 28], rows[:, 29] = 1 + f // 60000, 1 + f % 250
    rows[:, 34], rows[:, 35] = (f % 60000 + 1) >> 8, (f % 60000 + 1) & 0xFF
    rows[:, 38:42] = (0, 0, 0, 77)
    off, ln = (k * 64).astype(np.uint64), np.full(N, 54, dtype=np.uint32)
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
    from seqs_amd import (CLOSE_OUT_DTYPE, CLOSER_DTYPE, FLOW_DTYPE, FLOW_TOTALS_DTYPE, RUN_DTYPE, SEND_DTYPE, SND_DTYPE,
                          SND_OUT_DTYPE, SOCK_DTYPE, SOCK_OUT_DTYPE, Engine, segment_layout, split_close, split_socks)

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    eng = Engine(0)
    stream = torch.cuda.Stream(dev)

    if a.shape in ("a", "c"):
        n_flows = N if a.shape == "a" else FLOWS
        buf, off, ln, keys = control_frames(rng, n_flows, 0x11 if a.shape == "a" else 0x10)
        closers = np.zeros(n_flows, dtype=CLOSER_DTYPE)
        closers["key"], closers["state"], closers["rcv_nxt"], closers["rcv_wnd"] = keys, 5 if a.shape == "a" else 9, 77, 65535
        closers["snd_una"], closers["snd_nxt"], closers["snd_wnd"] = SND_NXT - 100, SND_NXT, 1000
        n_socks, socks, snd, rings_bytes = 0, np.zeros(0, dtype=SOCK_DTYPE), np.zeros(0, dtype=SND_DTYPE), 64
        frames = [torch.from_numpy(buf).to(dev) for _ in range(a.buffers)]
        desc = [(torch.from_numpy(off.astype(np.int64)).to(dev), torch.from_numpy(ln.astype(np.int32)).to(dev))] * a.buffers
        rings = [torch.zeros(64, dtype=torch.uint8, device=dev) for _ in range(a.buffers)]
    else:
        # tools/accept_bench.py's shape b: F flows of data frames built by fs_segment_batch
        closers = np.zeros(0, dtype=CLOSER_DTYPE)
        per_flow = N // FLOWS
        per_send = min(per_flow, MAX_SEND)
        sends_per_flow = per_flow // per_send
        ring_size = per_flow * MSS
        n_sends, n_socks = FLOWS * sends_per_flow, FLOWS
        sends, socks, snd = np.zeros(n_sends, dtype=SEND_DTYPE), np.zeros(FLOWS, dtype=SOCK_DTYPE), np.zeros(FLOWS, dtype=SND_DTYPE)
        for f in range(FLOWS):
            h = tcp_template(rng, f)
            seq0, ack0 = int.from_bytes(h[38:42], "big"), int.from_bytes(h[42:46], "big")
            socks["key"][f] = np.frombuffer(bytes([6]) + bytes(h[26:38]), dtype=np.uint8)
            socks["rcv_nxt"][f], socks["snd_nxt"][f] = seq0, (ack0 + (1 << 20)) % (1 << 32)
            snd["snd_una"][f], snd["snd_wnd"][f] = ack0, 1000
            for s in range(sends_per_flow):
                h[38:42] = ((seq0 + s * per_send * MSS) % (1 << 32)).to_bytes(4, "big")
                sends["hdr"][f * sends_per_flow + s] = np.frombuffer(bytes(h), dtype=np.uint8)
        socks["rcv_wnd"], socks["ring_size"], socks["ring_free"] = 65535, ring_size, ring_size
        socks["ring_off"] = np.arange(FLOWS, dtype=np.uint64) * np.uint64(ring_size)
        sends["mss"], sends["payload_len"] = MSS, per_send * MSS
        sends["payload_off"] = np.arange(n_sends, dtype=np.uint64) * np.uint64(per_send * MSS)
        n_built, data_bytes = segment_layout(sends, 0, 4)
        assert n_built == N
        rings_bytes = N * MSS
        src = torch.from_numpy(rng.integers(0, 256, rings_bytes, dtype=np.uint8)).to(dev)
        frames = [torch.empty(data_bytes + 64, dtype=torch.uint8, device=dev) for _ in range(a.buffers)]
        rings = [torch.zeros(rings_bytes, dtype=torch.uint8, device=dev) for _ in range(a.buffers)]
        with torch.cuda.stream(stream):
            built = [eng.segment_device(sends, src, 0, 0, 4, stream=stream, frames=frames[b][:data_bytes]) for b in range(a.buffers)]
        stream.synchronize()
        k = torch.arange(N, device=dev)
        j = (k % FLOWS) * per_flow + k // FLOWS  # slot t of flow f is batch frame t * F + f
        desc = [(built[b][1][j].contiguous(), built[b][2][j].contiguous()) for b in range(a.buffers)]
    n_closers = int(closers.size)

    def empty(shape, dtype=torch.uint8):
        return torch.empty(shape, dtype=dtype, device=dev)

    runs, flows_t = empty((N, RUN_DTYPE.itemsize)), empty((N, FLOW_DTYPE.itemsize))
    order_t, run_of = empty((N,), torch.int32), empty((N,), torch.int32)
    ftotals, out, status = empty((FLOW_TOTALS_DTYPE.itemsize,)), empty((N, 2), torch.int32), empty((N,))
    socks_out, snd_out = empty((max(n_socks, 1), SOCK_OUT_DTYPE.itemsize)), empty((max(n_socks, 1), SND_OUT_DTYPE.itemsize))
    delivered, code, accept_of = empty((N,)), empty((N,)), empty((N,), torch.int32)
    closers_out, socks_close = empty((max(n_closers, 1), CLOSE_OUT_DTYPE.itemsize)), empty((max(n_socks, 1), CLOSE_OUT_DTYPE.itemsize))
    ctl_code = empty((N,))
    vp = ctypes.c_void_p

    def args_of(b, close):
        head = (eng._ctx, vp(frames[b].data_ptr()), vp(desc[b][0].data_ptr()), vp(desc[b][1].data_ptr()), N, 0, 0,
                vp(socks.ctypes.data), n_socks, vp(rings[b].data_ptr()), rings_bytes, vp(socks_out.data_ptr()),
                vp(delivered.data_ptr()), vp(snd.ctypes.data), vp(snd_out.data_ptr()), vp(code.data_ptr()))
        listen = (None, 0, None, 0, 0, None, None, vp(accept_of.data_ptr()), None, None, None)
        mid = (vp(closers.ctypes.data) if n_closers else None, n_closers, vp(closers_out.data_ptr()), vp(socks_close.data_ptr()),
               vp(ctl_code.data_ptr())) if close else ()
        tail = (None, 0, vp(runs.data_ptr()), vp(flows_t.data_ptr()), vp(order_t.data_ptr()), vp(run_of.data_ptr()),
                vp(ftotals.data_ptr()), vp(out.data_ptr()), vp(status.data_ptr()), vp(stream.cuda_stream))
        return head + listen + mid + tail

    def kind(close):
        fn = eng.lib.fs_close_flows_batch if close else eng.lib.fs_accept_flows_batch
        args = [args_of(b, close) for b in range(a.buffers)]

        def run(b):
            st = fn(*args[b])
            assert st == 0, eng.lib.fs_last_error(eng._ctx)
        return run

    kinds = [("close", kind(True)), ("accept", kind(False))]

    # checked once: the shape does what it says
    with torch.cuda.stream(stream):
        kinds[0][1](0)
    stream.synchronize()
    co, sc, ctl = split_close(closers_out[:n_closers], socks_close[:n_socks], ctl_code)
    assert int(status.max()) == 0
    if a.shape == "a":
        assert (co["state"] == 8).all() and (co["n_taken"] == 1).all() and (co["flags"] == 3).all() and (ctl == 1).all()
    elif a.shape == "c":
        assert (co["state"] == 9).all() and (co["n_taken"] == N // FLOWS).all() and (co["snd_una"] == SND_NXT).all() and (ctl == 1).all()
    else:
        assert (sc["state"] == 4).all() and not ctl.any() and (split_socks(socks_out)["n_delivered"] == N // FLOWS).all()
        assert torch.equal(rings[0], src)

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
        "shape": a.shape, "frames": N, "n_socks": n_socks, "n_closers": n_closers,
        "buffers": a.buffers, "rounds": a.rounds, "launches_per_round": a.launches,
        **{name + "_us": round(v, 2) for name, v in med.items()}, "round_min_max_us": spread,
        "close_minus_accept_us": round(med["close"] - med["accept"], 2), "close_over_accept": round(med["close"] / med["accept"], 3),
        "last_kernel": eng.last_kernel(), "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
    }
    lines.append("median of rounds [min, max]: " + "  ".join(f"{name} {med[name]:.2f} us {spread[name]}" for name, _ in kinds) +
                 f"  close - accept = {med['close'] - med['accept']:.2f} us")
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
