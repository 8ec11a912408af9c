#!/usr/bin/env python3
"""The accept call against the receive call it builds on, in one process on one GPU, from the same library
on the same frames, payload NULL in both.

Shapes:
  a  65,536 one-frame SYN flows (58 bytes: an MSS option) to 64 listeners of 1,024 slots each, no sockets:
     every SYN opens a connection and gets its SYN-ACK.
  b  the 64-flow shape of tools/recv_bench.py (65,536 data frames of 1500 B in 64 interleaved flows, 64
     sockets whose rings hold the whole flow) with 64 listeners of 16 slots and no SYN in the batch: what
     listening costs when nobody connects.
  c  b with n_listeners 0: the accept call adds memsets only, so its difference from the receive call
     must lie inside the spread of the rounds.
Timed with HIP events, one event pair per call, over interleaved rounds of calls that rotate over
distinct frame and rings buffers (the method of tools/recv_bench.py). Prints the per-round medians, the
medians over rounds with the rounds' spread, and one JSON line.

    python tools/accept_bench.py --shape a|b|c [--rounds 3] [--launches 100] [--buffers 4] [--out FILE]
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
LOCAL_IP, MAC = bytes([10, 0, 0, 1]), bytes([2, 0, 0, 0, 0, 1])


def syn_frames(rng):
    """N SYNs of 58 bytes, 64 apart, to ports 1000 .. 1063 in turn: (buffer, offsets, lengths)."""
    from oracle import coracle

    h = bytearray(tcp_template(rng, 0))
    h[16:18], h[30:34], h[42:46], h[46], h[47] = (44).to_bytes(2, "big"), LOCAL_IP, bytes(4), 0x60, 0x02
    rows = np.zeros((N, 64), dtype=np.uint8)
    rows[:, :54] = np.frombuffer(bytes(h), dtype=np.uint8)
    rows[:, 54:58] = (2, 4, 5, 0xB4)
    k = np.arange(N, dtype=np.int64)
    rows[:, 28], rows[:, 29] = 1 + k // 60000, 1 + k % 250
    rows[:, 34], rows[:, 35] = (k % 60000 + 1) >> 8, (k % 60000 + 1) & 0xFF
    rows[:, 36], rows[:, 37] = (1000 + k % FLOWS) >> 8, (1000 + k % FLOWS) & 0xFF
    off, ln = (k * 64).astype(np.uint64), np.full(N, 58, dtype=np.uint32)
    flat = rows.reshape(-1)
    _, st = coracle.fill_batch(flat, off, ln, 0, coracle.FILL_CSUM)
    assert not st.any()
    return flat, off, ln


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
    from seqs_amd import (ACCEPT_CONN_DTYPE, ACCEPT_SLOT_DTYPE, FLOW_DTYPE, FLOW_TOTALS_DTYPE, LISTENER_DTYPE,
                          LISTENER_OUT_DTYPE, RUN_DTYPE, SEND_DTYPE, SND_DTYPE, SND_OUT_DTYPE, SOCK_DTYPE, SOCK_OUT_DTYPE, Engine,
                          segment_layout, split_accept, split_socks)

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    eng = Engine(0)
    stream = torch.cuda.Stream(dev)
    per = 1024 if a.shape == "a" else 16  # slots per listener
    n_listeners = 0 if a.shape == "c" else FLOWS
    listeners = np.zeros(FLOWS, dtype=LISTENER_DTYPE)
    for i in range(FLOWS):
        listeners["local"][i] = np.frombuffer(LOCAL_IP + (1000 + i).to_bytes(2, "big"), dtype=np.uint8)
        listeners["mac"][i] = np.frombuffer(MAC, dtype=np.uint8)
    listeners["slot_first"], listeners["n_slots"] = np.arange(FLOWS) * per, per
    n_slots = FLOWS * per
    slots = np.zeros(n_slots, dtype=ACCEPT_SLOT_DTYPE)
    slots["iss"], slots["rcv_wnd"], slots["ip_id"] = np.arange(n_slots) * 4099, 65535, np.arange(n_slots) % 65536

    if a.shape == "a":
        buf, off, ln = syn_frames(rng)
        n_socks, socks, snd, rings_bytes = 0, np.zeros(0, dtype=SOCK_DTYPE), np.zeros(0, dtype=SND_DTYPE), 64
        frames = [torch.from_numpy(buf).to(dev) for _ in range(a.buffers)]
        desc = [(torch.from_numpy(off.astype(np.int64)).to(dev), torch.from_numpy(ln.astype(np.int32)).to(dev))] * a.buffers
        rings = [torch.zeros(64, dtype=torch.uint8, device=dev) for _ in range(a.buffers)]
    else:
        # tools/recv_bench.py's shape without pure ACKs: F flows of data frames built by fs_segment_batch
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

    def empty(shape, dtype=torch.uint8):
        return torch.empty(shape, dtype=dtype, device=dev)

    runs, flows_t = empty((N, RUN_DTYPE.itemsize)), empty((N, FLOW_DTYPE.itemsize))
    order_t, run_of = empty((N,), torch.int32), empty((N,), torch.int32)
    ftotals, out, status = empty((FLOW_TOTALS_DTYPE.itemsize,)), empty((N, 2), torch.int32), empty((N,))
    socks_out, snd_out = empty((max(n_socks, 1), SOCK_OUT_DTYPE.itemsize)), empty((max(n_socks, 1), SND_OUT_DTYPE.itemsize))
    delivered, code = empty((N,)), empty((N,))
    conns, lout = empty((n_slots, ACCEPT_CONN_DTYPE.itemsize)), empty((FLOWS, LISTENER_OUT_DTYPE.itemsize))
    accept_of, synacks = empty((N,), torch.int32), torch.zeros(n_slots * 64, dtype=torch.uint8, device=dev)
    syn_out, syn_st = empty((n_slots, 2), torch.int32), empty((n_slots,))
    vp = ctypes.c_void_p

    def args_of(b, accept):
        head = (eng._ctx, vp(frames[b].data_ptr()), vp(desc[b][0].data_ptr()), vp(desc[b][1].data_ptr()), N, 0, 0,
                vp(socks.ctypes.data), n_socks, vp(rings[b].data_ptr()), rings_bytes, vp(socks_out.data_ptr()),
                vp(delivered.data_ptr()), vp(snd.ctypes.data), vp(snd_out.data_ptr()), vp(code.data_ptr()))
        mid = (vp(listeners.ctypes.data), n_listeners, vp(slots.ctypes.data), n_slots, 0, vp(conns.data_ptr()),
               vp(lout.data_ptr()), vp(accept_of.data_ptr()), vp(synacks.data_ptr()), vp(syn_out.data_ptr()),
               vp(syn_st.data_ptr())) if accept else ()
        tail = (None, 0, vp(runs.data_ptr()), vp(flows_t.data_ptr()), vp(order_t.data_ptr()), vp(run_of.data_ptr()),
                vp(ftotals.data_ptr()), vp(out.data_ptr()), vp(status.data_ptr()), vp(stream.cuda_stream))
        return head + mid + tail

    def kind(accept):
        fn = eng.lib.fs_accept_flows_batch if accept else eng.lib.fs_recv_flows_batch
        args = [args_of(b, accept) for b in range(a.buffers)]

        def run(b):
            st = fn(*args[b])
            assert st == 0, eng.lib.fs_last_error(eng._ctx)
        return run

    kinds = [("accept", kind(True)), ("recv", kind(False))]

    # checked once: the shape does what it says
    with torch.cuda.stream(stream):
        kinds[0][1](0)
    stream.synchronize()
    c, lo, of = split_accept(conns, lout[:n_listeners], accept_of)
    if a.shape == "a":
        assert int(c["used"].sum()) == N and (lo["n_accepted"] == per).all() and not lo["n_full"].any()
        assert sorted(of.tolist()) == list(range(N)) and int(syn_st.max()) == 0 and int(status.max()) == 0
    else:
        assert not c["used"].any() and (of == 0xFFFFFFFF).all() and not lo.view(np.uint8).any()
        assert (split_socks(socks_out)["n_delivered"] == N // FLOWS).all() and torch.equal(rings[0], src)

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
        "shape": a.shape, "frames": N, "n_socks": n_socks, "n_listeners": n_listeners, "n_slots": n_slots,
        "buffers": a.buffers, "rounds": a.rounds, "launches_per_round": a.launches,
        **{name + "_us": round(v, 2) for name, v in med.items()}, "round_min_max_us": spread,
        "accept_minus_recv_us": round(med["accept"] - med["recv"], 2), "accept_over_recv": round(med["accept"] / med["recv"], 3),
        "last_kernel": eng.last_kernel(), "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
    }
    lines.append("median of rounds [min, max]: " + "  ".join(f"{name} {med[name]:.2f} us {spread[name]}" for name, _ in kinds) +
                 f"  accept - recv = {med['accept'] - med['recv']:.2f} us")
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
