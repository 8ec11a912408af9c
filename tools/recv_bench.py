#!/usr/bin/env python3
"""The receive call against the in-order delivery it builds on, in one process on one GPU, from the
same library on the same frames.

Shape (that of tools/deliver_bench.py): 65,536 TCP frames, device-resident, F flows listed round-robin
across the flows, F sockets whose rings hold the whole flow; the data frames are 1500 B, built by
fs_segment_batch. With --acks every second frame of a flow is a 54-byte pure ACK behind the data
frame before it (Seq at rcv.NXT, an Ack that rises by one, a window of its own): half the frames are
data then. The sockets' snd_nxt lies 2^20 above the Ack the data frames carry, so every data frame
sets snd.UNA back and every pure ACK raises it. Timed with HIP events, one event pair per call, over
interleaved rounds of calls that rotate over distinct frame and rings buffers:
  (a) fs_recv_flows_batch, payload NULL;      (b) fs_deliver_flows_batch, payload NULL;
  (c) fs_recv_flows_batch, packed payload;    (d) fs_deliver_flows_batch, packed payload.
--flows 1 is the walk's worst case: one wave walks all the frames alone.
Prints the per-round medians, the medians over rounds with the rounds' spread, and one JSON line.

    python tools/recv_bench.py [--flows 64] [--acks] [--rounds 3] [--launches 100] [--buffers 4] [--out FILE]
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

ABOVE = 1 << 20  # snd_nxt above the Ack of the data frames


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--launches", type=int, default=100)
    p.add_argument("--buffers", type=int, default=4)
    p.add_argument("--frames", type=int, default=65536)
    p.add_argument("--mss", type=int, default=1446)
    p.add_argument("--flows", type=int, default=64, help="F flows, their frames interleaved round-robin, F sockets")
    p.add_argument("--acks", action="store_true", help="every second frame of a flow is a 54-byte pure ACK")
    p.add_argument("--out", default=None, help="also write the report to this file")
    a = p.parse_args()

    import torch

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    from oracle import coracle
    from seqs_amd import (FLOW_DTYPE, FLOW_TOTALS_DTYPE, RUN_DTYPE, SEND_DTYPE, SND_DTYPE, SND_OUT_DTYPE, SOCK_DTYPE,
                          SOCK_OUT_DTYPE, Engine, segment_layout, split_snd, split_socks)

    n_data = a.frames // 2 if a.acks else a.frames
    assert n_data % a.flows == 0, "--flows must divide the data frames"
    per_flow = n_data // a.flows  # data frames per flow
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
    snd = np.zeros(a.flows, dtype=SND_DTYPE)
    ack_frames = np.zeros((n_data if a.acks else 0, 56), dtype=np.uint8)  # 54 bytes each, 56 apart
    for f in range(a.flows):
        h = tcp_template(rng, f)
        seq0, ack0 = int.from_bytes(h[38:42], "big"), int.from_bytes(h[42:46], "big")
        socks["key"][f] = np.frombuffer(bytes([6]) + bytes(h[26:38]), dtype=np.uint8)
        socks["rcv_nxt"][f], socks["snd_nxt"][f] = seq0, (ack0 + ABOVE) % (1 << 32)
        snd["snd_una"][f], snd["snd_wnd"][f] = ack0, 1000
        for s in range(sends_per_flow):
            h[38:42] = ((seq0 + s * per_send * a.mss) % (1 << 32)).to_bytes(4, "big")
            sends["hdr"][f * sends_per_flow + s] = np.frombuffer(bytes(h), dtype=np.uint8)
        if a.acks:
            j = np.arange(per_flow, dtype=np.int64)
            rows = ack_frames[f * per_flow : (f + 1) * per_flow]
            rows[:, :54] = np.frombuffer(bytes(h), dtype=np.uint8)
            rows[:, 16], rows[:, 17] = 0, 40
            for col, val in ((38, (seq0 + (j + 1) * a.mss) % (1 << 32)), (42, (ack0 + 1 + j) % (1 << 32))):
                for k in range(4):
                    rows[:, col + k] = (val >> (24 - 8 * k)) & 0xFF
            rows[:, 48], rows[:, 49] = (2000 + j % 1000) >> 8, (2000 + j % 1000) & 0xFF
    socks["rcv_wnd"], socks["ring_size"], socks["ring_free"] = 65535, ring_size, ring_size
    socks["ring_off"] = np.arange(a.flows, dtype=np.uint64) * np.uint64(ring_size)
    sends["mss"] = a.mss
    sends["payload_len"] = per_send * a.mss
    sends["payload_off"] = np.arange(n_sends, dtype=np.uint64) * np.uint64(per_send * a.mss)
    align = 4
    n_built, data_bytes = segment_layout(sends, 0, align)
    payload_bytes = n_data * a.mss
    assert n_built == n_data
    ack_off = np.uint64((data_bytes + 63) // 64 * 64) + np.arange(ack_frames.shape[0], dtype=np.uint64) * np.uint64(56)
    ack_len = np.full(ack_frames.shape[0], 54, dtype=np.uint32)
    if a.acks:
        flat = ack_frames.reshape(-1)
        coracle.fill_batch(flat, ack_off - ack_off[0], ack_len, 0, coracle.FILL_CSUM)
    frames_bytes = int(ack_off[0]) + ack_frames.size if a.acks else data_bytes
    n_frames = n_data + ack_frames.shape[0]

    eng = Engine(0)
    stream = torch.cuda.Stream(dev)
    src = torch.from_numpy(rng.integers(0, 256, payload_bytes, dtype=np.uint8)).to(dev)
    frames = [torch.empty(frames_bytes + 64, dtype=torch.uint8, device=dev) for _ in range(a.buffers)]
    gathered = [torch.empty(payload_bytes, dtype=torch.uint8, device=dev) for _ in range(a.buffers)]
    rings = [torch.zeros(payload_bytes, dtype=torch.uint8, device=dev) for _ in range(a.buffers)]
    built = []
    with torch.cuda.stream(stream):
        for b in range(a.buffers):
            built.append(eng.segment_device(sends, src, 0, 0, align, stream=stream, frames=frames[b][:data_bytes]))
            if a.acks:
                frames[b][int(ack_off[0]) : int(ack_off[0]) + ack_frames.size].copy_(torch.from_numpy(ack_frames.reshape(-1)).to(dev))
    stream.synchronize()
    assert all(int(r[4].max()) == 0 for r in built), "a built frame is not FS_OK"
    # the interleaved descriptors: slot t of flow f is batch frame t * F + f; with --acks slot 2 j is the
    # flow's data frame j and slot 2 j + 1 the pure ACK behind it
    k = torch.arange(n_frames, device=dev)
    flow, slot = k % a.flows, k // a.flows
    t_ack_off = torch.from_numpy(ack_off.astype(np.int64)).to(dev)
    inter = []
    for b in range(a.buffers):
        d_off, d_len = built[b][1], built[b][2]
        if a.acks:
            j = flow * per_flow + slot // 2
            is_ack = slot % 2 == 1
            off = torch.where(is_ack, t_ack_off[j], d_off[j].to(torch.int64))
            ln = torch.where(is_ack, torch.full_like(j, 54), d_len[j].to(torch.int64)).to(torch.int32)
        else:
            j = flow * per_flow + slot
            off, ln = d_off[j], d_len[j]
        inter.append((off.contiguous(), ln.contiguous()))

    runs = torch.empty((n_frames, RUN_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    flows_t = torch.empty((n_frames, FLOW_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    order_t = torch.empty((n_frames,), dtype=torch.int32, device=dev)
    run_of = torch.empty((n_frames,), dtype=torch.int32, device=dev)
    ftotals = torch.empty((FLOW_TOTALS_DTYPE.itemsize,), dtype=torch.uint8, device=dev)
    out = torch.empty((n_frames, 2), dtype=torch.int32, device=dev)
    status = torch.empty((n_frames,), dtype=torch.uint8, device=dev)
    socks_out = torch.empty((a.flows, SOCK_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    snd_out = torch.empty((a.flows, SND_OUT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    delivered = torch.empty((n_frames,), dtype=torch.uint8, device=dev)
    code = torch.empty((n_frames,), dtype=torch.uint8, device=dev)
    vp = ctypes.c_void_p

    def call(b, recv, packed):
        head = (eng._ctx, vp(frames[b].data_ptr()), vp(inter[b][0].data_ptr()), vp(inter[b][1].data_ptr()), n_frames, 0, 0,
                vp(socks.ctypes.data), a.flows, vp(rings[b].data_ptr()), payload_bytes, vp(socks_out.data_ptr()),
                vp(delivered.data_ptr()))
        mid = (vp(snd.ctypes.data), vp(snd_out.data_ptr()), vp(code.data_ptr())) if recv else ()
        tail = ((vp(gathered[b].data_ptr()), payload_bytes) if packed else (None, 0)) + \
            (vp(runs.data_ptr()), vp(flows_t.data_ptr()), vp(order_t.data_ptr()), vp(run_of.data_ptr()),
             vp(ftotals.data_ptr()), vp(out.data_ptr()), vp(status.data_ptr()), vp(stream.cuda_stream))
        return head + mid + tail

    def kind(recv, packed):
        fn = eng.lib.fs_recv_flows_batch if recv else eng.lib.fs_deliver_flows_batch
        args = [call(b, recv, packed) for b in range(a.buffers)]

        def run(b):
            st = fn(*args[b])
            assert st == 0, eng.lib.fs_last_error(eng._ctx)
        return run

    kinds = [("recv", kind(True, False)), ("deliver", kind(False, False)), ("recv_packed", kind(True, True)),
             ("deliver_packed", kind(False, True))]

    # checked once: every flow arrives whole in its ring under both calls, and the send side is what the shape says
    with torch.cuda.stream(stream):
        kinds[1][1](0)
    stream.synchronize()
    want = split_socks(socks_out).copy()
    assert torch.equal(rings[0], src) and (want["n_delivered"] == per_flow).all() and (want["ring_free"] == 0).all()
    rings[0].zero_()
    with torch.cuda.stream(stream):
        kinds[0][1](0)
    stream.synchronize()
    assert torch.equal(rings[0], src) and split_socks(socks_out).tobytes() == want.tobytes()
    so = split_snd(snd_out)
    slots = n_frames // a.flows
    assert (so["n_taken"] == slots).all() and int(code.min()) == 1 and int(code.max()) == 1 and (so["flags"] == 1).all()
    last = (snd["snd_una"].astype(np.int64) + (per_flow if a.acks else 0)) % (1 << 32)
    assert (so["snd_una"] == last).all()

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
        "shape": f"{n_frames} frames ({n_data} of {54 + a.mss} B, {n_frames - n_data} pure ACKs of 54 B) in {a.flows} "
                 f"interleaved flows of {slots}, {a.flows} sockets, rings of {ring_size} B",
        "frames": n_frames, "flows": a.flows, "acks": bool(a.acks), "buffers": a.buffers, "rounds": a.rounds,
        "launches_per_round": a.launches, **{name + "_us": round(v, 2) for name, v in med.items()},
        "round_min_max_us": spread, "recv_minus_deliver_us": round(med["recv"] - med["deliver"], 2),
        "recv_over_deliver": round(med["recv"] / med["deliver"], 3),
        "recv_packed_over_deliver_packed": round(med["recv_packed"] / med["deliver_packed"], 3),
        "last_kernel": eng.last_kernel(), "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
    }
    lines.append("median of rounds [min, max]: " + "  ".join(f"{name} {med[name]:.2f} us {spread[name]}" for name, _ in kinds) +
                 f"  recv - deliver = {med['recv'] - med['deliver']:.2f} us  recv / deliver = {med['recv'] / med['deliver']:.3f}")
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
