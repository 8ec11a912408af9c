#!/usr/bin/env python3
"""TCP segments built straight from socket TX rings against the TX frame build over the same bytes
linearised, in one process on one GPU and from one library.

Shape: S sockets of F frames of mss bytes each (64 x 1,024 x 1,446: 65,536 frames of 1,500 B), device-
resident. Every socket's ring is exactly full and read from its middle, so every socket's data wraps
at mid-range. Three things are timed with HIP events, one event pair per call, over interleaved
rounds of calls that rotate over distinct ring, linear and frame buffers (more than the 256 MiB
Infinity Cache holds in total):
  (a) fs_send_rings_batch from the rings;
  (b) fs_segment_batch over the same bytes already linear (the yardstick: the same frame body with a
      linear source);
  (c) (b) behind the device-to-device copy that linearises the rings (two strided copies for all
      sockets: each ring's upper half, then its lower half), which is what a caller needs today.
(a) - (b) is the cost of the ring source. The frames of (a) and (b) are compared byte for byte once.
Prints the per-round medians, the medians over rounds with the rounds' spread, and one JSON line.

    python tools/send_bench.py [--socks 64] [--frames 1024] [--rounds 3] [--launches 100] [--buffers 4] [--out FILE]
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


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--launches", type=int, default=100)
    p.add_argument("--buffers", type=int, default=4)
    p.add_argument("--socks", type=int, default=64)
    p.add_argument("--frames", type=int, default=1024, help="frames per socket (at most 4096)")
    p.add_argument("--mss", type=int, default=1446)
    p.add_argument("--out", default=None, help="also write the report to this file")
    a = p.parse_args()

    import torch

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    from seqs_amd import SEND_DTYPE, TX_SOCK_DTYPE, TX_SOCK_OUT_DTYPE, Engine, segment_layout, send_rings_layout

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    size = a.frames * a.mss
    half = size // 2
    socks = np.zeros(a.socks, dtype=TX_SOCK_DTYPE)
    hdr = rng.integers(0, 256, (a.socks, 54), dtype=np.uint8)
    hdr[:, 12], hdr[:, 13], hdr[:, 14], hdr[:, 23], hdr[:, 46] = 0x08, 0x00, 0x45, 6, 0x50
    hdr[:, 34:38] = [0x12, 0x34, 0x00, 0x50]
    socks["hdr"], socks["mss"], socks["ring_size"], socks["ring_rpos"], socks["ring_buffered"] = hdr, a.mss, size, half, size
    socks["ring_off"] = np.arange(a.socks, dtype=np.uint64) * np.uint64(size)
    socks["snd_una"] = socks["snd_nxt"] = rng.integers(0, 1 << 32, a.socks, dtype=np.uint64).astype(np.uint32)
    socks["snd_wnd"], socks["rcv_wnd"], socks["max_frames"] = 0xFFFFFFFF, 65535, a.frames
    socks["rcv_nxt"] = rng.integers(0, 1 << 32, a.socks, dtype=np.uint64).astype(np.uint32)
    # the same sends as the TX frame build takes them: the state written into the template by hand
    sends = np.zeros(a.socks, dtype=SEND_DTYPE)
    sends["hdr"] = hdr
    sends["hdr"][:, 38:42] = socks["snd_nxt"].astype(">u4").view(np.uint8).reshape(-1, 4)
    sends["hdr"][:, 42:46] = socks["rcv_nxt"].astype(">u4").view(np.uint8).reshape(-1, 4)
    sends["hdr"][:, 47], sends["hdr"][:, 48], sends["hdr"][:, 49] = 0x10, 0xFF, 0xFF
    sends["mss"], sends["payload_len"], sends["payload_off"] = a.mss, size, socks["ring_off"]
    align = 4
    n_frames, frames_bytes, expect = send_rings_layout(socks, 0, align)
    assert (n_frames, frames_bytes) == segment_layout(sends, 0, align) and n_frames == a.socks * a.frames
    total = a.socks * size

    eng = Engine(0)
    stream = torch.cuda.Stream(dev)
    rings = [torch.from_numpy(rng.integers(0, 256, total, dtype=np.uint8)).to(dev) for _ in range(a.buffers)]
    linear = [torch.empty(total, dtype=torch.uint8, device=dev) for _ in range(a.buffers)]
    frames = [torch.empty(frames_bytes, dtype=torch.uint8, device=dev) for _ in range(a.buffers)]
    offsets = torch.empty((n_frames,), dtype=torch.int64, device=dev)
    lengths = torch.empty((n_frames,), dtype=torch.int32, device=dev)
    out = torch.empty((n_frames, 2), dtype=torch.int32, device=dev)
    status = torch.empty((n_frames,), dtype=torch.uint8, device=dev)
    socks_out = np.zeros(a.socks, dtype=TX_SOCK_OUT_DTYPE)
    vp = ctypes.c_void_p

    def linearise(b):
        src, dst = rings[b].view(a.socks, size), linear[b].view(a.socks, size)
        dst[:, : size - half].copy_(src[:, half:])
        dst[:, size - half :].copy_(src[:, :half])

    results = (vp(offsets.data_ptr()), vp(lengths.data_ptr()), vp(out.data_ptr()), vp(status.data_ptr()))
    ring_args = [(eng._ctx, vp(socks.ctypes.data), a.socks, vp(rings[b].data_ptr()), total, 0, 0, align,
                  vp(frames[b].data_ptr()), frames_bytes, *results, vp(socks_out.ctypes.data), vp(stream.cuda_stream))
                 for b in range(a.buffers)]
    seg_args = [(eng._ctx, vp(sends.ctypes.data), a.socks, vp(linear[b].data_ptr()), total, 0, 0, align,
                 vp(frames[b].data_ptr()), frames_bytes, *results, vp(stream.cuda_stream)) for b in range(a.buffers)]

    def run_rings(b):
        st = eng.lib.fs_send_rings_batch(*ring_args[b])
        assert st == 0, eng.lib.fs_last_error(eng._ctx)

    def run_segment(b):
        st = eng.lib.fs_segment_batch(*seg_args[b])
        assert st == 0, eng.lib.fs_last_error(eng._ctx)

    def run_copy_segment(b):
        linearise(b)
        run_segment(b)

    kinds = [("send_rings", run_rings), ("segment", run_segment), ("copy_segment", run_copy_segment)]

    # both calls build the same frames: checked once per buffer
    with torch.cuda.stream(stream):
        for b in range(a.buffers):
            linearise(b)
            run_segment(b)
            want = (frames[b].clone(), offsets.clone(), lengths.clone(), out.clone())
            frames[b].zero_()
            run_rings(b)
            stream.synchronize()
            assert int(status.max()) == 0 and np.array_equal(socks_out, expect)
            assert all(torch.equal(x, y) for x, y in zip(want, (frames[b], offsets, lengths, out))), "the frames differ"
    stream.synchronize()

    def timed(fn, launches):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        with torch.cuda.stream(stream):
            for i, (e0, e1) in enumerate(ev):
                e0.record(stream)
                fn(i % a.buffers)
                e1.record(stream)
        stream.synchronize()
        return [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]  # us

    for _, fn in kinds:  # warm-up
        timed(fn, 40)
    rounds = {name: [] for name, _ in kinds}
    lines = []
    for rd in range(a.rounds):
        for name, fn in kinds:
            rounds[name].append(statistics.median(timed(fn, a.launches)))
        lines.append(f"round {rd}: " + "  ".join(f"{name} {rounds[name][-1]:9.2f} us" for name, _ in kinds))
    med = {name: statistics.median(v) for name, v in rounds.items()}
    spread = {name: [round(min(v), 2), round(max(v), 2)] for name, v in rounds.items()}
    wire = n_frames * (54 + a.mss)
    res = {
        "shape": f"{a.socks} sockets x {a.frames} frames of {54 + a.mss} B (mss {a.mss}), rings of {size} B read from {half}",
        "frames": n_frames, "ring_bytes": total, "buffers": a.buffers, "rounds": a.rounds, "launches_per_round": a.launches,
        "send_rings_us": round(med["send_rings"], 2), "segment_us": round(med["segment"], 2),
        "copy_segment_us": round(med["copy_segment"], 2), "round_min_max_us": spread,
        "ring_source_cost_us": round(med["send_rings"] - med["segment"], 2),
        "send_rings_over_segment": round(med["send_rings"] / med["segment"], 3),
        "send_rings_over_copy_segment": round(med["send_rings"] / med["copy_segment"], 3),
        "send_rings_gbps_of_frames": round(wire / med["send_rings"] / 1e3, 1),
        "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
    }
    lines.append(f"median of rounds [min, max]: (a) send_rings {med['send_rings']:.2f} us {spread['send_rings']}  "
                 f"(b) segment, linear source {med['segment']:.2f} us {spread['segment']}  "
                 f"(c) linearising copy + segment {med['copy_segment']:.2f} us {spread['copy_segment']}  "
                 f"(a) - (b) = {med['send_rings'] - med['segment']:.2f} us  "
                 f"(a) / (c) = {med['send_rings'] / med['copy_segment']:.3f}")
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
