#!/usr/bin/env python3
"""TX frame build against what a caller pays without it, in one process on one GPU.

Shape: 1,024 sends x 64 frames, mss 1446 (65,536 frames of 1500 B, the C2 shape), align 4, with FCS.
Three things are timed with HIP events, one event pair per launch, over interleaved rounds of
launches that rotate over distinct payload and frame buffers (more than the 256 MiB Infinity Cache
holds in total, as bench.py rotates its batches for C2):
  (a) fs_segment_batch: payload -> finished frames;
  (b) a device-to-device hipMemcpyAsync of the same payload byte count;
  (c) the existing fs_fill_batch with FS_FILL_CSUM | FS_FCS_APPEND on the built frames.
(b) + (c) is a floor for the two-step path (assemble, then fill): it leaves out the header writes.
Prints the per-round medians, the medians over rounds and one JSON line.

    python tools/segment_bench.py [--rounds 3] [--launches 100] [--buffers 4] [--out FILE]
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


def tcp_template(rng) -> bytes:
    h = bytearray(rng.integers(0, 256, 54, dtype=np.uint8).tobytes())
    h[12:14], h[14], h[23], h[46], h[47] = b"\x08\x00", 0x45, 6, 0x50, 0x18
    h[34:38] = b"\x12\x34\x00\x50"
    return bytes(h)


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--launches", type=int, default=100)
    p.add_argument("--buffers", type=int, default=4)
    p.add_argument("--sends", type=int, default=1024)
    p.add_argument("--frames-per-send", type=int, default=64)
    p.add_argument("--mss", type=int, default=1446)
    p.add_argument("--out", default=None, help="also write the report to this file")
    a = p.parse_args()

    import torch

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    from seqs_amd import FCS_APPEND, FILL_CSUM, SEND_DTYPE, Engine, segment_layout

    dev = torch.device("cuda:0")
    # the HIP runtime this process already runs on (the one torch and the library loaded), by its path
    with open("/proc/self/maps") as f:
        hip_path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = ctypes.CDLL(hip_path)
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    D2D = 3  # hipMemcpyDeviceToDevice

    rng = np.random.default_rng(1)
    per = a.frames_per_send * a.mss
    sends = np.zeros(a.sends, dtype=SEND_DTYPE)
    for i in range(a.sends):
        sends["hdr"][i] = np.frombuffer(tcp_template(rng), dtype=np.uint8)
    sends["mss"], sends["payload_len"] = a.mss, per
    sends["payload_off"] = np.arange(a.sends, dtype=np.uint64) * np.uint64(per)
    flags, align = FCS_APPEND, 4
    n_frames, frames_bytes = segment_layout(sends, flags, align)
    payload_bytes = a.sends * per

    eng = Engine(0)
    stream = torch.cuda.Stream(dev)
    payloads = [torch.from_numpy(rng.integers(0, 256, payload_bytes, dtype=np.uint8)).to(dev) for _ in range(a.buffers)]
    frames = [torch.empty(frames_bytes, dtype=torch.uint8, device=dev) for _ in range(a.buffers)]
    copies = [torch.empty(payload_bytes, dtype=torch.uint8, device=dev) for _ in range(a.buffers)]
    built = []
    with torch.cuda.stream(stream):
        for b in range(a.buffers):
            built.append(eng.segment_device(sends, payloads[b], 0, flags, align, stream=stream, frames=frames[b]))
    stream.synchronize()
    assert all(int(r[4].max()) == 0 for r in built), "a built frame is not FS_OK"
    fills = [eng.prepare_digest(frames[b], built[b][1], built[b][2], 0, stream=stream, op="fill",
                                flags=FILL_CSUM | FCS_APPEND) for b in range(a.buffers)]

    vp = ctypes.c_void_p
    seg_args = [(eng._ctx, sends.ctypes.data_as(vp), a.sends, vp(payloads[b].data_ptr()), payload_bytes, 0, flags, align,
                 vp(frames[b].data_ptr()), frames_bytes, vp(built[b][1].data_ptr()), vp(built[b][2].data_ptr()),
                 vp(built[b][3].data_ptr()), vp(built[b][4].data_ptr()), vp(stream.cuda_stream))
                for b in range(a.buffers)]

    def run_segment(b):
        st = eng.lib.fs_segment_batch(*seg_args[b])
        assert st == 0, eng.lib.fs_last_error(eng._ctx)

    def run_copy(b):
        st = hip.hipMemcpyAsync(copies[b].data_ptr(), payloads[b].data_ptr(), payload_bytes, D2D, stream.cuda_stream)
        assert st == 0, st

    def run_fill(b):
        fills[b]()

    kinds = [("segment", run_segment), ("copy", run_copy), ("fill", run_fill)]

    def timed(fn, launches):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        with torch.cuda.stream(stream):
            for i, (e0, e1) in enumerate(ev):
                e0.record(stream)
                fn(i % a.buffers)
                e1.record(stream)
        stream.synchronize()
        return [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]  # us

    for _, fn in kinds:  # warm-up (also past the fill's automatic kernel choice window)
        timed(fn, 40)
    rounds = {k: [] for k, _ in kinds}
    lines = []
    for r in range(a.rounds):
        for k, fn in kinds:
            t = timed(fn, a.launches)
            rounds[k].append(statistics.median(t))
        lines.append(f"round {r}: " + "  ".join(f"{k} {rounds[k][-1]:8.2f} us" for k, _ in kinds))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    floor = med["copy"] + med["fill"]
    res = {
        "shape": f"{a.sends} sends x {a.frames_per_send} frames, mss {a.mss}, align {align}, FCS",
        "frames": n_frames, "payload_bytes": payload_bytes, "frames_bytes": frames_bytes,
        "buffers": a.buffers, "rounds": a.rounds, "launches_per_round": a.launches,
        "segment_us": round(med["segment"], 2), "copy_us": round(med["copy"], 2), "fill_us": round(med["fill"], 2),
        "copy_plus_fill_us": round(floor, 2), "goal_met": bool(med["segment"] <= floor),
        "segment_GBps_out": round(frames_bytes / med["segment"] / 1e3, 1),
        "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
    }
    lines.append(f"median of rounds: (a) segment {med['segment']:.2f} us  (b) copy {med['copy']:.2f} us  "
                 f"(c) fill {med['fill']:.2f} us  (b)+(c) {floor:.2f} us  goal (a) <= (b)+(c): "
                 f"{'met' if res['goal_met'] else 'MISSED'}")
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
