#!/usr/bin/env python3
"""RX coalesce against the traffic floor of its design, in one process on one GPU.

Shape: 65,536 TCP frames of 1500 B, device-resident, built by fs_segment_batch from sends of
44 x 1,446 bytes (1,489 such sends and one of 20 frames), align 4, no FCS. Three things are timed with
HIP events, one event pair per launch, over interleaved rounds of launches that rotate over distinct
frame and payload buffers (more than the 256 MiB Infinity Cache holds in total):
  (a) fs_coalesce_batch: frames -> verdicts, packed payload, runs;
  (b) fs_digest_batch on the same frames;
  (c) a device-to-device hipMemcpyAsync of payload_bytes.
(b) + (c) is the floor of a design that digests first and gathers behind it: the frames are read
twice and the payload is written once. The goal is (a) <= 1.5 x ((b) + (c)).
Prints the per-round medians, the medians over rounds and one JSON line.

With --flows F the same 65,536 frames come from F sends of 65,536 / F frames each, and a second set of
`offsets` / `lengths` lists them round-robin across the sends (A0 B0 ... A1 B1 ...; no bytes move).
Then five things are timed the same way:
  (a) fs_coalesce_flows_batch on the interleaved descriptors;
  (b) fs_coalesce_batch on the same frames un-interleaved;
  (c) the flow coalesce's sort alone (through the test library's fs_test_set_flow_steps, on the keys
      a whole call has left in the context's scratch);
  and the digest and the copy as above. The report states (a) / (b).

    python tools/coalesce_bench.py [--flows F] [--rounds 3] [--launches 100] [--buffers 4] [--out FILE]
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


def tcp_template(rng, sport: int) -> bytes:
    h = bytearray(rng.integers(0, 256, 54, dtype=np.uint8).tobytes())
    h[12:14], h[14], h[23], h[46], h[47] = b"\x08\x00", 0x45, 6, 0x50, 0x18
    h[34:36], h[36:38] = (1024 + sport % 60000).to_bytes(2, "big"), b"\x00\x50"
    return bytes(h)


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--launches", type=int, default=100)
    p.add_argument("--buffers", type=int, default=4)
    p.add_argument("--frames", type=int, default=65536)
    p.add_argument("--frames-per-send", type=int, default=44)
    p.add_argument("--mss", type=int, default=1446)
    p.add_argument("--flows", type=int, default=0, help="F sends, their frames interleaved round-robin (0: off)")
    p.add_argument("--out", default=None, help="also write the report to this file")
    a = p.parse_args()

    import torch

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    from seqs_amd import (FLOW_DTYPE, FLOW_TOTALS_DTYPE, RUN_DTYPE, SEND_DTYPE, TOTALS_DTYPE, Engine, segment_layout,
                          split_flows, split_runs)
    from seqs_amd.framesum import TEST_LIB_PATH

    if a.flows:
        assert a.frames % a.flows == 0 and a.frames // a.flows <= 4096, "--flows must divide --frames into sends of <= 4096"
        a.frames_per_send = a.frames // a.flows

    dev = torch.device("cuda:0")
    # the HIP runtime this process already runs on (the one torch and the library loaded), by its path
    with open("/proc/self/maps") as f:
        hip_path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = ctypes.CDLL(hip_path)
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    D2D = 3  # hipMemcpyDeviceToDevice

    rng = np.random.default_rng(1)
    n_sends = -(-a.frames // a.frames_per_send)
    counts = np.full(n_sends, a.frames_per_send, dtype=np.uint64)
    counts[-1] = a.frames - a.frames_per_send * (n_sends - 1)
    sends = np.zeros(n_sends, dtype=SEND_DTYPE)
    for i in range(n_sends):
        sends["hdr"][i] = np.frombuffer(tcp_template(rng, i), dtype=np.uint8)
    sends["mss"] = a.mss
    sends["payload_len"] = counts * np.uint64(a.mss)
    sends["payload_off"][1:] = np.cumsum(sends["payload_len"][:-1].astype(np.uint64))
    align = 4
    n_frames, frames_bytes = segment_layout(sends, 0, align)
    payload_bytes = int(sends["payload_len"].sum(dtype=np.uint64))
    assert n_frames == a.frames

    eng = Engine(0)
    stream = torch.cuda.Stream(dev)
    src = torch.from_numpy(rng.integers(0, 256, payload_bytes, dtype=np.uint8)).to(dev)
    frames = [torch.empty(frames_bytes, dtype=torch.uint8, device=dev) for _ in range(a.buffers)]
    gathered = [torch.empty(payload_bytes, dtype=torch.uint8, device=dev) for _ in range(a.buffers)]
    copies = [torch.empty(payload_bytes, dtype=torch.uint8, device=dev) for _ in range(a.buffers)]
    built = []
    with torch.cuda.stream(stream):
        for b in range(a.buffers):
            built.append(eng.segment_device(sends, src, 0, 0, align, stream=stream, frames=frames[b]))
    stream.synchronize()
    assert all(int(r[4].max()) == 0 for r in built), "a built frame is not FS_OK"
    digests = [eng.prepare_digest(frames[b], built[b][1], built[b][2], 0, stream=stream) for b in range(a.buffers)]

    runs = torch.empty((n_frames, RUN_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    run_of = torch.empty((n_frames,), dtype=torch.int32, device=dev)
    totals = torch.empty((TOTALS_DTYPE.itemsize,), dtype=torch.uint8, device=dev)
    out = torch.empty((n_frames, 2), dtype=torch.int32, device=dev)
    status = torch.empty((n_frames,), dtype=torch.uint8, device=dev)
    vp = ctypes.c_void_p
    co_args = [(eng._ctx, vp(frames[b].data_ptr()), vp(built[b][1].data_ptr()), vp(built[b][2].data_ptr()), n_frames, 0, 0,
                vp(gathered[b].data_ptr()), payload_bytes, vp(runs.data_ptr()), vp(run_of.data_ptr()),
                vp(totals.data_ptr()), vp(out.data_ptr()), vp(status.data_ptr()), vp(stream.cuda_stream))
               for b in range(a.buffers)]

    def run_coalesce(b):
        st = eng.lib.fs_coalesce_batch(*co_args[b])
        assert st == 0, eng.lib.fs_last_error(eng._ctx)

    def run_digest(b):
        digests[b]()

    def run_copy(b):
        st = hip.hipMemcpyAsync(copies[b].data_ptr(), gathered[b].data_ptr(), payload_bytes, D2D, stream.cuda_stream)
        assert st == 0, st

    # the coalesce gives the sends back: checked once, outside the timed launches
    with torch.cuda.stream(stream):
        run_coalesce(0)
    stream.synchronize()
    r, total, n_runs = split_runs(runs, totals)
    assert (total, n_runs) == (payload_bytes, n_sends) and torch.equal(gathered[0], src)
    assert np.array_equal(r["n_frames"], counts.astype(np.uint32)) and int(status.max()) == 0

    kinds = [("coalesce", run_coalesce), ("digest", run_digest), ("copy", run_copy)]

    if a.flows:
        # the interleaved descriptors: frame k of the batch is frame k // F of send k % F
        k = torch.arange(n_frames, device=dev)
        perm = (k % a.flows) * a.frames_per_send + k // a.flows
        inter = [(built[b][1][perm].contiguous(), built[b][2][perm].contiguous()) for b in range(a.buffers)]
        flows_t = torch.empty((n_frames, FLOW_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        order_t = torch.empty((n_frames,), dtype=torch.int32, device=dev)
        ftotals = torch.empty((FLOW_TOTALS_DTYPE.itemsize,), dtype=torch.uint8, device=dev)

        def flow_args(ctx, b):
            return (ctx, vp(frames[b].data_ptr()), vp(inter[b][0].data_ptr()), vp(inter[b][1].data_ptr()), n_frames, 0, 0,
                    vp(gathered[b].data_ptr()), payload_bytes, vp(runs.data_ptr()), vp(flows_t.data_ptr()),
                    vp(order_t.data_ptr()), vp(run_of.data_ptr()), vp(ftotals.data_ptr()), vp(out.data_ptr()),
                    vp(status.data_ptr()), vp(stream.cuda_stream))

        fl_args = [flow_args(eng._ctx, b) for b in range(a.buffers)]
        teng = Engine(0, lib_path=TEST_LIB_PATH)  # (c): its context's scratch keeps the sort keys of one whole call
        t_args = flow_args(teng._ctx, 0)

        def run_flows(b):
            st = eng.lib.fs_coalesce_flows_batch(*fl_args[b])
            assert st == 0, eng.lib.fs_last_error(eng._ctx)

        def run_sort(b):
            st = teng.lib.fs_coalesce_flows_batch(*t_args)
            assert st == 0, teng.lib.fs_last_error(teng._ctx)

        # each send's payload comes back contiguous, one flow and one run per send: checked once
        gathered[0].zero_()
        with torch.cuda.stream(stream):
            run_flows(0)
            run_sort(0)
        stream.synchronize()
        fr, ff, fo, ft = split_flows(runs, flows_t, order_t, ftotals)
        assert (int(ft["payload_bytes"]), int(ft["n_runs"]), int(ft["n_flows"]), int(ft["n_accepted"])) == \
            (payload_bytes, n_sends, n_sends, n_frames) and torch.equal(gathered[0], src)
        assert np.array_equal(fr["n_frames"], counts.astype(np.uint32)) and np.array_equal(perm.cpu().numpy()[fo], np.arange(n_frames))
        assert teng.lib.fs_test_set_flow_steps(teng._ctx, 2) == 0  # from here on the test context only sorts
        kinds = [("flows", run_flows), ("coalesce", run_coalesce), ("sort", run_sort), ("digest", run_digest),
                 ("copy", run_copy)]

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
    rounds = {k: [] for k, _ in kinds}
    lines = []
    for rd in range(a.rounds):
        for k, fn in kinds:
            t = timed(fn, a.launches)
            rounds[k].append(statistics.median(t))
        lines.append(f"round {rd}: " + "  ".join(f"{k} {rounds[k][-1]:8.2f} us" for k, _ in kinds))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    floor = med["digest"] + med["copy"]
    ratio = med["coalesce"] / floor
    res = {
        "shape": f"{n_frames} frames of {54 + a.mss} B from {n_sends} sends of {a.frames_per_send} x {a.mss} B, align {align}",
        "frames": n_frames, "runs": n_runs, "payload_bytes": payload_bytes, "frames_bytes": frames_bytes,
        "buffers": a.buffers, "rounds": a.rounds, "launches_per_round": a.launches,
        "coalesce_us": round(med["coalesce"], 2), "digest_us": round(med["digest"], 2), "copy_us": round(med["copy"], 2),
        "digest_plus_copy_us": round(floor, 2), "ratio": round(ratio, 3), "goal_met": bool(ratio <= 1.5),
        "last_kernel": eng.last_kernel(), "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
    }
    lines.append(f"median of rounds: (a) coalesce {med['coalesce']:.2f} us  (b) digest {med['digest']:.2f} us  "
                 f"(c) copy {med['copy']:.2f} us  (b)+(c) {floor:.2f} us  (a) / ((b)+(c)) = {ratio:.3f}  "
                 f"goal <= 1.5: {'met' if res['goal_met'] else 'MISSED'}")
    if a.flows:
        spread = {k: round(max(v) - min(v), 2) for k, v in rounds.items()}
        res.update({"flows": a.flows, "flows_us": round(med["flows"], 2), "sort_us": round(med["sort"], 2),
                    "flows_over_coalesce": round(med["flows"] / med["coalesce"], 3), "round_spread_us": spread})
        lines.append(f"--flows {a.flows}: (a) coalesce_flows {med['flows']:.2f} us  (b) coalesce, un-interleaved "
                     f"{med['coalesce']:.2f} us  (c) sort alone {med['sort']:.2f} us  (a) / (b) = {med['flows'] / med['coalesce']:.3f}")
        teng.close()
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
