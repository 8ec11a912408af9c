#!/usr/bin/env python3
"""The HIP calls and the kernels of each of the fourteen RX entry points (the plain and the flow-aware
coalesce, the delivery, the receive, the accept, the close and the connect call; device and host forms),
to compare two libraries call for call. Measurement tool.

  run:  python3 tools/rx_calls_trace.py run
        two calls of each entry point: the first four kinds on the 19-frame batch of
        tests/test_gpu_host_calls.py (rx_pin_case: three interleaved flows, three sockets), the accept, the
        close and the connect call on tests/connect_cases.py's mixed() (sockets, listeners, closers and
        openers in one batch), every array passed and allocated before the first call; a torch.cuda.synchronize() (hipDeviceSynchronize, which the library never
        calls) before the first call and behind each call marks the calls in the trace. The host forms
        run on the context's own stream, where which staging block the receive call's second staged
        launch gets (and so one hipEventQuery more or less) depends on whether the GPU has finished the
        delivery's few kernels by then
  seq:  python3 tools/rx_calls_trace.py seq <trace dir> [--call 2]
        from a rocprofv3 --hip-trace --kernel-trace of `run`, per entry point, the HIP API names of its
        second call in order and its kernels in order, each with its grid and workgroup size

  FRAMESUM_LIB=<library> rocprofv3 --hip-trace --kernel-trace --output-format csv -d <dir> -- \\
      python3 tools/rx_calls_trace.py run
"""
import csv
import ctypes
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BASES = ("fs_coalesce_batch", "fs_coalesce_flows_batch", "fs_deliver_flows_batch", "fs_recv_flows_batch",
         "fs_accept_flows_batch", "fs_close_flows_batch", "fs_connect_flows_batch")
NAMES = [b + suffix for b in BASES for suffix in ("", "_host")]
CALLS_EACH = 2
BUSY_CYCLES = 20_000_000  # about 10 ms of a spinning kernel in front of each device form


def run():
    import numpy as np
    import torch

    import connect_cases
    import flows_ref as fref
    from seqs_amd import Engine
    from test_gpu_host_calls import rx_pin_case

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    pin, mixed = rx_pin_case(), connect_cases.mixed()
    buf, off, ln = fref.pack(mixed.frames, lead=3)
    later = dict(buf=buf, off=off, ln=ln, n=int(ln.size), socks=mixed.socks, snd=mixed.snd, room=int(ln.sum()),
                 noise=np.zeros(int(ln.sum()), dtype=np.uint8), rings=np.zeros(mixed.rings_bytes, dtype=np.uint8))
    lists = [mixed.listeners, mixed.slots, mixed.closers, mixed.openers]
    n_listeners, n_slots, n_closers, n_openers = (int(x.size) for x in lists)
    eng = Engine(0)
    stream = torch.cuda.current_stream().cuda_stream
    prepared = []
    for kind, base in enumerate(BASES):
        case = pin if kind <= 3 else later
        n, n_socks = case["n"], int(case["socks"].size)
        for host in (False, True):
            sizes = dict(frames=case["buf"], offsets=case["off"].view(np.uint8), lengths=case["ln"].view(np.uint8),
                         payload=case["noise"].copy(), rings=case["rings"].copy())
            sizes.update({k: np.zeros(v, dtype=np.uint8) for k, v in dict(
                runs=24 * n, flows=32 * n, order=4 * n, run_of=4 * n, totals=24, out=8 * n, status=n, delivered=n, code=n,
                socks_out=32 * n_socks, snd_out=32 * n_socks, conns=48 * n_slots, listeners_out=16 * n_listeners, accept_of=4 * n,
                synacks=64 * n_slots, synack_out=8 * n_slots, synack_status=n_slots, closers_out=32 * n_closers,
                socks_close=32 * n_socks, ctl_code=n, openers_out=48 * n_openers, replies=64 * n_openers, reply_out=8 * n_openers,
                reply_status=n_openers).items()})
            held = sizes if host else {k: torch.from_numpy(v).to("cuda:0") for k, v in sizes.items()}
            at = (lambda k, h=held: h[k].ctypes.data) if host else (lambda k, h=held: h[k].data_ptr())
            args = [eng._ctx, at("frames")] + ([case["buf"].size] if host else []) + [at("offsets"), at("lengths"), n, 0, 0]
            if kind >= 2:
                args += [case["socks"].ctypes.data, n_socks, at("rings"), case["rings"].size, at("socks_out"), at("delivered")]
            if kind >= 3:
                args += [case["snd"].ctypes.data, at("snd_out"), at("code")]
            if kind >= 4:
                args += [lists[0].ctypes.data, n_listeners, lists[1].ctypes.data, n_slots, 0, at("conns"), at("listeners_out"),
                         at("accept_of"), at("synacks"), at("synack_out"), at("synack_status")]
            if kind >= 5:
                args += [lists[2].ctypes.data, n_closers, at("closers_out"), at("socks_close"), at("ctl_code")]
            if kind >= 6:
                args += [lists[3].ctypes.data, n_openers, 0, at("openers_out"), at("replies"), at("reply_out"), at("reply_status")]
            args += [at("payload"), case["room"], at("runs")] + ([at("flows"), at("order")] if kind >= 1 else [])
            args += [at("run_of"), at("totals"), at("out"), at("status")] + ([] if host else [stream])
            prepared.append((getattr(eng.lib, base + ("_host" if host else "")), args, held))
    torch.cuda.synchronize()
    for (fn, args, _), name in zip(prepared, NAMES):
        for _ in range(CALLS_EACH):
            if not name.endswith("_host"):
                # the stream is busy while a device form enqueues, so that the staging block of the call's
                # first staged launch is in flight when its second one looks for a block, as in a loaded stack
                # (with an idle stream that is a race between the GPU and the calling thread)
                torch.cuda._sleep(BUSY_CYCLES)
            st = fn(*args)
            assert st == 0, eng.lib.fs_last_error(eng._ctx)
            torch.cuda.synchronize()
    eng.close()
    print("calls", len(prepared) * CALLS_EACH)


def rows(tdir, pattern):
    out = []
    for f in glob.glob(os.path.join(tdir, "**", pattern), recursive=True):
        with open(f) as fh:
            out.extend(csv.DictReader(fh))
    return out


def seq(tdir, which):
    api = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Function"]) for r in rows(tdir, "*hip_api_trace.csv")))
    kernels = sorted(((int(r["Start_Timestamp"]), r) for r in rows(tdir, "*kernel_trace.csv")), key=lambda x: x[0])
    marks = [a for a in api if a[2] == "hipDeviceSynchronize"]
    total = len(NAMES) * CALLS_EACH
    assert len(marks) >= total + 1, f"{len(marks)} markers in the trace, {total + 1} expected"
    marks = marks[-(total + 1):]  # (the engine's close makes no such call)
    for j, name in enumerate(NAMES):
        before, behind = marks[j * CALLS_EACH + which - 1], marks[j * CALLS_EACH + which]
        print(f"== {name}, call {which}")
        print("  hip: " + " ".join(a[2] for a in api if before[1] <= a[0] < behind[0]))
        for t, r in kernels:
            if before[1] <= t < behind[1]:
                grid = "x".join(r.get(k, "?") for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z")) if "Grid_Size_X" in r \
                    else r.get("Grid_Size", "?")
                wg = "x".join(r.get(k, "?") for k in ("Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z")) \
                    if "Workgroup_Size_X" in r else r.get("Workgroup_Size", "?")
                name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0]
                print(f"  kernel: {name} grid {grid} wg {wg}")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) >= 3 and sys.argv[1] == "seq":
        seq(sys.argv[2], int(sys.argv[sys.argv.index("--call") + 1]) if "--call" in sys.argv else 2)
    else:
        sys.exit(__doc__)
