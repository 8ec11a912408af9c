#!/usr/bin/env python3
"""The ARP call against the UDP call it builds on, in one process on one GPU, on the same frames with otherwise
equal arguments: payload NULL in both, no sockets, listeners, closers, openers or ports in either. The UDP call
comes from `--baseline-lib` (a libframesum.so built from the parent commit) or, without it, from the same library.

Shapes:
  a  65,536 UDP frames of 1,500 bytes with no hosts and no queries: what a caller without ARP pays, which is the
     one launch that writes arp_code and arp_of. It is reported beside the tool's own measurement of two n-entry
     fills (one of bytes, one of 32-bit words), the bound.
  b  shape a's batch with every hundredth frame a 60-byte ARP request, to 64 hosts with room for every request.
  c  65,536 ARP requests of 60 bytes to 1,000 hosts of 65 reply slots each (65,000 of the 65,536 slots a call may
     have): 536 hosts get a 66th request, which finds no slot.
Timed with HIP events, one event pair per call, over interleaved rounds of calls that rotate over distinct frame
buffers (the method of tools/udp_bench.py): each round times the ARP call, then the UDP call, so the rounds are
A/B pairs. Prints the per-round medians, the medians over rounds with the rounds' spread, and one JSON line.

    python tools/arp_bench.py --shape a|b|c [--rounds 8] [--launches 100] [--buffers 4] [--baseline-lib SO] [--out FILE]
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


def host_ip(h):
    return bytes([10, 1, h >> 8, h & 255])


def batch_of(rng, shape, n_hosts):
    """(buffer, offsets, lengths, is_request): shape a and b are 1,500-byte UDP frames at a stride of 1,500 (in b every
    hundredth slot holds a 60-byte request instead); shape c is 60-byte requests at a stride of 60. The j-th
    request asks for host j mod n_hosts."""
    from oracle import coracle
    from seqs_amd import synth

    frame_len = 60 if shape == "c" else 1500
    rows = np.zeros((N, frame_len), dtype=np.uint8)
    ln = np.full(N, frame_len, dtype=np.uint32)
    is_req = np.ones(N, dtype=bool) if shape == "c" else (np.arange(N) % 100 == 99) & (shape == "b")
    if shape != "c":
        rows[:] = synth.make_frames(N, frame_len, 17, rng)
        rows[:, 30:34] = LOCAL_IP
    idx = np.flatnonzero(is_req)
    req = np.zeros((idx.size, 60), dtype=np.uint8)
    req[:, 0:6] = 255
    req[:, 6:12] = req[:, 22:28] = np.stack([np.full(idx.size, 2, np.uint8), np.full(idx.size, 7, np.uint8), (idx >> 24).astype(np.uint8),
                                             (idx >> 16).astype(np.uint8), (idx >> 8).astype(np.uint8), idx.astype(np.uint8)], axis=1)
    req[:, 12:22] = np.frombuffer(bytes([8, 6, 0, 1, 8, 0, 6, 4, 0, 1]), dtype=np.uint8)
    req[:, 28:32] = np.stack([np.full(idx.size, 172, np.uint8), (idx >> 16).astype(np.uint8) + 16, (idx >> 8).astype(np.uint8),
                              idx.astype(np.uint8)], axis=1)
    which = np.arange(idx.size) % max(n_hosts, 1)
    req[:, 38:42] = np.stack([np.full(idx.size, 10, np.uint8), np.full(idx.size, 1, np.uint8), (which >> 8).astype(np.uint8),
                              which.astype(np.uint8)], axis=1)
    rows[idx, :60] = req
    rows[idx, 60:] = 0
    ln[idx] = 60
    flat = np.concatenate([rows.reshape(-1), np.zeros(64, dtype=np.uint8)])
    off = np.arange(N, dtype=np.uint64) * frame_len
    if shape != "c":
        _, st = coracle.fill_batch(flat, off, ln, 0, coracle.FILL_CSUM)
        assert (st[~is_req] == 0).all() and (st[is_req] == 4).all()
    return flat, off, ln, is_req


def baseline_of(path):
    """fs_udp_flows_batch of another library, with a context of its own: (function, context, library)."""
    from seqs_amd import abi

    lib = ctypes.CDLL(path)
    for name in ("fs_ctx_create", "fs_ctx_destroy", "fs_last_error"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = abi.PROTOTYPES[name]
    lib.fs_udp_flows_batch.restype, lib.fs_udp_flows_batch.argtypes = abi.UDP_PROTOTYPES["fs_udp_flows_batch"]
    ctx = ctypes.c_void_p()
    assert lib.fs_ctx_create(0, ctypes.byref(ctx)) == 0
    return lib.fs_udp_flows_batch, ctx, lib


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--shape", choices=("a", "b", "c"), required=True)
    p.add_argument("--rounds", type=int, default=8)
    p.add_argument("--launches", type=int, default=100)
    p.add_argument("--buffers", type=int, default=4)
    p.add_argument("--baseline-lib", default=None, help="the libframesum.so whose fs_udp_flows_batch is the baseline")
    p.add_argument("--out", default=None, help="also write the report to this file")
    a = p.parse_args()
    assert a.rounds >= 1

    import torch

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    from seqs_amd import (ARP_ANSWERED, ARP_FULL, ARP_HOST_DTYPE, ARP_HOST_OUT_DTYPE, ARP_NONE, ARP_PAD, CLOSE_OUT_DTYPE, CONNECT_OUT_DTYPE,
                          FLOW_DTYPE, FLOW_TOTALS_DTYPE, RUN_DTYPE, SND_DTYPE, SND_OUT_DTYPE, SOCK_DTYPE, SOCK_OUT_DTYPE,
                          UDP_PORT_OUT_DTYPE, Engine, arp_host)

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    eng = Engine(0)
    stream = torch.cuda.Stream(dev)

    n_hosts = {"a": 0, "b": 64, "c": 1000}[a.shape]
    buf, off, ln, is_req = batch_of(rng, a.shape, n_hosts)
    n_req = int(is_req.sum())
    per_host = min(-(-n_req // max(n_hosts, 1)), 65536 // max(n_hosts, 1))
    hosts = (np.concatenate([arp_host(host_ip(h), bytes([2, 0, 0, 0, h >> 8, h & 255]), h * per_host, per_host) for h in range(n_hosts)])
             if n_hosts else np.zeros(0, dtype=ARP_HOST_DTYPE))
    hosts = np.ascontiguousarray(hosts, dtype=ARP_HOST_DTYPE)
    n_reply = n_hosts * per_host
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
    closers_out, socks_close = empty((1, CLOSE_OUT_DTYPE.itemsize)), empty((1, CLOSE_OUT_DTYPE.itemsize))
    ctl_code = empty((N,))
    openers_out = empty((1, CONNECT_OUT_DTYPE.itemsize))
    replies = torch.zeros((64,), dtype=torch.uint8, device=dev)
    reply_out, reply_status = empty((1, 2), torch.int32), empty((1,))
    cells = torch.zeros((8,), dtype=torch.uint8, device=dev)
    ports_out = empty((1, UDP_PORT_OUT_DTYPE.itemsize))
    port_of, cell_of = empty((N,), torch.int32), empty((N,), torch.int32)
    hosts_out = empty((max(n_hosts, 1), ARP_HOST_OUT_DTYPE.itemsize))
    arp_frames = torch.zeros((max(n_reply, 1) * 64,), dtype=torch.uint8, device=dev)
    arp_out, arp_status = empty((max(n_reply, 1), 2), torch.int32), empty((max(n_reply, 1),))
    arp_code, arp_of = empty((N,)), empty((N,), torch.int32)
    vp = ctypes.c_void_p

    def args_of(ctx, b, arp):
        head = (ctx, vp(frames[b].data_ptr()), vp(d_off.data_ptr()), vp(d_len.data_ptr()), N, 0, 0,
                vp(socks.ctypes.data), 0, vp(rings.data_ptr()), 64, vp(socks_out.data_ptr()), vp(delivered.data_ptr()),
                vp(snd.ctypes.data), vp(snd_out.data_ptr()), vp(code.data_ptr()))
        listen = (None, 0, None, 0, 0, None, None, vp(accept_of.data_ptr()), None, None, None)
        mid = (None, 0, vp(closers_out.data_ptr()), vp(socks_close.data_ptr()), vp(ctl_code.data_ptr()))
        opening = (None, 0, 0, vp(openers_out.data_ptr()), vp(replies.data_ptr()), vp(reply_out.data_ptr()), vp(reply_status.data_ptr()))
        udp = (None, 0, vp(cells.data_ptr()), 8, vp(ports_out.data_ptr()), vp(port_of.data_ptr()), vp(cell_of.data_ptr()))
        more = (vp(hosts.ctypes.data) if n_hosts else None, n_hosts, None, 0, n_reply, ARP_PAD, vp(hosts_out.data_ptr()), None,
                vp(arp_frames.data_ptr()), vp(arp_out.data_ptr()), vp(arp_status.data_ptr()), vp(arp_code.data_ptr()),
                vp(arp_of.data_ptr())) if arp else ()
        tail = (None, 0, vp(runs.data_ptr()), vp(flows_t.data_ptr()), vp(order_t.data_ptr()), vp(run_of.data_ptr()),
                vp(ftotals.data_ptr()), vp(out.data_ptr()), vp(status.data_ptr()), vp(stream.cuda_stream))
        return head + listen + mid + opening + udp + more + tail

    base_fn, base_ctx, base_lib = (eng.lib.fs_udp_flows_batch, eng._ctx, eng.lib) if a.baseline_lib is None else baseline_of(a.baseline_lib)

    def kind(arp):
        fn, ctx, lib = (eng.lib.fs_arp_flows_batch, eng._ctx, eng.lib) if arp else (base_fn, base_ctx, base_lib)
        args = [args_of(ctx, b, arp) for b in range(a.buffers)]

        def run(b):
            st = fn(*args[b])
            assert st == 0, lib.fs_last_error(ctx)
        return run

    def fills(b):  # the bound of shape a, on its own: two fills of n entries, one of bytes and one of 32-bit words
        arp_code.fill_(0)
        arp_of.fill_(-1)

    kinds = [("arp", kind(True)), ("udp", kind(False))] + ([("fills", fills)] if a.shape == "a" else [])

    # checked once: the shape does what it says
    with torch.cuda.stream(stream):
        kinds[0][1](0)
    stream.synchronize()
    st, co, of = status.cpu().numpy(), arp_code.cpu().numpy(), arp_of.cpu().numpy().view(np.uint32)
    assert (st[is_req] == 4).all() and (st[~is_req] == 0).all()
    assert (co[~is_req] == 0).all() and (of[~is_req] == ARP_NONE).all()
    if n_hosts:
        idx = np.flatnonzero(is_req)
        j = np.arange(idx.size)
        seen = np.bincount(j % n_hosts, minlength=n_hosts)
        room = j // n_hosts < per_host
        assert (co[idx] == np.where(room, ARP_ANSWERED, ARP_FULL)).all()
        assert (of[idx] == np.where(room, (j % n_hosts) * per_host + j // n_hosts, ARP_NONE)).all()
        o = hosts_out.cpu().numpy().reshape(-1).view(ARP_HOST_OUT_DTYPE)
        assert (o["n_answered"] == np.minimum(seen, per_host)).all() and (o["n_requests"] == seen).all()
        built = arp_frames.cpu().numpy()
        last = int(np.flatnonzero(room)[-1])  # the last answered request's reply: to its sender, from the host it asked for
        k, at = int(idx[last]), int(of[idx[last]]) * 64
        assert bytes(built[at : at + 6]) == bytes(buf[int(off[k]) + 6 : int(off[k]) + 12]) and bytes(built[at + 28 : at + 32]) == host_ip(last % n_hosts)
        assert int(arp_status.cpu().numpy()[at // 64]) == 4

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
        lines.append(f"pair {rd}: " + "  ".join(f"{name} {rounds[name][-1]:9.2f} us" for name, _ in kinds) +
                     f"  arp - udp {rounds['arp'][-1] - rounds['udp'][-1]:8.2f} us")
    med = {name: statistics.median(v) for name, v in rounds.items()}
    spread = {name: [round(min(v), 2), round(max(v), 2)] for name, v in rounds.items()}
    pair_diffs = [x - y for x, y in zip(rounds["arp"], rounds["udp"])]
    diff = statistics.median(pair_diffs)
    res = {
        "shape": a.shape, "frames": N, "requests": n_req, "n_hosts": n_hosts, "reply_slots": n_reply, "buffers": a.buffers,
        "pairs": a.rounds, "launches_per_round": a.launches, "baseline": "parent library" if a.baseline_lib else "same library",
        **{name + "_us": round(v, 2) for name, v in med.items()}, "round_min_max_us": spread,
        "arp_minus_udp_us": round(diff, 2), "pair_diff_min_max_us": [round(min(pair_diffs), 2), round(max(pair_diffs), 2)],
        "arp_over_udp": round(med["arp"] / med["udp"], 3),
        "last_kernel": eng.last_kernel(), "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
    }
    lines.append("median of pairs [min, max]: " + "  ".join(f"{name} {med[name]:.2f} us {spread[name]}" for name, _ in kinds) +
                 f"  arp - udp = {diff:.2f} us [{min(pair_diffs):.2f}, {max(pair_diffs):.2f}]")
    if a.shape == "a":
        bound = med["fills"]
        res["bound_us"], res["within_bound"] = round(bound, 2), bool(diff <= bound)
        lines.append(f"bound: two n-entry fills take {bound:.2f} us {spread['fills']}; arp - udp = {diff:.2f} us: "
                     f"{'within' if diff <= bound else 'OUTSIDE'} the bound")
    lines.append(json.dumps(res))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("command: python " + " ".join(sys.argv) + "\n" + text + "\n")
    if a.baseline_lib is not None:
        base_lib.fs_ctx_destroy(base_ctx)
    eng.close()


if __name__ == "__main__":
    main()
