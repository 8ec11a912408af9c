"""The expected output of the flow-aware RX coalesce (fs_coalesce_flows_batch), restated sequentially
from the semantics in include/framesum.h with code the kernels do not share: verdicts and digests
come from the C oracle, the payload ranges and the join rule from tests/coalesce_ref.py, the flows
from a dict keyed by the 13 key bytes in insertion order, and the result is packed into a
noise-filled buffer."""
import numpy as np

from coalesce_ref import (ACK, FIN, NO_RUN, PSH, RX_FCS, finish, flow_header, joins, pack, payload_range,  # noqa: F401
                          segments, tcp_frame, udp_frame)


def flow_key(f: bytes) -> bytes:
    """Protocol, source and destination address, source and destination port."""
    l4 = 14 + (f[14] & 15) * 4
    return bytes([f[23]]) + bytes(f[26:34]) + bytes(f[l4 : l4 + 4])


def expected(buf: np.ndarray, offsets, lengths, mtu: int, flags: int, noise: np.ndarray, plead: int = 0, cap=None):
    """What fs_coalesce_flows_batch of the batch into noise[plead : plead + cap] must give: a dict of
    the whole payload buffer (a copy of `noise` with the payloads packed in), runs (RUN_DTYPE), flows
    (FLOW_DTYPE), order, run_of, the four totals, digests and status."""
    from oracle import coracle
    from seqs_amd.framesum import FLOW_DTYPE, RUN_DTYPE

    offsets = np.asarray(offsets, dtype=np.uint64)
    lengths = np.asarray(lengths, dtype=np.uint32)
    if flags & RX_FCS:
        dig, st = coracle.digest_fcs_batch(buf, offsets, lengths, mtu)
    else:
        dig, st = coracle.digest_batch(buf, offsets, lengths, mtu)
    n = lengths.size
    cap = noise.size - plead if cap is None else cap
    raw = buf.tobytes()
    frame = lambda i: raw[int(offsets[i]) : int(offsets[i]) + int(lengths[i])]  # noqa: E731
    # the flows, in the order of their first frames, each with its frames in batch order
    table = {}
    for i in range(n):
        if st[i] == 0:
            table.setdefault(flow_key(frame(i)), []).append(i)
    order = [i for members in table.values() for i in members]
    out = noise.copy()
    runs, flows, run_of, at = [], [], np.full(n, NO_RUN, dtype=np.uint32), 0
    k = 0
    for members in table.values():
        fl = dict(payload_off=at, payload_len=0, first_run=len(runs), n_runs=0, first_frame=k, n_frames=len(members))
        prev = None
        for i in members:
            f = frame(i)
            s, e = payload_range(f)
            if prev is not None and joins(prev, f):
                r = runs[-1]
                r["n_frames"] += 1
                r["payload_len"] = (r["payload_len"] + e - s) % (1 << 32)  # a run past 4 GiB: its length modulo 2^32
                r["tcp_flags"] |= f[47] & (FIN | PSH)
            else:
                l4 = 14 + (f[14] & 15) * 4
                runs.append(dict(payload_off=at, payload_len=e - s, first_frame=k, n_frames=1,
                                 tcp_flags=f[l4 + 13] if f[23] == 6 else 0))
                fl["n_runs"] += 1
            run_of[i] = len(runs) - 1
            if at + (e - s) <= cap:
                out[plead + at : plead + at + (e - s)] = np.frombuffer(f[s:e], dtype=np.uint8)
            at += e - s
            fl["payload_len"] += e - s
            prev = f
            k += 1
        flows.append(fl)
    ra = np.zeros(len(runs), dtype=RUN_DTYPE)
    for j, r in enumerate(runs):
        for key, v in r.items():
            ra[key][j] = v
    fa = np.zeros(len(flows), dtype=FLOW_DTYPE)
    for j, fl in enumerate(flows):
        for key, v in fl.items():
            fa[key][j] = v
    return dict(payload=out, runs=ra, flows=fa, order=np.array(order, dtype=np.uint32), run_of=run_of, payload_bytes=at,
                n_runs=len(runs), n_flows=len(flows), n_accepted=len(order), dig=dig, st=st)


def interleave(groups) -> list:
    """Round-robin over the groups: the first of each, then the second of each, ... (shorter groups
    drop out). Returns a list of (group, index in group)."""
    out, depth = [], 0
    while any(depth < len(g) for g in groups):
        out += [(gi, depth) for gi, g in enumerate(groups) if depth < len(g)]
        depth += 1
    return out
