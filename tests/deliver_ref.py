"""The expected output of the in-order TCP delivery (fs_deliver_flows_batch), restated sequentially
from the contract in include/framesum_deliver.h with code the kernels do not share: the flows part is
tests/flows_ref.py's, and each listed socket's flow is walked frame by frame, in Python integers, the
admitted payloads written byte range by byte range into a copy of the rings."""
import numpy as np

import flows_ref
from flows_ref import ACK, FIN  # noqa: F401

SYN, RST = 0x02, 0x04
NONE = 0xFFFFFFFF
M32 = 1 << 32


def sock(key, rcv_nxt, ring_off, ring_size, rcv_wnd=65535, snd_nxt=0, ring_wpos=0, ring_free=None):
    """One SOCK_DTYPE record."""
    from seqs_amd.framesum import SOCK_DTYPE

    s = np.zeros(1, dtype=SOCK_DTYPE)
    s["key"][0] = np.frombuffer(bytes(key), dtype=np.uint8)
    s["rcv_nxt"], s["rcv_wnd"], s["snd_nxt"] = rcv_nxt % M32, rcv_wnd, snd_nxt % M32
    s["ring_off"], s["ring_size"], s["ring_wpos"] = ring_off, ring_size, ring_wpos
    s["ring_free"] = ring_size if ring_free is None else ring_free
    return s


def socks_of(*records):
    from seqs_amd.framesum import SOCK_DTYPE

    return np.concatenate(records) if records else np.zeros(0, dtype=SOCK_DTYPE)


def key_of_header(hdr: bytes) -> bytes:
    """The key of the flow whose frames start with the 54-byte header `hdr` (IHL 5)."""
    return flows_ref.flow_key(hdr)


def ring_write(ring: np.ndarray, wpos: int, data: bytes) -> int:
    """`data` into the ring from wpos on, wrapping; returns the new wpos. (len(data) <= len(ring).)"""
    size = ring.size
    first = min(len(data), size - wpos)
    ring[wpos : wpos + first] = np.frombuffer(data[:first], dtype=np.uint8)
    if first < len(data):
        ring[: len(data) - first] = np.frombuffer(data[first:], dtype=np.uint8)
    return (wpos + len(data)) % size


def admitted(seq, ack, length, flags, nxt, free, rcv_wnd, snd_nxt) -> bool:
    """Rules (a) to (d) for a considered frame."""
    fin = 1 if flags & FIN else 0
    if seq != nxt:                                   # (a)
        return False
    if length + fin > rcv_wnd:                       # (b)
        return False
    if flags & ACK:                                  # (c): Ack - snd_nxt as a signed 32-bit number
        d = (ack - snd_nxt) % M32
        if 0 < d < (1 << 31):
            return False
    return length <= free                            # (d)


def walk(frames, st, socks, rings, e):
    """The delivery part: (socks_out, delivered, rings) for the batch's frames (a list of bytes), their
    verdicts `st` and the flows part `e` (flows_ref.expected's dict)."""
    from seqs_amd.framesum import SOCK_OUT_DTYPE

    rings = rings.copy()
    delivered = np.zeros(len(frames), dtype=np.uint8)
    out = np.zeros(len(socks), dtype=SOCK_OUT_DTYPE)
    order = e["order"]
    flow_of_key = {flows_ref.flow_key(frames[int(order[int(fl["first_frame"])])]): f for f, fl in enumerate(e["flows"])}
    for s, sk in enumerate(socks):
        nxt, wpos, free = int(sk["rcv_nxt"]), int(sk["ring_wpos"]), int(sk["ring_free"])
        off, size = int(sk["ring_off"]), int(sk["ring_size"])
        ring = rings[off : off + size]
        f = flow_of_key.get(bytes(sk["key"]), None)
        rec = dict(bytes=0, n_delivered=0, n_dropped=0, flow=NONE, stop=NONE)
        if f is not None:
            fl = e["flows"][f]
            first, count = int(fl["first_frame"]), int(fl["n_frames"])
            rec["flow"], rec["stop"] = f, first + count
            for k in range(first, first + count):
                i = int(order[k])
                fr = frames[i]
                l4 = 14 + (fr[14] & 15) * 4
                seq, ack = int.from_bytes(fr[l4 + 4 : l4 + 8], "big"), int.from_bytes(fr[l4 + 8 : l4 + 12], "big")
                flags = fr[l4 + 13]
                a, b = flows_ref.payload_range(fr)
                if flags & (SYN | RST):
                    rec["stop"] = k
                    break
                if b - a == 0 and not flags & FIN:
                    continue
                if admitted(seq, ack, b - a, flags, nxt, free, int(sk["rcv_wnd"]), int(sk["snd_nxt"])):
                    wpos = ring_write(ring, wpos, fr[a:b])
                    free -= b - a
                    nxt = (nxt + (b - a) + (1 if flags & FIN else 0)) % M32
                    delivered[i] = 1
                    rec["bytes"] += b - a
                    rec["n_delivered"] += 1
                    if flags & FIN:
                        rec["stop"] = k + 1
                        break
                else:
                    delivered[i] = 2
                    rec["n_dropped"] += 1
        out[s] = (nxt, wpos, free, rec["bytes"], rec["n_delivered"], rec["n_dropped"], rec["flow"], rec["stop"])
    return out, delivered, rings


def expected(buf, offsets, lengths, mtu, flags, noise, plead, cap, socks, rings):
    """flows_ref.expected's dict plus socks_out, delivered and rings (the whole buffer)."""
    e = flows_ref.expected(buf, offsets, lengths, mtu, flags, noise, plead, cap)
    raw = buf.tobytes()
    room = 4 if flags & flows_ref.RX_FCS else 0
    frames = [raw[int(o) : int(o) + max(0, int(l) - room)] for o, l in zip(offsets, lengths)]
    e["socks_out"], e["delivered"], e["rings"] = walk(frames, e["st"], socks, rings, e)
    return e
