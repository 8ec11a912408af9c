"""The expected output of the RX coalesce (fs_coalesce_batch), from code the kernels do not share:
verdicts and digests come from the C oracle, the payload ranges (stacks/portstack.go:217, :239,
:301-303), the join rule and the runs from a plain sequential loop written from the semantics in
include/framesum.h, and the result is packed into a noise-filled buffer. Also the frame builders the
CPU and the GPU tests share."""
import os
import re

import numpy as np

RX_FCS = 1
NO_RUN = 0xFFFFFFFF
FIN, SYN, RST, PSH, ACK, URG = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
# header bytes a run's frames may differ in: TotalLength, ID, IPv4 checksum, Seq, TCP checksum
VARIED = [16, 17, 18, 19, 24, 25, 38, 39, 40, 41, 50, 51]
COMPARED = [i for i in range(54) if i not in VARIED]  # (byte 47 less its FIN and PSH bits)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scan_block() -> int:
    """The scan kernels' block size, as seqs_amd/csrc/framesum_coalesce.h exports it."""
    src = open(os.path.join(ROOT, "seqs_amd", "csrc", "framesum_coalesce.h")).read()
    return int(re.search(r"constexpr uint32_t kScanBlock = (\d+);", src).group(1))


# ---- the semantics, restated ---------------------------------------------------------------------

def payload_range(f: bytes):
    """(start, end) of an accepted frame's payload."""
    l4 = 14 + (f[14] & 15) * 4
    end = 14 + int.from_bytes(f[16:18], "big")
    if f[23] == 17:
        return l4 + 8, end
    return l4 + (f[l4 + 12] >> 4) * 4, end


def plain_tcp(f: bytes) -> bool:
    return f[23] == 6 and (f[14] & 15) == 5 and (f[46] >> 4) == 5


def joins(p: bytes, c: bytes) -> bool:
    """Does accepted frame c continue accepted frame p?"""
    if not (plain_tcp(p) and plain_tcp(c)):
        return False
    (ps, pe), (cs, ce) = payload_range(p), payload_range(c)
    if pe - ps == 0 or ce - cs == 0:
        return False
    if (p[47] | c[47]) & (SYN | RST | URG) or p[47] & (FIN | PSH):
        return False
    if int.from_bytes(c[38:42], "big") != (int.from_bytes(p[38:42], "big") + (pe - ps)) % (1 << 32):
        return False
    a, b = bytearray(p[:54]), bytearray(c[:54])
    for h in (a, b):
        for i in VARIED:
            h[i] = 0
        h[47] &= ~(FIN | PSH) & 0xFF
    return a == b


def expected(buf: np.ndarray, offsets, lengths, mtu: int, flags: int, noise: np.ndarray, plead: int = 0, cap=None):
    """What a coalesce of the batch into noise[plead : plead + cap] must give: a dict of the whole
    payload buffer (a copy of `noise` with the payloads packed in), runs (RUN_DTYPE, n_runs of them),
    run_of, payload_bytes, n_runs, digests and status."""
    from oracle import coracle
    from seqs_amd.framesum import RUN_DTYPE

    offsets = np.asarray(offsets, dtype=np.uint64)
    lengths = np.asarray(lengths, dtype=np.uint32)
    if flags & RX_FCS:
        dig, st = coracle.digest_fcs_batch(buf, offsets, lengths, mtu)
    else:
        dig, st = coracle.digest_batch(buf, offsets, lengths, mtu)
    n = lengths.size
    cap = noise.size - plead if cap is None else cap
    out = noise.copy()
    raw = buf.tobytes()
    runs, run_of, at, prev = [], np.full(n, NO_RUN, dtype=np.uint32), 0, None
    for i in range(n):
        if st[i] != 0:
            prev = None
            continue
        f = raw[int(offsets[i]) : int(offsets[i]) + int(lengths[i])]
        s, e = payload_range(f)
        if prev is not None and joins(prev, f):
            r = runs[-1]
            r["n_frames"] += 1
            r["payload_len"] = (r["payload_len"] + e - s) % (1 << 32)  # a run past 4 GiB: its length modulo 2^32
            r["tcp_flags"] |= f[47] & (FIN | PSH)
        else:
            l4 = 14 + (f[14] & 15) * 4
            runs.append(dict(payload_off=at, payload_len=e - s, first_frame=i, n_frames=1,
                             tcp_flags=f[l4 + 13] if f[23] == 6 else 0))
        run_of[i] = len(runs) - 1
        if at + (e - s) <= cap:
            out[plead + at : plead + at + (e - s)] = np.frombuffer(f[s:e], dtype=np.uint8)
        at += e - s
        prev = f
    ra = np.zeros(len(runs), dtype=RUN_DTYPE)
    for k, r in enumerate(runs):
        for key, v in r.items():
            ra[key][k] = v
    return dict(payload=out, runs=ra, run_of=run_of, payload_bytes=at, n_runs=len(runs), dig=dig, st=st)


# ---- frames for the tests --------------------------------------------------------------------------

def flow_header(rng, sport: int = 0x1234, flags: int = ACK) -> bytes:
    """A random 54-byte Ethernet + IPv4 + TCP header of one flow (checksum fields left to finish())."""
    h = bytearray(rng.integers(0, 256, 54, dtype=np.uint8).tobytes())
    h[12:14] = b"\x08\x00"
    h[14] = 0x45
    h[23] = 6
    h[34:36] = sport.to_bytes(2, "big")
    h[36:38] = b"\x00\x50"
    h[46] = 0x50
    h[47] = flags
    return bytes(h)


def tcp_frame(hdr: bytes, seq: int, payload: bytes, flags=None, ident=None, options: bytes = b"", pad: int = 0,
              ip_options: bytes = b"") -> bytes:
    """One TCP segment of the flow `hdr`: Seq, TotalLength, (flags, ID), `options` (a multiple of 4
    bytes) and `pad` bytes of Ethernet padding behind the IP datagram. `ip_options` (a multiple of 4
    bytes): IPv4 options; IHL and TotalLength count them and the TCP header lies behind them."""
    assert len(options) % 4 == 0 and len(ip_options) % 4 == 0 and len(ip_options) <= 40
    h = bytearray(hdr)
    h[16:18] = (40 + len(ip_options) + len(options) + len(payload)).to_bytes(2, "big")
    h[38:42] = (seq % (1 << 32)).to_bytes(4, "big")
    h[46] = (5 + len(options) // 4) << 4
    if flags is not None:
        h[47] = flags
    if ident is not None:
        h[18:20] = ident.to_bytes(2, "big")
    if ip_options:
        h[14] = (h[14] & 0xF0) | (5 + len(ip_options) // 4)
    return bytes(h[:34]) + bytes(ip_options) + bytes(h[34:]) + options + bytes(payload) + bytes(pad)


def udp_frame(rng, payload: bytes, pad: int = 0) -> bytes:
    h = bytearray(rng.integers(0, 256, 42, dtype=np.uint8).tobytes())
    h[12:14] = b"\x08\x00"
    h[14] = 0x45
    h[23] = 17
    h[16:18] = (28 + len(payload)).to_bytes(2, "big")
    h[34:38] = b"\x00\x44\x00\x43"
    h[38:40] = (8 + len(payload)).to_bytes(2, "big")
    return bytes(h) + bytes(payload) + bytes(pad)


def segments(rng, hdr: bytes, seq: int, sizes, last_flags=None, pad_to: int = 0) -> list:
    """Consecutive segments of one flow carrying random payloads of the given sizes, IDs counting up."""
    out, ident = [], int(rng.integers(0, 1 << 16))
    for k, sz in enumerate(sizes):
        fl = last_flags if (last_flags is not None and k == len(sizes) - 1) else None
        f = tcp_frame(hdr, seq, rng.integers(0, 256, sz, dtype=np.uint8).tobytes(), fl, (ident + k) & 0xFFFF)
        out.append(f + bytes(max(0, pad_to - len(f))))
        seq += sz
    return out


def finish(frames, fcs: bool = False) -> list:
    """The frames with both checksums filled by the C oracle (frames RecvEth would not checksum come
    back as they are), and with their FCS appended when `fcs`."""
    from oracle import coracle

    room = 4 if fcs else 0
    lens = np.array([len(f) for f in frames], dtype=np.uint32)
    offs = np.zeros(len(frames), dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1].astype(np.uint64) + np.uint64(room))
    buf = np.zeros(int(lens.sum()) + room * len(frames) + 8, dtype=np.uint8)
    for f, o in zip(frames, offs):
        buf[int(o) : int(o) + len(f)] = np.frombuffer(bytes(f), dtype=np.uint8)
    coracle.fill_batch(buf, offs, lens, 0, coracle.FILL_CSUM | (coracle.FCS_APPEND if fcs else 0))
    return [buf[int(o) : int(o) + int(n) + room].tobytes() for o, n in zip(offs, lens)]


def pack(frames, lead: int = 0, seed: int = 0, tail: int = 64):
    """Frames back to back (every byte alignment) behind `lead` bytes of noise and before `tail`
    bytes of it: (buf, offsets, lengths)."""
    from seqs_amd import pack_frames

    packed, offs, lens = pack_frames(frames, 1)
    total = int(lens.sum())
    buf = np.random.default_rng(1000 + seed).integers(0, 256, lead + total + tail, dtype=np.uint8)
    buf[lead : lead + total] = packed[:total]
    return buf, offs + np.uint64(lead), lens


def pack_at(frames, order, gaps, seed: int = 0, tail: int = 64):
    """The frames laid out in memory in `order` (order[k]: the batch index of the k-th frame in
    memory, every index once) with gaps[k] bytes of noise in front of the k-th, and `tail` bytes of it
    behind the last: (buf, offsets, lengths), offsets and lengths in BATCH order. The buffer itself
    starts 4-byte aligned, as pack()'s does."""
    order = [int(i) for i in order]
    assert sorted(order) == list(range(len(frames))) and len(gaps) == len(frames)
    total = sum(len(f) for f in frames) + sum(int(g) for g in gaps)
    buf = np.random.default_rng(2000 + seed).integers(0, 256, total + tail, dtype=np.uint8)
    offs = np.zeros(len(frames), dtype=np.uint64)
    lens = np.array([len(f) for f in frames], dtype=np.uint32)
    at = 0
    for i, g in zip(order, gaps):
        at += int(g)
        offs[i] = at
        buf[at : at + len(frames[i])] = np.frombuffer(bytes(frames[i]), dtype=np.uint8)
        at += len(frames[i])
    return buf, offs, lens


def with_fcs(frames, damage=()) -> list:
    """Every frame with its FCS behind it, written by the C oracle; the frames' own bytes (checksum
    fields included) stay as they are. One bit of the FCS of the frames listed in `damage` is flipped."""
    from oracle import coracle

    lens = np.array([len(f) for f in frames], dtype=np.uint32)
    offs = np.zeros(len(frames), dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1].astype(np.uint64) + np.uint64(4))
    buf = np.zeros(int(lens.sum()) + 4 * len(frames) + 8, dtype=np.uint8)
    for f, o in zip(frames, offs):
        buf[int(o) : int(o) + len(f)] = np.frombuffer(bytes(f), dtype=np.uint8)
    coracle.fill_batch(buf, offs, lens, 0, coracle.FCS_APPEND)
    for k, i in enumerate(damage):
        buf[int(offs[i]) + int(lens[i]) + k % 4] ^= np.uint8(1 << (k % 8))
    out = [buf[int(o) : int(o) + int(n) + 4].tobytes() for o, n in zip(offs, lens)]
    assert all(o[: len(f)] == bytes(f) for o, f in zip(out, frames))
    return out


def kat_frames() -> list:
    import json

    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "kats.json")))
    return [bytes.fromhex(e["hex"]) for e in kats["frames"]]
