"""The expected output of the TX frame build (fs_segment_batch), from code the kernel does not
share: a pure-Python restatement of the reference's per-segment header fields
(stacks/port_tcp.go:162-194 CalculateHeaders, PutHeaders port_tcp.go:95-106 / port_udp.go:68-78)
that slices the payload, puts the fields, steps prand16, leaves both checksum fields zero and packs
the frames at the layout's offsets into a noise-filled buffer; the C oracle's fill_batch then writes
the checksums and the FCS and gives the digests and verdicts. Shared by the CPU and the GPU tests."""
import numpy as np

FCS_APPEND = 2


def prand16(x: int) -> int:  # stacks/port_tcp.go:197-203
    x ^= (x << 7) & 0xFFFF
    x ^= x >> 9
    x ^= (x << 8) & 0xFFFF
    return x


def n_frames(mss: int, length: int) -> int:
    return 1 if mss == 0 or length == 0 else -(-length // mss)


def send_frames(hdr: bytes, payload: bytes, mss: int) -> list:
    """The frames of one send, checksum fields zero."""
    udp = hdr[23] == 17
    H = 42 if udp else 54
    L, S = len(payload), n_frames(mss, len(payload))
    ident = int.from_bytes(hdr[18:20], "big")
    frames = []
    for k in range(S):
        chunk = payload[k * mss : min(L, (k + 1) * mss)] if mss else payload
        h = bytearray(hdr[:H])
        h[14] = 0x45  # IPv4Header.Put forces the version (eth/headers.go:289-291)
        h[16:18] = (H - 14 + len(chunk)).to_bytes(2, "big")
        h[18:20] = ident.to_bytes(2, "big")
        ident = prand16(ident)  # stepped once per CalculateHeaders (:173)
        h[24:26] = b"\0\0"
        if udp:
            h[38:40] = (8 + L).to_bytes(2, "big")
            h[40:42] = b"\0\0"
        else:
            seq = (int.from_bytes(hdr[38:42], "big") + k * mss) & 0xFFFFFFFF
            h[38:42] = seq.to_bytes(4, "big")
            if k != S - 1:
                h[47] &= ~0x09 & 0xFF  # FIN and PSH only on the last segment
            h[50:54] = b"\0\0\0\0"  # checksum, urgent pointer (:189)
        frames.append(bytes(h) + bytes(chunk))
    return frames


def layout(lens, flags: int, align: int):
    """Offsets of frames of the given lengths, and the sum of their slots."""
    fcs = 4 if flags & FCS_APPEND else 0
    off, at = [], 0
    for n in lens:
        off.append(at)
        at += (n + fcs + align - 1) // align * align
    return np.array(off, dtype=np.uint64), at


def make_sends(specs):
    """specs: (hdr bytes, payload_off, payload_len, mss) per send -> a SEND_DTYPE array."""
    from seqs_amd.framesum import SEND_DTYPE

    sends = np.zeros(len(specs), dtype=SEND_DTYPE)
    for i, (hdr, off, ln, mss) in enumerate(specs):
        sends["hdr"][i, : len(hdr)] = np.frombuffer(bytes(hdr), dtype=np.uint8)
        sends["mss"][i], sends["payload_off"][i], sends["payload_len"][i] = mss, off, ln
    return sends


def expected(specs, payload: np.ndarray, mtu: int, flags: int, align: int, noise: np.ndarray):
    """(buffer, offsets, lengths, digests, status) a build of `specs` into a copy of `noise` must give."""
    from oracle import coracle

    frames = []
    pb = payload.tobytes()
    for hdr, off, ln, mss in specs:
        frames += send_frames(bytes(hdr), pb[off : off + ln], mss)
    lens = np.array([len(f) for f in frames], dtype=np.uint32)
    offs, total = layout(lens, flags, align)
    buf = noise.copy()
    assert total <= buf.size
    for f, o in zip(frames, offs):
        buf[int(o) : int(o) + len(f)] = np.frombuffer(f, dtype=np.uint8)
    dig, st = coracle.fill_batch(buf, offs, lens, mtu, coracle.FILL_CSUM | flags)
    return buf, offs, lens, dig, st


def tcp_header(rng, seq=None, flags=0x19, ident=None) -> bytes:
    h = bytearray(rng.integers(0, 256, 54, dtype=np.uint8).tobytes())
    h[12:14] = b"\x08\x00"
    h[14] = 0x45
    h[23] = 6
    h[34:38] = b"\x12\x34\x00\x50"
    h[46] = 0x50
    h[47] = flags
    if seq is not None:
        h[38:42] = seq.to_bytes(4, "big")
    if ident is not None:
        h[18:20] = ident.to_bytes(2, "big")
    return bytes(h)


def udp_header(rng) -> bytes:
    h = bytearray(rng.integers(0, 256, 42, dtype=np.uint8).tobytes())
    h[12:14] = b"\x08\x00"
    h[14] = 0x45
    h[23] = 17
    h[34:38] = b"\x00\x44\x00\x43"
    return bytes(h)


def kat_sends():
    """From tests/golden/kats.json: every TCP or UDP frame with IHL 5 (and data offset 5), as a send
    of its own header bytes and its own payload with mss 0. Returns (frames, specs, payload)."""
    import json
    import os

    kats = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kats.json")))
    frames, specs, blob = [], [], b""
    for f in (bytes.fromhex(e["hex"]) for e in kats["frames"]):
        if len(f) < 42 or f[12:14] != b"\x08\x00" or f[14] != 0x45 or f[23] not in (6, 17):
            continue
        H = 42 if f[23] == 17 else 54
        if len(f) < H or (H == 54 and f[46] >> 4 != 5):
            continue
        frames.append(f)
        specs.append((f[:H], len(blob), len(f) - H, 0))
        blob += f[H:]
    return frames, specs, np.frombuffer(blob + b"\0", dtype=np.uint8)[:-1].copy()
