"""The expected output of the ring send (fs_send_rings_batch), from code the kernel does not share:
the per-socket rule of include/framesum_send.h in plain Python, the ring range unwrapped into linear
bytes, Seq, Ack, Window and the flags written into a copy of the template, and from there the pinned
restatement of the TX frame build (segment_ref.send_frames, segment_ref.layout and the C oracle's
fill). Shared by the CPU and the GPU tests."""
import numpy as np

import segment_ref as sref

FCS_APPEND = sref.FCS_APPEND
TX_ACK, TX_FIN, TX_PSH = 1, 2, 4
NONE = 0xFFFFFFFF
MAX_FRAMES = 4096
M32 = 0xFFFFFFFF


def sock(hdr, mss, ring_off, ring_size, ring_rpos, ring_buffered, snd_una=0, snd_nxt=0, snd_wnd=1 << 30, rcv_nxt=0,
         rcv_wnd=65535, max_frames=0, flags=0) -> dict:
    return dict(hdr=bytes(hdr), mss=mss, ring_off=ring_off, ring_size=ring_size, ring_rpos=ring_rpos,
                ring_buffered=ring_buffered, snd_una=snd_una, snd_nxt=snd_nxt, snd_wnd=snd_wnd, rcv_nxt=rcv_nxt,
                rcv_wnd=rcv_wnd, max_frames=max_frames, flags=flags)


def socks_of(socks):
    """A list of sock() dicts as the TX_SOCK_DTYPE array the binding takes."""
    from seqs_amd.framesum import TX_SOCK_DTYPE

    a = np.zeros(len(socks), dtype=TX_SOCK_DTYPE)
    for i, s in enumerate(socks):
        for k, v in s.items():
            a[k][i] = np.frombuffer(v, dtype=np.uint8) if k == "hdr" else v
    return a


def rule(s: dict) -> dict:
    """data, fin, S and the state after the call."""
    in_flight = (s["snd_nxt"] - s["snd_una"]) & M32
    room = s["snd_wnd"] - in_flight if s["snd_wnd"] > in_flight else 0
    data = min(s["ring_buffered"], room, (s["max_frames"] or MAX_FRAMES) * s["mss"])
    fin = bool(s["flags"] & TX_FIN) and data == s["ring_buffered"]
    S = -(-data // s["mss"])
    if S == 0 and (fin or s["flags"] & TX_ACK):
        S = 1
    ident = int.from_bytes(s["hdr"][18:20], "big")
    for _ in range(S):
        ident = sref.prand16(ident)
    return dict(data=data, fin=fin, S=S, snd_nxt=(s["snd_nxt"] + data + fin) & M32,
                ring_rpos=(s["ring_rpos"] + data) % s["ring_size"], ring_buffered=s["ring_buffered"] - data, ip_id=ident,
                sent=TX_FIN if fin else (TX_ACK if S and data == 0 else 0))


def ring_bytes(rings: np.ndarray, s: dict, count: int) -> bytes:
    """The `count` bytes from the ring's read position on, unwrapped."""
    at = (s["ring_rpos"] + np.arange(count, dtype=np.int64)) % s["ring_size"] + s["ring_off"]
    return rings[at].tobytes()


def template(s: dict, r: dict) -> bytes:
    """The socket's header as CalculateHeaders fills it for the LAST frame of the call."""
    h = bytearray(s["hdr"])
    h[38:42] = s["snd_nxt"].to_bytes(4, "big")
    h[42:46] = s["rcv_nxt"].to_bytes(4, "big")
    h[47] = 0x10 | (0x08 if s["flags"] & TX_PSH and r["data"] else 0) | (0x01 if r["fin"] else 0)
    h[48:50] = min(s["rcv_wnd"], 65535).to_bytes(2, "big")
    return bytes(h)


def frames_of(socks, rings: np.ndarray):
    """(the batch's frames with zero checksum fields, the socks_out records) in socket order."""
    from seqs_amd.framesum import TX_SOCK_OUT_DTYPE

    frames, outs = [], np.zeros(len(socks), dtype=TX_SOCK_OUT_DTYPE)
    for i, s in enumerate(socks):
        r = rule(s)
        outs[i] = (r["snd_nxt"], r["ring_rpos"], r["ring_buffered"], r["data"], r["S"], len(frames) if r["S"] else NONE,
                   r["ip_id"], r["sent"])
        if r["S"]:
            mine = sref.send_frames(template(s, r), ring_bytes(rings, s, r["data"]), s["mss"])
            assert len(mine) == r["S"]
            frames += mine
    return frames, outs


def segment_sends(socks, rings: np.ndarray):
    """The same frames asked of the TX frame build: (specs, payload) as segment_ref.make_sends and
    segment_ref.expected take them, one send per socket that makes a frame. Its header is the template
    with Seq, Ack, the window and the last frame's flags written in, its payload the socket's sent bytes
    unwrapped (the sends' ranges lie back to back in `payload`), its mss the socket's."""
    specs, blob = [], b""
    for s in socks:
        r = rule(s)
        if r["S"]:
            specs.append((template(s, r), len(blob), r["data"], s["mss"]))
            blob += ring_bytes(rings, s, r["data"])
    return specs, np.frombuffer(blob + b"\0", dtype=np.uint8)[:-1].copy()


def expected(socks, rings: np.ndarray, mtu: int, flags: int, align: int, noise: np.ndarray):
    """(buffer, offsets, lengths, digests, status, socks_out) a build of `socks` (sock() dicts) into a
    copy of `noise` must give."""
    from oracle import coracle

    frames, outs = frames_of(socks, rings)
    lens = np.array([len(f) for f in frames], dtype=np.uint32)
    offs, total = sref.layout(lens, flags, align)
    buf = noise.copy()
    assert total <= buf.size
    for f, o in zip(frames, offs):
        buf[int(o) : int(o) + len(f)] = np.frombuffer(f, dtype=np.uint8)
    if len(frames) == 0:
        return buf, offs, lens, np.zeros(0, dtype=coracle.DIGEST_DTYPE), np.zeros(0, dtype=np.uint8), outs
    dig, st = coracle.fill_batch(buf, offs, lens, mtu, coracle.FILL_CSUM | flags)
    return buf, offs, lens, dig, st, outs


def filled_rings(rng, socks, size=None) -> np.ndarray:
    """Random bytes for a rings buffer that ends with the last ring's last byte (or has `size` bytes)."""
    end = max((s["ring_off"] + s["ring_size"] for s in socks), default=0)
    return rng.integers(0, 256, end if size is None else size, dtype=np.uint8)
