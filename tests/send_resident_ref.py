"""The sequential model of the resident ring send (fs_send_rings_resident, include/framesum_send_resident.h),
from code the kernels do not share: the hand-off (tx_sock_from restated per socket), the checks, the rule
of tests/send_ref.py, the capacity cut and the write-back, in one loop over the sockets in index order;
and expected(), what the call must leave in every output, built from send_ref.expected() for the list of
built sockets. Shared by the CPU and the GPU tests. A socket is a send_ref.sock() dict."""
import numpy as np

import send_ref as ref

FCS_APPEND = ref.FCS_APPEND
WRITEBACK = 0x100
DEFERRED, INVALID = 0x100, 0x200
NO_RX = 0xFFFFFFFF
ACK_OWED = 1
(BAD_ETHERTYPE, BAD_IHL, BAD_PROTO, BAD_DATA_OFFSET, BAD_MSS, BAD_SOCK_FLAGS, BAD_MAX_FRAMES, BAD_RING_SIZE, BAD_RING_POS,
 BAD_BUFFERED, BAD_RING_RANGE, BAD_RX_INDEX) = range(1, 13)
BUILT, IDLE, DEFER, BAD = "built", "idle", "deferred", "invalid"


def check(s: dict, rings_bytes: int) -> int:
    """The first check a socket fails, in the order of the header's list (0: valid)."""
    h = s["hdr"]
    if h[12] != 0x08 or h[13] != 0x00:
        return BAD_ETHERTYPE
    if h[14] & 0x0F != 5:
        return BAD_IHL
    if h[23] != 6:
        return BAD_PROTO
    if h[46] >> 4 != 5:
        return BAD_DATA_OFFSET
    if not 1 <= s["mss"] <= 65495:
        return BAD_MSS
    if s["flags"] & ~7:
        return BAD_SOCK_FLAGS
    if s["max_frames"] > ref.MAX_FRAMES:
        return BAD_MAX_FRAMES
    if not 1 <= s["ring_size"] <= 1 << 31:
        return BAD_RING_SIZE
    if s["ring_rpos"] >= s["ring_size"]:
        return BAD_RING_POS
    if s["ring_buffered"] > s["ring_size"]:
        return BAD_BUFFERED
    if s["ring_off"] + s["ring_size"] > rings_bytes:
        return BAD_RING_RANGE
    return 0


def hand_off(s: dict, i: int, rx_socks_out, rx_snd_out, rx_index):
    """(the socket behind step 1, whether an RX record was applied, BAD_RX_INDEX or 0)."""
    if rx_socks_out is None:
        return s, False, 0
    r = i if rx_index is None else int(rx_index[i])
    if r == NO_RX:
        return s, False, 0
    if r >= len(rx_socks_out):
        return s, False, BAD_RX_INDEX
    t = dict(s, rcv_nxt=int(rx_socks_out["rcv_nxt"][r]), rcv_wnd=int(rx_socks_out["ring_free"][r]))
    if rx_snd_out is not None:
        t["snd_una"], t["snd_wnd"] = int(rx_snd_out["snd_una"][r]), int(rx_snd_out["snd_wnd"][r])
        if int(rx_snd_out["flags"][r]) & ACK_OWED:
            t["flags"] |= ref.TX_ACK
    return t, True, 0


def slot(length: int, flags: int, align: int) -> int:
    return (length + (4 if flags & FCS_APPEND else 0) + align - 1) // align * align


def sock_bytes(s: dict, r: dict, flags: int, align: int) -> int:
    last = r["data"] - (r["S"] - 1) * s["mss"]
    return (r["S"] - 1) * slot(54 + s["mss"], flags, align) + slot(54 + last, flags, align)


def plan(socks, rings_bytes, frames_cap, frames_bytes, flags=0, align=1, rx_socks_out=None, rx_snd_out=None, rx_index=None):
    """The four steps. Returns a dict: kinds (one of BUILT, IDLE, DEFER, BAD per socket), reasons, built (the
    built sockets behind the hand-off, in order), built_at (their indices), after (the table FS_TX_WRITEBACK
    leaves, as sock() dicts), totals (a dict of fs_tx_totals' fields)."""
    kinds, reasons, built, built_at, after = [], [], [], [], []
    F = B = 0
    tot = dict(n_frames=0, frames_bytes=0, data_bytes=0, n_built=0, n_idle=0, n_deferred=0, n_invalid=0)
    for i, s in enumerate(socks):
        t, handed, reason = hand_off(s, i, rx_socks_out, rx_snd_out, rx_index)
        reason = reason or check(t, rings_bytes)
        reasons.append(reason)
        if reason:
            kinds.append(BAD)
            after.append(dict(s))
            tot["n_invalid"] += 1
            continue
        r = ref.rule(t)
        if r["S"] == 0:
            kinds.append(IDLE)
            after.append(dict(t))
            tot["n_idle"] += 1
            continue
        F += r["S"]
        B += sock_bytes(t, r, flags, align)
        if F <= frames_cap and B <= frames_bytes:
            kinds.append(BUILT)
            built.append(t)
            built_at.append(i)
            hdr = bytearray(t["hdr"])
            hdr[18:20] = r["ip_id"].to_bytes(2, "big")
            after.append(dict(t, hdr=bytes(hdr), snd_nxt=r["snd_nxt"], ring_rpos=r["ring_rpos"],
                              ring_buffered=r["ring_buffered"], flags=t["flags"] & ~(ref.TX_ACK | (r["sent"] & ref.TX_FIN))))
            tot["n_built"] += 1
            tot["n_frames"], tot["frames_bytes"] = F, B
            tot["data_bytes"] += r["data"]
        else:
            kinds.append(DEFER)
            after.append(dict(t))
            tot["n_deferred"] += 1
    return dict(kinds=kinds, reasons=reasons, built=built, built_at=built_at, after=after, totals=tot)


def socks_out_of(socks, p, built_outs):
    """The call's socks_out: `built_outs` (the host call's records for p["built"]) at the built sockets, the
    unchanged state and the outcome at the others."""
    from seqs_amd.framesum import TX_SOCK_OUT_DTYPE

    outs = np.zeros(len(socks), dtype=TX_SOCK_OUT_DTYPE)
    at = {i: k for k, i in enumerate(p["built_at"])}
    for i, s in enumerate(socks):
        if i in at:
            outs[i] = built_outs[at[i]]
            continue
        sent = {IDLE: 0, DEFER: DEFERRED, BAD: INVALID | p["reasons"][i] << 16}[p["kinds"][i]]
        outs[i] = (s["snd_nxt"], s["ring_rpos"], s["ring_buffered"], 0, 0, ref.NONE, int.from_bytes(s["hdr"][18:20], "big"), sent)
    return outs


def totals_of(p):
    from seqs_amd.framesum import TX_TOTALS_DTYPE

    t = np.zeros(1, dtype=TX_TOTALS_DTYPE)
    for k, v in p["totals"].items():
        t[k] = v
    return t[0]


def expected(socks, rings, mtu, flags, align, noise, frames_cap, frames_bytes=None, rings_bytes=None, sentinels=None, **rx):
    """(buffer, offsets, lengths, digests, status, socks_out, totals, plan) the call must give into a copy of
    `noise`. With `sentinels` (offsets, lengths, digests, status arrays of frames_cap entries, prefilled) the
    four arrays come back whole, untouched tail included; else only the written entries."""
    frames_bytes = noise.size if frames_bytes is None else frames_bytes
    p = plan(socks, rings.size if rings_bytes is None else rings_bytes, frames_cap, frames_bytes, flags, align, **rx)
    buf, off, ln, dig, st, outs = ref.expected(p["built"], rings, mtu, flags & FCS_APPEND, align, noise)
    assert off.size == p["totals"]["n_frames"] <= frames_cap
    arrays = [off, ln, dig, st]
    if sentinels is not None:
        arrays = []
        for want, whole in zip((off, ln, dig, st), sentinels):
            whole = whole.copy()
            whole[: want.size] = want
            arrays.append(whole)
    return (buf, *arrays, socks_out_of(socks, p, outs), totals_of(p), p)
