"""Two endpoints that know only each other's IPv4 address, the library on BOTH ends of the link, every call's
output becoming the next call's input:
  1. the client's ARP call without a batch builds the who-has frame of a flagged query (fs_arp_flows_batch, n == 0,
     FS_ARP_SEND_REQUEST);
  2. the server's ARP call takes it (beside a request for another address and an IPv4 frame) and builds the reply;
  3. the client's next ARP call, the query now waiting, takes the reply: the query comes back done with the
     server's MAC;
  4. that MAC fills the opener of tests/dial.py's handshake -- the SYN of a connect call without a batch, the
     server's accept call, the SYN-ACK at the client -- which completes: the client is Established.
Then a sweep: a scanner asks for 300 addresses, twice over, of which the server lists 5 with one reply each; the
first pass is answered, the second finds the slots used.

The driver is written once; `arp` makes the ARP calls and `be` the handshake's (tests/dial.py's back ends). The
model (here) is tests/arp_ref.py; tests/test_gpu_neighbours.py has the device's, which compares every call's whole
output with the model's for the same inputs."""
import numpy as np

import accept_cases as acases
import accept_ref as aref
import arp_ref as ref
import connect_ref as cref
import conversation as conv
import deliver_ref as dref
import flows_ref as fref
import recv_ref as rref
import udp_ref

SERVER_IP, SERVER_MAC = acases.LOCAL_IP, acases.MAC
SWEEP = 300
LISTED = (3, 77, 150, 255, 299)  # the swept addresses the server lists
M32 = 1 << 32


def prefill(slots, seed):
    rng = np.random.default_rng(1300 + seed)
    return (rng.integers(1, 256, slots * ref.STRIDE, dtype=np.uint8), rng.integers(1, 256, slots * 8, dtype=np.uint8).view(ref.DIGEST_DTYPE),
            rng.integers(1, 256, slots, dtype=np.uint8))


def model_arp(frames, hosts, queries, n_reply_slots, arp_flags, seed):
    """One ARP call by the header's rules, over a prefill that the seed decides."""
    pre = prefill(n_reply_slots + len(queries), seed)
    return ref.expected(frames, ref.verdicts(frames), hosts, queries, n_reply_slots, arp_flags, *pre)


def swept(k):
    return bytes([10, 0, 1 + (k >> 8), k & 255])


def run(be, arp=model_arp, seed=9100):
    """The exchange with the back ends `arp` and `be`. Returns a dict of what check_end reads; `log` lists every ARP
    call as (who, frames, hosts, queries, n_reply_slots, arp_flags, seed, the call's tuple)."""
    from seqs_amd import arp_host, arp_query, hosts_after, split_arp
    from seqs_amd.framesum import CN_SEND_SYN, FCS_APPEND

    rng = np.random.default_rng(seed)
    log = []

    def call(who, frames, hosts, queries, n_reply, flags, s):
        out = arp(frames, hosts, queries, n_reply, flags, s)
        log.append((who, frames, hosts, queries, n_reply, flags, s, out))
        return out

    hdr = acases.header(rng, 0x6000)  # the client's frames to the server: its own address and MAC are the source
    client_ip, client_mac = hdr[26:30], hdr[6:12]
    c_hosts = arp_host(client_ip, client_mac, free=1)
    s_hosts = arp_host(SERVER_IP, SERVER_MAC, free=2)
    # 1: the request leaves the client
    ask = arp_query(0, SERVER_IP, send=True)
    o1 = call("client", [], c_hosts, ask, 1, 0, seed)
    _, requests, _ = split_arp(c_hosts, ask, o1[0], o1[1], o1[2], 1)
    # 2: the server answers it
    link = [ref.who_has(client_mac, client_ip, "10.0.0.99"), requests[0], udp_ref.udp_frame(client_ip, SERVER_IP, 68, 67, b"not arp")]
    o2 = call("server", link, s_hosts, np.zeros(0, dtype=ref.QUERY_DTYPE), 2, 0, seed + 1)
    replies, _, _ = split_arp(s_hosts, np.zeros(0, dtype=ref.QUERY_DTYPE), o2[0], o2[1], o2[2], 2)
    # 3: the reply resolves the client's query
    waiting = arp_query(0, SERVER_IP)
    o3 = call("client", replies[0], hosts_after(c_hosts, o1[0]), waiting, 1, 0, seed + 2)
    _, _, resolved = split_arp(c_hosts, waiting, o3[0], o3[1], o3[2], 1)
    peer_mac = resolved[0][0]
    # 4: the handshake, the opener's remote MAC the one ARP returned
    openers = cref.openers_of((fref.flow_key(conv.mirrored(hdr)), CN_SEND_SYN, client_mac, peer_mac, int(rng.integers(0, M32)), 1000, 0x711))
    slots = aref.slots_of((int(rng.integers(0, M32)), 256, 0x311))
    listeners = aref.listeners_of((acases.local(80), SERVER_MAC, 0, 1))
    rx_rings = be.rings(rng.integers(0, 256, 256 + 3, dtype=np.uint8))
    c1 = be.connect([], openers, seed + 3)
    syn = bytes(c1["replies"][:54])
    e1 = be.accept([syn], dref.socks_of(), rref.snd_of(), rx_rings, listeners, slots, seed + 4)
    synack = bytes(e1["synacks"][:54])
    idle = openers.copy()
    idle["flags"] = 0
    c2 = be.connect([synack], idle, seed + 5)
    # the sweep: 300 addresses twice over against 5 listed ones, padded frames with their FCS coming back
    rows = [arp_host(swept(k), bytes([2, 0, 0, 9, k >> 8, k & 255]), slot0=i, free=1) for i, k in enumerate(LISTED)]
    sw_hosts = np.concatenate(rows)
    scanner_mac, scanner_ip = bytes([2, 0, 0, 0, 0, 0x55]), "10.0.0.55"
    sweep = [ref.who_has(scanner_mac, scanner_ip, swept(k % SWEEP), pad=b"\0" * 18) for k in range(2 * SWEEP)]
    o4 = call("server", sweep, sw_hosts, np.zeros(0, dtype=ref.QUERY_DTYPE), len(LISTED), ref.PAD | FCS_APPEND, seed + 6)
    return dict(log=log, hdr=hdr, requests=requests, replies=replies, resolved=resolved, openers=openers, slots=slots, c1=c1, e1=e1,
                c2=c2, syn=syn, synack=synack, sweep=o4, sw_hosts=sw_hosts, scanner=(scanner_mac, ref.ip4(scanner_ip)))


def check_end(r):
    from seqs_amd import split_arp
    from seqs_amd.framesum import FCS_APPEND

    hdr, log = r["hdr"], r["log"]
    client_ip, client_mac = hdr[26:30], hdr[6:12]
    assert [c[0] for c in log] == ["client", "server", "client", "server"]
    # 1: the who-has frame, and the query comes back sent with nothing else written
    assert r["requests"] == {0: ref.who_has(client_mac, client_ip, SERVER_IP)} and int(log[0][7][1]["state"][0]) == ref.Q_SENT
    assert int(log[0][7][0]["free"][0]) == 1 and int(log[0][7][4][1]) == ref.FS_ARP
    # 2: only the request for the server's address is answered, to the asker's MAC
    assert list(log[1][7][5]) == [ref.IGNORED, ref.ANSWERED, ref.NOT_ARP] and list(log[1][7][0][0]) == [1, 1, 1, 1]
    assert r["replies"] == [[ref.arp_frame(2, SERVER_MAC, SERVER_IP, client_mac, client_ip, dst=client_mac, src=SERVER_MAC)]]
    # 3: the query is done and carries the server's MAC, which nothing but ARP told the client
    assert r["resolved"] == {0: (bytes(SERVER_MAC), 0)} and list(log[2][7][5]) == [ref.RESOLVED]
    # 4: the handshake completes on that MAC
    assert bytes(r["openers"]["remote_mac"][0]) == bytes(SERVER_MAC) and r["syn"][:6] == bytes(SERVER_MAC) and r["syn"][6:12] == client_mac
    assert int(r["e1"]["accept_of"][0]) == 0 and r["synack"][:6] == client_mac and r["synack"][6:12] == bytes(SERVER_MAC)
    out = r["c2"]["openers_out"]
    iss, s_iss = int(r["openers"]["iss"][0]), int(r["slots"]["iss"][0])
    assert int(out["state"][0]) == 4 and int(out["reply"][0]) == cref.REPLY_ACK  # Established, and the third ACK is owed
    assert (int(out["rcv_nxt"][0]), int(out["snd_nxt"][0])) == ((s_iss + 1) % M32, (iss + 1) % M32)
    ack = bytes(r["c2"]["replies"][:54])
    assert ack[:6] == bytes(SERVER_MAC) and int.from_bytes(ack[42:46], "big") == (s_iss + 1) % M32
    # the sweep: each listed address answered once, in the order the sweep reached it; the second pass finds no slot
    o = r["sweep"]
    code = np.asarray(o[5])
    assert (code == ref.ANSWERED).sum() == len(LISTED) == (code == ref.FULL).sum() and (code == ref.IGNORED).sum() == 2 * (SWEEP - len(LISTED))
    assert list(np.flatnonzero(code == ref.ANSWERED)) == list(LISTED) and list(np.flatnonzero(code == ref.FULL)) == [SWEEP + k for k in LISTED]
    assert list(o[0]["n_requests"]) == [2] * len(LISTED) and list(o[0]["first"]) == list(LISTED) and not o[0]["free"].any()
    replies, _, _ = split_arp(r["sw_hosts"], np.zeros(0, dtype=ref.QUERY_DTYPE), o[0], o[1], o[2], len(LISTED), ref.PAD | FCS_APPEND)
    mac, ip = r["scanner"]
    for (k, h), (fr,) in zip(zip(LISTED, r["sw_hosts"]), replies):
        assert len(fr) == 64 and fr[:42] == ref.arp_frame(2, bytes(h["mac"]), swept(k), mac, ip, dst=mac, src=bytes(h["mac"]))
        assert not any(fr[42:60]) and ref.verdicts([fr], fcs=True)[0] == ref.FS_ARP
