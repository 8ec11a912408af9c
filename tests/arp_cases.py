"""The batches of tests/test_gpu_arp.py. Every builder returns a Case: the frames, the host and query lists, the
call's flags, and `reaches(want)`, which asserts on tests/arp_ref.py's expected tuple (hosts_out, queries_out,
arp_frames, arp_out, arp_status, arp_code, arp_of) that the batch reaches what its name says.
tests/test_arp_case_builders.py runs every `reaches` on the CPU."""
import functools

import numpy as np

import arp_ref as ref
import udp_ref

US, US_MAC = "10.0.0.1", "02:00:00:00:00:01"
PEER, PEER_MAC = "10.0.0.2", "02:00:00:00:00:02"
RANKS = (0, 1, 62, 63, 64, 65, 255, 256, 257)
NO_QUERIES = np.zeros(0, dtype=ref.QUERY_DTYPE)
NO_HOSTS = np.zeros(0, dtype=ref.HOST_DTYPE)


class Case:
    def __init__(self, frames, hosts, queries, n_reply_slots, reaches, arp_flags=0, flags=0, mtu=0, lists=None, ports=None,
                 batch=None, status=None):
        self.frames, self.hosts, self.queries, self.n_reply_slots, self.reaches = frames, hosts, queries, n_reply_slots, reaches
        self.arp_flags, self.flags, self.mtu = arp_flags, flags, mtu
        self.lists = lists    # a tests/connect_cases.py case whose lists the call takes beside the hosts
        self.ports = ports    # (ports, cells_bytes) of tests/udp_ref.py where the call has UDP ports too
        self.batch = batch    # (buf, off, ln) where the frames lie in a buffer of the builder's own
        self.status = status  # the frames' verdicts where the builder knows them


def expected(case):
    """The reference's tuple for the case over zeroed arrays, with pyref's verdicts unless the case has its own."""
    status = ref.verdicts(case.frames, case.mtu, bool(case.flags & 1)) if case.status is None else case.status
    return ref.expected(case.frames, status, case.hosts, case.queries, case.n_reply_slots, case.arp_flags, mtu=case.mtu,
                        fcs=bool(case.flags & 1))


def source(k):
    return f"172.{16 + (k >> 16) % 16}.{(k >> 8) & 255}.{k & 255}"


def source_mac(k):
    return bytes([2, 1, (k >> 24) & 255, (k >> 16) & 255, (k >> 8) & 255, k & 255])


def noise(r, ip=US):
    """A frame that takes no rank: a request for another address, an unsupported one, an IPv4 datagram, a short ARP
    frame of 34 .. 41 bytes, in turn."""
    return (ref.who_has(source_mac(r), source(r), "10.9.9.9"), ref.who_has(source_mac(r), source(r), ip, hlen=5),
            udp_ref.udp_frame(source(r), ip, 1024 + r, 67, b"ipv4"), ref.who_has(source_mac(r), source(r), ip)[: 34 + (r // 4) % 8])[r % 4]


@functools.lru_cache(maxsize=None)
def noisy(n_matched=258, ip=US):
    """`n_matched` requests for `ip` from changing senders (every third unicast to US_MAC, every seventh padded to 60
    bytes), with a frame that takes no rank after each."""
    frames = []
    for r in range(n_matched):
        f = ref.who_has(source_mac(r), source(r), ip, dst=US_MAC if r % 3 == 1 else ref.BROADCAST, pad=b"\0" * 18 if r % 7 == 0 else b"")
        frames += [f, noise(r, ip)]
    return tuple(frames)


# ---- requests ---------------------------------------------------------------------------------------------------

def rank(free):
    """Ranks 0 .. 257 of one host (RANKS among them) with frames that take no rank between; `free` reply slots."""
    hosts, n_reply = ref.hosts_of([ref.host_row("10.0.0.7", "02:00:00:00:00:07", free=3), ref.host_row(US, US_MAC, free=free)])

    def reaches(want):
        assert want[0]["n_requests"][1] == 258 and want[0]["n_answered"][1] == min(free, 258) and want[0]["n_requests"][0] == 0
        assert list(want[6][::2][list(RANKS)]) == [3 + r if r < free else ref.NONE for r in RANKS]
        assert list(want[5][::2][list(RANKS)]) == [ref.ANSWERED if r < free else ref.FULL for r in RANKS]
        assert set(want[5][1::2]) == {ref.NOT_ARP, ref.UNSUPPORTED, ref.IGNORED} and (want[6][1::2] == ref.NONE).all()
        assert want[0]["first"][1] == 0 and want[0]["free"][1] == max(0, free - 258) and want[0]["first"][0] == ref.NONE
        assert not want[2][: 3 * 64].any()  # the other host's slots take no frame
    return Case(list(noisy()), hosts, NO_QUERIES, n_reply, reaches)


def three_hosts():
    """Three hosts whose requests interleave; one of them hears only broadcasts for it (its MAC differs)."""
    rows = [ref.host_row(US, US_MAC, free=40), ref.host_row("10.0.0.3", "02:00:00:00:00:03", free=70), ref.host_row("0.0.0.0", US_MAC, free=64)]
    hosts, n_reply = ref.hosts_of(rows)
    which = np.random.default_rng(2).integers(0, 4, 200)
    frames = []
    for k in range(200):
        tpa, dst = ((US, ref.BROADCAST), ("10.0.0.3", US_MAC), ("0.0.0.0", US_MAC), ("10.0.0.3", ref.BROADCAST))[which[k]]
        frames.append(ref.who_has(source_mac(k), source(k), tpa, dst=dst))

    def reaches(want):
        n = [int((which == w).sum()) for w in range(4)]
        assert list(want[0]["n_requests"]) == [n[0], n[3], n[2]] and list(want[0]["n_answered"]) == [40, min(70, n[3]), min(64, n[2])]
        assert (want[5][which == 1] == ref.IGNORED).all()  # 10.0.0.3 does not hear US_MAC
        assert (want[5] == ref.FULL).sum() == n[0] - 40 and np.count_nonzero(np.diff(want[5].astype(np.int64))) > 60
    return Case(frames, hosts, NO_QUERIES, n_reply, reaches)


def shared_mac():
    """Two hosts sharing a MAC: a unicast request reaches the host whose address it names."""
    hosts, n_reply = ref.hosts_of([ref.host_row(US, US_MAC, free=4), ref.host_row("10.0.0.3", US_MAC, free=4)])
    frames = [ref.who_has(source_mac(k), source(k), (US, "10.0.0.3")[k % 2], dst=US_MAC) for k in range(6)]

    def reaches(want):
        assert list(want[6]) == [0, 4, 1, 5, 2, 6] and list(want[0]["n_answered"]) == [3, 3]
        assert bytes(want[2][4 * 64 + 28 : 4 * 64 + 32]) == ref.ip4("10.0.0.3") and bytes(want[2][6:12]) == ref.mac6(US_MAC)
    return Case(frames, hosts, NO_QUERIES, n_reply, reaches)


# ---- replies ----------------------------------------------------------------------------------------------------

def replies(pos):
    """The reply that resolves query 0 at batch position `pos`, behind noise; a later duplicate of it; query 1
    resolved and its duplicate gone stale before that (where there is room); a reply nobody asked for."""
    hosts, n_reply = ref.hosts_of([ref.host_row(US, US_MAC, free=1)])
    queries = ref.queries_of([ref.query_row(0, PEER), ref.query_row(0, "10.0.0.5"), ref.query_row(0, "10.0.0.6")])
    frames = [noise(r) for r in range(pos)]
    if pos >= 3:
        frames[0] = ref.is_at("02:00:00:00:00:05", "10.0.0.5", US_MAC, US)
        frames[1] = ref.is_at("02:00:00:00:00:55", "10.0.0.5", US_MAC, US)  # another sender for the same address: stale
        frames[2] = ref.is_at("02:00:00:00:00:66", "10.0.0.66", US_MAC, US)
    frames += [ref.is_at(PEER_MAC, PEER, US_MAC, US), noise(0), ref.is_at("02:ff:ff:ff:ff:ff", PEER, US_MAC, US, dst=ref.BROADCAST)]

    def reaches(want):
        q = want[1]
        assert (int(q[0]["state"]), int(q[0]["frame"]), int(q[0]["n_replies"]), bytes(q[0]["mac"])) == (ref.Q_DONE, pos, 2, ref.mac6(PEER_MAC))
        assert list(want[5][pos:]) == [ref.RESOLVED, ref.IGNORED, ref.STALE] and list(want[6][pos:]) == [0, ref.NONE, 0]
        assert int(q[2]["state"]) == ref.Q_WAIT and int(q[2]["frame"]) == ref.NONE and not q[2]["mac"].any()
        if pos >= 3:
            assert list(want[5][:3]) == [ref.RESOLVED, ref.STALE, ref.IGNORED] and int(q[1]["frame"]) == 0 and int(q[1]["n_replies"]) == 2
            assert bytes(q[1]["mac"]) == ref.mac6("02:00:00:00:00:05")
    return Case(frames, hosts, queries, n_reply, reaches)


def flagged_and_near():
    """A flagged query beside its own reply, which must stay unanswered; a reply whose ProtoSender is one bit off; a
    reply to an address that has a query on another host only."""
    hosts, n_reply = ref.hosts_of([ref.host_row(US, US_MAC, free=1), ref.host_row("10.0.0.3", "02:00:00:00:00:03", free=1)])
    queries = ref.queries_of([ref.query_row(0, PEER, send=True), ref.query_row(0, "10.0.0.6"), ref.query_row(1, "10.0.0.8")])
    frames = [ref.is_at(PEER_MAC, PEER, US_MAC, US), ref.is_at("02:00:00:00:00:06", "10.0.0.7", US_MAC, US),
              ref.is_at("02:00:00:00:00:08", "10.0.0.8", US_MAC, US), ref.is_at("02:00:00:00:00:06", "10.0.0.6", US_MAC, US)]

    def reaches(want):
        assert list(want[5]) == [ref.IGNORED, ref.IGNORED, ref.IGNORED, ref.RESOLVED] and list(want[1]["state"]) == [ref.Q_SENT, ref.Q_DONE, ref.Q_WAIT]
        assert bytes(want[2][2 * 64 : 2 * 64 + 42]) == ref.who_has(US_MAC, US, PEER) and want[4][2] == ref.FS_ARP
        assert not want[2][: 2 * 64].any() and not want[2][3 * 64 :].any() and want[1]["n_replies"][0] == 0
    return Case(frames, hosts, queries, n_reply, reaches)


# ---- frames -----------------------------------------------------------------------------------------------------

def lengths(arp_flags):
    """Requests and replies of 42, 60 and 1,500 bytes (the test packs them at every start alignment 0 .. 63)."""
    hosts, n_reply = ref.hosts_of([ref.host_row(US, US_MAC, free=3)])
    queries = ref.queries_of([ref.query_row(0, f"10.0.1.{k}") for k in range(3)] + [ref.query_row(0, "10.0.1.99", send=True)])
    frames = []
    for k, size in enumerate((42, 60, 1500)):
        pad = bytes((7 * j + k) & 255 or 1 for j in range(size - 42))
        frames += [ref.who_has(source_mac(k), source(k), US, pad=pad), ref.is_at(source_mac(9 + k), f"10.0.1.{k}", US_MAC, US, pad=pad)]

    def reaches(want):
        assert list(want[5]) == [ref.ANSWERED, ref.RESOLVED] * 3 and list(want[6]) == [0, 0, 1, 1, 2, 2] and list(want[1]["frame"][:3]) == [1, 3, 5]
        size = (60 if arp_flags & ref.PAD else 42) + (4 if arp_flags & ref.FCS_APPEND else 0)
        for slot in (0, 1, 2, 6):
            assert want[2][slot * 64 : slot * 64 + 42].any() and not want[2][slot * 64 + size : slot * 64 + 64].any()
            assert want[4][slot] == ref.FS_ARP and want[3][slot]["crc32"] != 0 and want[3][slot]["l4_csum"] == 0
    return Case(frames, hosts, queries, n_reply, reaches, arp_flags=arp_flags)


def with_fcs():
    """noisy() with the frames' FCS on them (FS_RX_FCS), one request's FCS damaged; the built frames padded with FCS."""
    import zlib

    wire = [f + zlib.crc32(f).to_bytes(4, "little") for f in noisy()[:40]]
    wire[4] = wire[4][:-2] + bytes([wire[4][-2] ^ 0x10]) + wire[4][-1:]
    hosts, n_reply = ref.hosts_of([ref.host_row(US, US_MAC, free=30)])

    def reaches(want):
        assert want[5][4] == ref.NOT_ARP and want[0]["n_requests"][0] == 19 and list(want[6][:8:2]) == [0, 1, ref.NONE, 2]
    return Case(wire, hosts, NO_QUERIES, n_reply, reaches, arp_flags=3, flags=1)


def near_keys():
    """Requests whose ProtoTarget or destination MAC, and replies whose ProtoTarget or ProtoSender, differ from the
    listed ones in one bit."""
    hosts, n_reply = ref.hosts_of([ref.host_row(US, US_MAC, free=200)])
    queries = ref.queries_of([ref.query_row(0, PEER)])

    def flip(b, bit):
        b = bytearray(b)
        b[bit // 8] ^= 1 << (bit % 8)
        return bytes(b)

    us, peer, mac = ref.ip4(US), ref.ip4(PEER), ref.mac6(US_MAC)
    frames = [ref.who_has(PEER_MAC, PEER, US, dst=US_MAC)]
    frames += [ref.who_has(PEER_MAC, PEER, flip(us, bit), dst=US_MAC) for bit in range(32)]
    frames += [ref.who_has(PEER_MAC, PEER, US, dst=flip(mac, bit)) for bit in range(48)]
    frames += [ref.is_at(PEER_MAC, flip(peer, bit), US_MAC, US) for bit in range(32)]
    frames += [ref.is_at(PEER_MAC, PEER, US_MAC, flip(us, bit)) for bit in range(32)]
    frames += [ref.is_at(PEER_MAC, PEER, US_MAC, US), ref.who_has(PEER_MAC, PEER, US)]

    def reaches(want):
        assert len(frames) == 147 and list(want[5][[0, 145, 146]]) == [ref.ANSWERED, ref.RESOLVED, ref.ANSWERED]
        assert (want[5][1:145] == ref.IGNORED).all() and want[0]["n_requests"][0] == 2 and want[1]["n_replies"][0] == 1
    return Case(frames, hosts, queries, n_reply, reaches)


# ---- launch shapes ------------------------------------------------------------------------------------------------

def many_hosts(n_hosts, free=1):
    hosts = np.zeros(n_hosts, dtype=ref.HOST_DTYPE)
    idx = np.arange(n_hosts, dtype=np.uint32)
    hosts["ip"] = np.stack([np.full(n_hosts, 10, np.uint8), (idx >> 16).astype(np.uint8) + 1, (idx >> 8).astype(np.uint8), idx.astype(np.uint8)], axis=1)
    hosts["mac"] = np.stack([np.full(n_hosts, 2, np.uint8), np.zeros(n_hosts, np.uint8), np.zeros(n_hosts, np.uint8),
                             (idx >> 16).astype(np.uint8), (idx >> 8).astype(np.uint8), idx.astype(np.uint8)], axis=1)
    hosts["slot0"], hosts["free"] = idx * free, free
    return hosts, n_hosts * free


@functools.lru_cache(maxsize=None)
def table_load():
    """300 hosts with a query each and 700 frames: frame k is a request for host 37 k mod 300, every fifth a reply to
    that host's query, every seventh for an address one above the host's (the next host's, or nobody's)."""
    hosts, n_reply = many_hosts(300, 2)
    queries = ref.queries_of([ref.query_row(h, source(h)) for h in range(300)])
    frames = []
    for k in range(700):
        h = (k * 37) % 300
        ip = bytes(hosts[h]["ip"])
        if k % 7 == 6:
            ip = (int.from_bytes(ip, "big") + 41).to_bytes(4, "big")
        frames.append(ref.is_at(source_mac(k), source(h), bytes(hosts[h]["mac"]), ip, dst=ref.BROADCAST) if k % 5 == 4 else
                      ref.who_has(source_mac(k), source(k), ip))

    def reaches(want):
        assert (want[0]["n_requests"] > 0).sum() > 200 and (want[5] == ref.FULL).any() and (want[5] == ref.STALE).any()
        assert (want[1]["state"] == ref.Q_DONE).sum() > 50 and (want[5] == ref.IGNORED).any()
    return Case(frames, hosts, queries, n_reply, reaches)


def two_hosts():
    """noisy() to two hosts (the second one's requests come first), 200 and 65 free slots."""
    hosts, n_reply = ref.hosts_of([ref.host_row(US, US_MAC, free=200), ref.host_row("10.0.0.3", US_MAC, free=65)])
    frames = list(noisy(65, "10.0.0.3")) + list(noisy())

    def reaches(want):
        assert list(want[0]["n_requests"]) == [258, 65] and list(want[0]["n_answered"]) == [200, 65] and list(want[0]["first"]) == [130, 0]
    return Case(frames, hosts, NO_QUERIES, n_reply, reaches)


def columns():
    """300 frames of noisy() and the replies of replies(64), for every engine column."""
    other = replies(64)

    def reaches(want):
        assert want[0]["n_requests"][0] == 150 and want[0]["n_answered"][0] == 1 and want[1]["frame"][0] == 300 + 64
    return Case(list(noisy()[:300]) + other.frames, other.hosts, other.queries, other.n_reply_slots, reaches, arp_flags=ref.PAD)


# ---- mixed and large batches --------------------------------------------------------------------------------------

def mixed():
    """tests/connect_cases.py's three_lists() (sockets, a listener, closers, openers) and two UDP ports with 40 ARP
    frames and 20 datagrams between its frames."""
    import connect_cases

    case = connect_cases.three_lists()
    frames = list(case.frames)
    for k in range(60):
        f = (ref.who_has(source_mac(k), source(k), US), ref.is_at(source_mac(k), f"10.0.2.{(k // 3) % 6}", US_MAC, US),
             udp_ref.udp_frame(source(k), US, 5000 + k, 67, b"between the flows %d" % k))[k % 3]
        frames.insert(min(len(frames), 3 * k + 1), f)
    hosts, n_reply = ref.hosts_of([ref.host_row(US, US_MAC, free=16)])
    queries = ref.queries_of([ref.query_row(0, f"10.0.2.{k}", send=k == 5) for k in range(6)])
    ports = udp_ref.lay_out([udp_ref.port_row(US, 67, 16, 64)], lead=8)

    def reaches(want):
        assert want[0]["n_requests"][0] == 20 and want[0]["n_answered"][0] == 16 and list(want[1]["state"]) == [ref.Q_DONE] * 5 + [ref.Q_SENT]
        assert len(case.socks) and len(case.listeners) and len(case.closers) and len(case.openers)
        assert (want[5] == ref.NOT_ARP).sum() == len(case.frames) + 20 and (want[5] == ref.STALE).sum() > 0
    return Case(frames, hosts, queries, n_reply, reaches, lists=case, ports=ports)


def big(n_hosts):
    """65,793 60-byte requests (more than 2^16 and no multiple of a workgroup's 256): to one host with room for all
    but 793; to 1,000 hosts of 2 slots for 65 or 66 requests each; to 65,536 hosts of one slot, 257 of which get two."""
    n = 65793
    if n_hosts == 1:
        hosts, n_reply = ref.hosts_of([ref.host_row(US, US_MAC, free=65000)])
    else:
        hosts, n_reply = many_hosts(n_hosts, 2 if n_hosts == 1000 else 1)
    which = (np.arange(n) * 7919) % n_hosts
    idx = np.arange(n, dtype=np.uint32)
    arr = np.zeros((n, 60), dtype=np.uint8)
    arr[:, 0:6] = 255
    arr[:, 6:12] = arr[:, 22:28] = np.stack([np.full(n, 2, np.uint8), np.full(n, 1, np.uint8), (idx >> 24).astype(np.uint8), (idx >> 16).astype(np.uint8),
                                             (idx >> 8).astype(np.uint8), idx.astype(np.uint8)], axis=1)
    arr[:, 12:22] = np.frombuffer(bytes([8, 6, 0, 1, 8, 0, 6, 4, 0, 1]), dtype=np.uint8)
    arr[:, 28:32] = np.stack([np.full(n, 172, np.uint8), (idx >> 16).astype(np.uint8) + 16, (idx >> 8).astype(np.uint8), idx.astype(np.uint8)], axis=1)
    arr[:, 38:42] = hosts["ip"][which]
    buf = np.concatenate([arr.reshape(-1), np.zeros(64, np.uint8)])
    off, ln = np.arange(n, dtype=np.uint64) * 60, np.full(n, 60, dtype=np.uint32)
    frames = [buf[60 * i : 60 * i + 60].tobytes() for i in range(n)]

    def reaches(want):
        m = want[0]["n_requests"]
        if n_hosts == 1:
            assert m[0] == n and want[0]["n_answered"][0] == 65000 and (want[5] == ref.FULL).sum() == 793
        elif n_hosts == 1000:
            assert set(m) == {65, 66} and (want[0]["n_answered"] == 2).all()
        else:
            assert m.sum() == n and (m == 2).sum() == 257 and (want[5] == ref.FULL).sum() == 257
    return Case(frames, hosts, NO_QUERIES, n_reply, reaches, batch=(buf, off, ln), status=np.full(n, ref.FS_ARP, dtype=np.uint8))


# ---- calls --------------------------------------------------------------------------------------------------------

def empty_batch():
    """n == 0: every host keeps its slots, a flagged query's request is still built."""
    hosts, n_reply = ref.hosts_of([ref.host_row(US, US_MAC, free=2), ref.host_row("10.0.0.3", US_MAC, free=0)])
    queries = ref.queries_of([ref.query_row(1, PEER), ref.query_row(0, PEER, send=True)])

    def reaches(want):
        assert list(want[0]["free"]) == [2, 0] and (want[0]["first"] == ref.NONE).all() and not want[0]["n_requests"].any()
        assert list(want[1]["state"]) == [ref.Q_WAIT, ref.Q_SENT] and bytes(want[2][3 * 64 : 3 * 64 + 42]) == ref.who_has(US_MAC, US, PEER)
        assert not want[2][: 3 * 64].any() and want[5].size == 0
    return Case([], hosts, queries, n_reply, reaches, arp_flags=ref.FCS_APPEND)


def no_hosts(n=40):
    """n_hosts == 0: the codes alone."""
    def reaches(want):
        assert want[0].size == 0 and want[2].size == 0 and (want[6] == ref.NONE).all() and want[6].size == n
        assert set(want[5]) == {ref.NOT_ARP, ref.UNSUPPORTED, ref.IGNORED}
    return Case(list(noisy()[:n]), NO_HOSTS, NO_QUERIES, 0, reaches)


def in_flight(k):
    """The k-th of eight calls in flight: 120 frames of noisy() from 2 k on and a reply, slots of its own number."""
    hosts, n_reply = ref.hosts_of([ref.host_row(US, US_MAC, free=50 + k)])
    queries = ref.queries_of([ref.query_row(0, f"10.0.3.{k}")])
    frames = list(noisy()[2 * k : 2 * k + 120]) + [ref.is_at(source_mac(k), f"10.0.3.{k}", US_MAC, US)]

    def reaches(want):
        assert want[0]["n_requests"][0] == 60 and want[0]["n_answered"][0] == min(60, 50 + k) and want[1]["frame"][0] == 120
    return Case(frames, hosts, queries, n_reply, reaches, arp_flags=k % 4)


def host_form():
    """The host form's batch: requests, replies and a flagged query."""
    hosts, n_reply = ref.hosts_of([ref.host_row(US, US_MAC, free=40), ref.host_row("10.0.0.3", US_MAC, free=0)])
    queries = ref.queries_of([ref.query_row(0, PEER), ref.query_row(1, PEER, send=True)])
    frames = list(noisy()[:200]) + [ref.is_at(PEER_MAC, PEER, US_MAC, US), ref.who_has(PEER_MAC, PEER, "10.0.0.3")]

    def reaches(want):
        assert list(want[0]["n_requests"]) == [100, 1] and list(want[0]["n_answered"]) == [40, 0] and want[5][201] == ref.FULL
        assert list(want[1]["state"]) == [ref.Q_DONE, ref.Q_SENT] and want[1]["frame"][0] == 200
    return Case(frames, hosts, queries, n_reply, reaches, arp_flags=ref.PAD | ref.FCS_APPEND)


def rejected_lists():
    """Three good hosts of two slots and three good queries: (hosts, queries, n_reply_slots)."""
    hosts, n_reply = ref.hosts_of([ref.host_row(f"10.0.0.{k + 1}", US_MAC, free=2) for k in range(3)])
    return hosts, ref.queries_of([ref.query_row(0, PEER), ref.query_row(0, "10.0.0.5"), ref.query_row(2, PEER)]), n_reply


# (change(hosts, queries), the text); the call's own numbers and flags are in the test
REJECTIONS = [
    (lambda h, q: h["reserved"].__setitem__(1, 1), "host or query 1: a host's reserved must be 0"),
    (lambda h, q: h["ip"].__setitem__(2, h["ip"][0]), "host or query 2: its ip equals an earlier host's"),
    (lambda h, q: h["free"].__setitem__(2, 3), "host or query 2: its slot range ends past n_reply_slots"),
    (lambda h, q: h["slot0"].__setitem__(2, 7), "host or query 2: its slot range ends past n_reply_slots"),
    (lambda h, q: h["slot0"].__setitem__(1, 1), "host or query 1: its slot range overlaps another host's"),
    (lambda h, q: q["host"].__setitem__(1, 3), "host or query 1: its host is not below n_hosts"),
    (lambda h, q: q["target"].__setitem__(1, q["target"][0]), "host or query 1: its host and target equal an earlier query's"),
    (lambda h, q: q["flags"].__setitem__(0, 2), "host or query 0: its flags must be 0 or FS_ARP_SEND_REQUEST"),
    (lambda h, q: q["reserved"].__setitem__(2, 1), "host or query 2: a query's reserved must be 0"),
]
