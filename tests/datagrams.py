"""Two endpoints that exchange UDP datagrams for several rounds, each call's output the next call's input: the
INTEGRATION.md "Datagrams" loop. A client asks a server's two ports (a 4-cell queue on port 67, which fills, and
a roomy one on port 53); a link interleaves its frames with frames that are nobody's; the server's call puts
them into its queues; the server reads the cells (seqs_amd.split_dgrams), answers each cell's source from the
cell's header alone, and hands cells back (seqs_amd.ports_after) -- at first fewer than it got, so that the
queue stays full, then all, so that it drains; the client's call takes the answers into its own queues.

How frames are built and how a call is made are the caller's: tests/test_datagrams_model.py passes
tests/udp_ref.py for both, tests/test_gpu_datagrams.py the library (fs_segment_batch's UDP build and
fs_udp_flows_batch). run() returns every call's whole output in order."""
import numpy as np

import udp_ref as ref

CLIENT_IP, SERVER_IP = "10.0.0.2", "10.0.0.1"
CLIENT_MAC, SERVER_MAC = b"\x02\x00\x00\x00\x00\x0c", b"\x02\x00\x00\x00\x00\x05"
ROUNDS = 6


def template(src_mac, dst_mac, src_ip, dst_ip, sport, dport) -> bytes:
    """The 42-byte header template of a UDP send (include/framesum.h): lengths and checksums are the build's."""
    return (bytes(dst_mac) + bytes(src_mac) + b"\x08\x00" + bytes([0x45, 0, 0, 0, 0, 0, 0x40, 0, 64, 17, 0, 0]) + ref.ip4(src_ip) +
            ref.ip4(dst_ip) + int(sport).to_bytes(2, "big") + int(dport).to_bytes(2, "big") + b"\0\0\0\0")


def model_build(headers, payloads):
    """The frames of the sends, by tests/udp_ref.py's frame builder."""
    return [ref.udp_frame(h[26:30], h[30:34], int.from_bytes(h[34:36], "big"), int.from_bytes(h[36:38], "big"), p,
                          src_mac=h[6:12], dst_mac=h[0:6]) for h, p in zip(headers, payloads)]


def model_call(frames, ports, cells):
    """One call by tests/udp_ref.py: (ports_out, port_of, cell_of, cells)."""
    return ref.expected(frames, ref.verdicts(frames), ports, cells)


def link(frames, rnd):
    """What the wire adds: a TCP frame to the same port behind every third frame, a datagram to a port nobody
    has behind every fourth, and the second half of the frames in front of the first in odd rounds."""
    out = []
    for k, f in enumerate(frames):
        out.append(f)
        if k % 3 == 2:
            out.append(ref.udp_frame("192.168.7.7", f[30:34], 999, int.from_bytes(f[36:38], "big"), b"tcp", proto=6))
        if k % 4 == 3:
            out.append(ref.udp_frame("192.168.7.7", f[30:34], 999, 4444, b"nobody's"))
    half = len(out) // 2
    return out[half:] + out[:half] if rnd % 2 else out


def run(build=model_build, call=model_call, rounds=ROUNDS):
    """Drives the exchange; returns the log: per call (who, frames, ports, (ports_out, port_of, cell_of, cells))."""
    from seqs_amd import ports_after, split_dgrams

    server_ports, server_bytes = ref.lay_out([ref.port_row(SERVER_IP, 67, 4, 48), ref.port_row("0.0.0.0", 53, 16, 96)], lead=8, gap=16)
    client_ports, client_bytes = ref.lay_out([ref.port_row(CLIENT_IP, 68, 8, 64, wcell=6), ref.port_row(CLIENT_IP, 5353, 16, 72)])
    server_cells = np.full(server_bytes, 0xEE, dtype=np.uint8)
    client_cells = np.full(client_bytes, 0xDD, dtype=np.uint8)
    service = {67: 68, 53: 5353}  # the server's port -> the client's port that asks it
    log, got_back = [], []
    for rnd in range(rounds):
        # the client asks: six questions to port 67 (more than its queue holds), three to port 53 (one to the
        # broadcast address, which the server's wildcard port takes), the first answer it got echoed in one
        headers, payloads = [], []
        for k in range(6):
            headers.append(template(CLIENT_MAC, SERVER_MAC, CLIENT_IP, SERVER_IP, 68, 67))
            payloads.append(bytes([rnd, k]) + b"q" * (3 * k))  # 2 .. 17 bytes: the last one is cut by the 16-byte room
        for k in range(3):
            dst = "255.255.255.255" if k == 2 else SERVER_IP
            headers.append(template(CLIENT_MAC, SERVER_MAC if k != 2 else b"\xff" * 6, CLIENT_IP, dst, 5353, 53))
            payloads.append(bytes([rnd, 100 + k]) + (got_back[0][1][:20] if got_back else b"first"))
        frames = link(build(headers, payloads), rnd)
        out = call(frames, server_ports, server_cells)
        log.append(("server", frames, server_ports.copy(), out))
        server_cells = out[3]
        queues = split_dgrams(server_cells, server_ports, out[0])
        # the server's handlers: in the first three rounds port 67's reads two cells only; then whatever is there
        consumed, headers, payloads = [], [], []
        for p, q in enumerate(queues):
            take = min(len(q), 2) if (p == 0 and rnd < 3) else len(q)
            consumed.append(take)
            for h, data in q[:take]:
                sport = int.from_bytes(bytes(server_ports[p]["local"][4:6]), "big")
                assert service[sport] == int(h["src_port"])
                headers.append(template(h["dst_mac"].tobytes() if h["dst_mac"][0] != 0xFF else SERVER_MAC, h["src_mac"].tobytes(),
                                        SERVER_IP, h["src_ip"].tobytes(), sport, int(h["src_port"])))
                payloads.append(int(h["len"]).to_bytes(2, "big") + data[::-1])
        # (cells the handler has not read stay in the queue: they are handed back in a later round)
        backlog = out[0]["n_admitted"].astype(np.int64) - np.array(consumed)
        server_ports = ports_after(server_ports, out[0], consumed=consumed)
        if rnd >= 3:  # the backlog of the first rounds drains: the queue's oldest cells are free again
            held = server_ports["n_cells"].astype(np.int64) - server_ports["free"]
            server_ports["free"] += held.astype(np.uint32)
        frames = link(build(headers, payloads), rnd + 1) if headers else []
        out = call(frames, client_ports, client_cells)
        log.append(("client", frames, client_ports.copy(), out))
        client_cells = out[3]
        queues = split_dgrams(client_cells, client_ports, out[0])
        got_back = [d for q in queues for d in q] or got_back
        client_ports = ports_after(client_ports, out[0])
        assert (backlog >= 0).all()
    return log
