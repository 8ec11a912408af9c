"""tests/neighbours.py's exchange against the models alone (no GPU): two endpoints start from IP addresses, ARP
gives the client the server's MAC, and tests/dial.py's handshake completes on it; every ARP call's output by the
header's rules is also what the transliteration of RecvEth's ARP branch and arpClient gives; the sweep of 300
addresses is answered for the 5 listed ones, once each."""
import dial
import neighbours as nb

import arp_ref as ref


def test_the_exchange_against_the_models():
    r = nb.run(dial.Model())
    nb.check_end(r)
    assert len(r["log"]) == 4
    for who, frames, hosts, queries, n_reply, flags, seed, out in r["log"]:
        pre = nb.prefill(n_reply + len(queries), seed)
        other = ref.recv_eth_model(frames, hosts, queries, n_reply, flags, *pre)  # the second statement, on the same input
        assert ref.same(out, other) == [], (who, ref.same(out, other))
    # what the reference would do with the sweep: one pendingResponse per PortStack, which is `free` = 1
    who, frames, hosts, queries, n_reply, flags, seed, out = r["log"][3]
    faithful, clients = ref.recv_eth_model(frames, hosts, queries, n_reply, flags, *nb.prefill(n_reply, seed), faithful=True)
    assert ref.same(out, faithful) == [] and all(len(c.seen) == 2 for c in clients)


def test_nothing_but_arp_tells_the_client_the_mac():
    """The driver reads the MAC from the query's out record: a reply from another MAC gives another opener."""
    def lying(frames, hosts, queries, n_reply, flags, seed):
        frames = [f[:6] + bytes([2, 0xBA, 0xD0, 0, 0, 1]) + f[12:22] + bytes([2, 0xBA, 0xD0, 0, 0, 1]) + f[28:] if f[21] == 2 else f for f in frames]
        return nb.model_arp(frames, hosts, queries, n_reply, flags, seed)

    r = nb.run(dial.Model(), lying)
    assert bytes(r["openers"]["remote_mac"][0]) == bytes([2, 0xBA, 0xD0, 0, 0, 1]) == r["syn"][:6]
