"""Every batch of tests/arp_cases.py reaches what it names, shown with tests/arp_ref.py alone (no GPU, no
library): each case's `reaches` runs on the reference's expected tuple, and the transliteration agrees with it."""
import numpy as np
import pytest

import arp_cases as cases
import arp_ref as ref

BUILDERS = (
    [pytest.param(cases.rank, (free,), id=f"rank-free{free}") for free in (0, 1, 63, 64, 65, 300)] +
    [pytest.param(cases.replies, (pos,), id=f"replies-{pos}") for pos in (0, 63, 64, 257)] +
    [pytest.param(cases.lengths, (f,), id=f"lengths-flags{f}") for f in range(4)] +
    [pytest.param(cases.in_flight, (k,), id=f"in_flight-{k}") for k in range(8)] +
    [pytest.param(f, (), id=f.__name__) for f in (cases.three_hosts, cases.shared_mac, cases.flagged_and_near, cases.with_fcs,
                                                  cases.near_keys, cases.table_load, cases.two_hosts, cases.columns, cases.mixed,
                                                  cases.empty_batch, cases.no_hosts, cases.host_form)] +
    [pytest.param(cases.big, (n,), id=f"big-{n}") for n in (1, 1000, 65536)]
)


@pytest.mark.parametrize("builder, args", BUILDERS)
def test_the_batch_reaches_what_it_names(builder, args):
    case = builder(*args)
    want = cases.expected(case)
    assert want[5].size == want[6].size == len(case.frames) and want[0].size == len(case.hosts) and want[1].size == len(case.queries)
    assert want[2].size == 64 * (case.n_reply_slots + len(case.queries)) == 64 * want[3].size == 64 * want[4].size
    case.reaches(want)
    if len(case.frames) < 1000:  # the second statement says the same
        model = ref.recv_eth_model(case.frames, case.hosts, case.queries, case.n_reply_slots, case.arp_flags, mtu=case.mtu,
                                   fcs=bool(case.flags & 1))
        assert ref.same(want, model) == []


def test_the_noise_takes_no_rank():
    frames = cases.noisy()
    v = ref.verdicts(frames)
    assert len(frames) == 516 and (v[::2] == ref.FS_ARP).all() and set(int(x) for x in v[1::2]) == {0, 1, ref.FS_ARP}
    assert sorted({len(f) for f in frames[7::8]}) == list(range(34, 42)) and {len(f) for f in frames[::2]} == {42, 60}


def test_every_rejection_changes_one_good_list():
    hosts, queries, n_reply = cases.rejected_lists()
    assert n_reply == 6 and ref.expected([], [], hosts, queries, n_reply)[0].size == 3
    texts = set()
    for change, text in cases.REJECTIONS:
        h, q = hosts.copy(), queries.copy()
        change(h, q)
        assert (h.tobytes() != hosts.tobytes()) != (q.tobytes() != queries.tobytes()) and h[0].tobytes() == hosts[0].tobytes()
        texts.add(text)
    assert len(cases.REJECTIONS) == 9 and len(texts) == 8  # (two slot ranges past the end)
