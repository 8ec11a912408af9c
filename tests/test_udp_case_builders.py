"""Every batch of tests/udp_cases.py reaches what it names, shown with tests/udp_ref.py alone (no GPU, no
library): each case's `reaches` runs on the reference's expected tuple."""
import numpy as np
import pytest

import udp_cases as cases
import udp_ref as ref

BUILDERS = (
    [pytest.param(cases.rank, (free,), id=f"rank-free{free}") for free in (0, 1, 63, 64, 65, 300)] +
    [pytest.param(cases.wrap, (n,), id=f"wrap-{n}") for n in (1, 5)] +
    [pytest.param(cases.payload_lengths, (c,), id=f"payload_lengths-{c}") for c in (1504, 96)] +
    [pytest.param(cases.truncation, (c,), id=f"truncation-{c}") for c in (40, 48, 1504)] +
    [pytest.param(cases.headers, (listed,), id=f"headers-{listed}") for listed in ("exact", "wildcard", "both")] +
    [pytest.param(cases.in_flight, (k,), id=f"in_flight-{k}") for k in range(8)] +
    [pytest.param(f, (), id=f.__name__) for f in (cases.three_ports, cases.largest, cases.with_fcs, cases.near_keys, cases.table_load,
                                                  cases.two_queues, cases.columns, cases.mixed, cases.empty_batch, cases.no_ports,
                                                  cases.host_span)] +
    [pytest.param(cases.benchmark, (n,), id=f"benchmark-{n}") for n in (1, 1000, 65536)]
)


@pytest.mark.parametrize("builder, args", BUILDERS)
def test_the_batch_reaches_what_it_names(builder, args):
    case = builder(*args)
    want = cases.expected(case)
    assert want[1].size == len(case.frames) and want[0].size == len(case.ports)
    case.reaches(want)


def test_the_copy_kernels_both_have_cases():
    """A port list whose largest cell is at most 96 bytes takes the 4-lane copy, any other the 16-lane copy
    (seqs_amd/csrc/framesum_udp.h copy_lanes): both have batches, with truncation on either side."""
    largest = {name: int(builder(*args).ports["cell_size"].max()) for name, builder, args in
               (("narrow", cases.truncation, (40,)), ("edge", cases.payload_lengths, (96,)), ("wide", cases.truncation, (1504,)),
                ("mixed sizes", cases.largest, ()))}
    assert largest == {"narrow": 40, "edge": 96, "wide": 1504, "mixed sizes": 65568}


def test_the_noise_takes_no_rank():
    frames = cases.noisy()
    v = ref.verdicts(frames)
    assert len(frames) == 516 and (v[::2] == 0).all() and set(int(x) for x in v[1::2]) == {0, 13}
    assert [f[23] for f in frames[1:8:2]] == [17, 6, 17, 17]


def test_every_rejection_changes_one_good_list():
    ports, cells_bytes = cases.rejected_ports()
    assert int(ports["cells_off"][1]) + 4 * 48 == cells_bytes
    texts = set()
    for change, text in cases.REJECTIONS:
        p = ports.copy()
        change(p)
        assert p.tobytes() != ports.tobytes() and p[0].tobytes() == ports[0].tobytes()
        texts.add(text)
    assert len(cases.REJECTIONS) == 13 and len(texts) == 10  # (three bad cell sizes, two bad cell counts)
