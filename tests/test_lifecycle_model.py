"""The six lifecycles of tests/lifecycle.py against the models alone (tests/segment_ref.py, tests/send_ref.py,
tests/close_ref.py): no GPU, no library call. It shows that the driver reaches what it names."""
import close_ref as cref
import lifecycle as lc


def test_the_lifecycles_against_the_models():
    r = lc.run(lc.Model())
    lc.check_end(r)
    # every ending went through the states its name says, one RX call per batch
    assert [name for name, _ in r["log"]] == ["data", "round A", "round B", "round C"]
    e3 = r["e3"]
    assert int(e3["n_flows"]) == 6 and int(e3["closers_out"]["n_taken"].sum()) == 3
    assert [int(x) for x in r["e4"]["closers_out"]["n_taken"]] == [1, 1, 0, 0]
    assert int(r["e5"]["closers_out"]["flags"][0]) == 0 and int(r["e5"]["closers_out"]["state"][0]) == cref.CLOSED
