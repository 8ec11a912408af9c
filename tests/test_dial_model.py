"""The handshake of tests/dial.py with the library's contract on both ends, run against the models alone (no
GPU): what tests/test_gpu_dial.py must also show on the device."""
import dial


def test_the_dial_against_the_models():
    r = dial.run(dial.Model())
    dial.check_end(r)
    # the duplicated SYN-ACKs reached the clients' flows and were left alone
    assert int(r["c2"]["n_accepted"]) == dial.N_CLIENTS + len(dial.DUPLICATED) + 2
