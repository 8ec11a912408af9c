"""The conversation of tests/conversation.py with the model back end alone (tests/send_ref.py and
tests/recv_ref.py, no GPU): it terminates, and it passes through what tests/test_gpu_conversation.py
runs it for: Seq across 2^32, ring wraps on both sides, a closed window, duplicates, three FINs and
their ACKs."""
import conversation as conv


def test_the_conversation_completes_and_reaches_what_it_names():
    A, B, stats = conv.run(conv.Model())
    print("rounds", stats["rounds"], "codes", stats["codes"].tolist(), "window closed", stats["window_closed"],
          "most frames in a call", stats["max_frames"], "calls", stats["calls"])
    conv.check_end(A, B, stats)
    assert stats["rounds"] <= 100 and conv.Params.max_rounds == 100
    # nothing is acknowledged that was not sent, no keepalive, and every admitted segment had room in its ring
    assert stats["codes"][3] == stats["codes"][5] == stats["codes"][6] == 0
    assert stats["window_closed"]["B"] == 0 and stats["max_frames"] <= 20
