"""What the host-form methods of seqs_amd/framesum.py hand to the C ABI, checked against a recording
stand-in for the library (no GPU, no built library): the function called, every scalar, every pointer,
the empty-batch rules and the error text. The loader's rules are checked on the same stand-in. The
device-form methods need CUDA tensors and are covered by the GPU suites."""
import ctypes

import numpy as np
import pytest

from seqs_amd import abi, framesum
from seqs_amd.framesum import (DIGEST_DTYPE, FCS_APPEND, FILL_CSUM, FLOW_DTYPE, FLOW_TOTALS_DTYPE, RUN_DTYPE,
                               SEND_DTYPE, TOTALS_DTYPE, Engine, FramesumError)

MESSAGE = b"the stand-in says no"
LAYOUT = (3, 4096)  # what the stand-in's fs_segment_layout reports: frames, bytes
TOTALS = {"payload_bytes": 3000, "n_runs": 2, "n_flows": 1, "n_accepted": 3}


def record_at(ptr, dtype):
    """The one record of `dtype` a c_void_p argument points to, as a writable numpy view."""
    raw = (ctypes.c_uint8 * dtype.itemsize).from_address(ptr.value)
    return np.frombuffer(raw, dtype=dtype, count=1)


class StandInFunction:
    def __init__(self, lib, name):
        self.lib, self.name, self.restype, self.argtypes = lib, name, None, None

    def __call__(self, *args):
        lib = self.lib
        lib.calls.append((self.name, args))
        if self.name in ("fs_last_error", "fs_group_last_error"):
            return MESSAGE
        if self.name in lib.fail:
            return lib.fail[self.name]
        if self.name == "fs_ctx_create":
            lib.contexts += 1
            args[1]._obj.value = 0x1000 * lib.contexts
        elif self.name == "fs_group_create":
            args[2]._obj.value = 0x9000
        elif self.name == "fs_segment_layout":
            args[4]._obj.value, args[5]._obj.value = LAYOUT
        elif self.name in ("fs_coalesce_batch_host", "fs_coalesce_flows_batch_host"):
            flows = "flows" in self.name
            t = record_at(args[14 if flows else 12], FLOW_TOTALS_DTYPE if flows else TOTALS_DTYPE)
            for field in t.dtype.names:
                t[field] = TOTALS.get(field, 0)
        return 0


class StandInLibrary:
    """ctypes.CDLL's stand-in: every fs_* attribute is a function that records (name, args) and
    returns 0, except the names in `absent`."""

    absent = frozenset()
    loaded = []

    def __init__(self, path):
        self.path, self.calls, self.fail, self.contexts = path, [], {}, 0
        StandInLibrary.loaded.append(self)

    def __getattr__(self, name):
        if not name.startswith("fs_") or name in self.absent:
            raise AttributeError(name)
        fn = StandInFunction(self, name)
        setattr(self, name, fn)
        return fn


@pytest.fixture
def standin(monkeypatch, tmp_path):
    """The stand-in class, in place of ctypes.CDLL, with the loader's cache empty and its product path an
    existing file; monkeypatch puts all of it back."""
    product = tmp_path / "libframesum.so"
    product.write_bytes(b"")
    monkeypatch.setattr(ctypes, "CDLL", StandInLibrary)
    monkeypatch.setattr(StandInLibrary, "absent", frozenset(abi.OPTIONAL_PROTOTYPES))
    monkeypatch.setattr(StandInLibrary, "loaded", [])
    monkeypatch.setattr(abi, "_LIB_PATH", str(product))
    monkeypatch.setattr(abi, "_lib", None)
    monkeypatch.setattr(abi, "_libs", {})
    return StandInLibrary


@pytest.fixture
def eng(standin):
    e = Engine(0)
    e.lib.calls.clear()
    yield e
    e.close()


def batch():
    """3 frames of 60, 61 and 1514 bytes at 4-aligned offsets."""
    lengths = np.array([60, 61, 1514], dtype=np.uint32)
    offsets = np.array([0, 60, 124], dtype=np.uint64)
    frames = np.arange(1640, dtype=np.uint32).astype(np.uint8)
    return frames, offsets, lengths


def plain(a):
    """An argument as the integer the C function receives."""
    return getattr(a, "value", a)


def check_call(call, name, expected):
    """`call` is (name, args) with the args equal to `expected`: an array stands for a pointer to its
    first byte, anything else for itself."""
    got_name, args = call
    assert got_name == name and len(args) == len(expected)
    for k, (a, e) in enumerate(zip(args, expected)):
        want = e.ctypes.data if isinstance(e, np.ndarray) else e
        assert plain(a) == want, f"{name} argument {k}"


def test_digest_host(eng):
    frames, offsets, lengths = batch()
    out, status = eng.digest_host(frames, offsets, lengths, 1500)
    assert out.dtype == DIGEST_DTYPE and out.shape == (3,) and status.dtype == np.uint8 and status.shape == (3,)
    (call,) = eng.lib.calls
    check_call(call, "fs_digest_batch_host",
               [eng._ctx.value, frames, frames.nbytes, offsets, lengths, 3, 1500, out, status])
    mine = np.zeros(4, dtype=DIGEST_DTYPE), np.zeros(3, dtype=np.uint8)
    out, status = eng.digest_host(frames, offsets, lengths, out=mine[0], status=mine[1])
    assert out is mine[0] and status is mine[1]
    check_call(eng.lib.calls[1], "fs_digest_batch_host",
               [eng._ctx.value, frames, frames.nbytes, offsets, lengths, 3, 0, out, status])


def test_host_batch_is_normalised(eng):
    # lists and other integer types are converted; what C sees has the ABI's element sizes
    frames, offsets, lengths = batch()
    eng.digest_host(frames, [int(o) for o in offsets], lengths.astype(np.int64))
    args = eng.lib.calls[0][1]
    assert plain(args[1]) == frames.ctypes.data and plain(args[5]) == 3
    assert plain(args[3]) != offsets.ctypes.data and plain(args[4]) != lengths.ctypes.data
    with pytest.raises(AssertionError, match="same frames"):
        eng.digest_host(frames, offsets[:2], lengths)


def test_fill_host(eng):
    frames, offsets, lengths = batch()
    out, status = eng.fill_host(frames, offsets, lengths, 9000, FILL_CSUM | FCS_APPEND)
    (call,) = eng.lib.calls
    check_call(call, "fs_fill_batch_host",
               [eng._ctx.value, frames, frames.nbytes, offsets, lengths, 3, 9000, 3, out, status])
    assert out.dtype == DIGEST_DTYPE and out.shape == (3,) and status.shape == (3,)
    eng.fill_host(frames, offsets, lengths)
    assert plain(eng.lib.calls[1][1][7]) == FILL_CSUM
    # the frames are written in place: never copied, so they must be a writable uint8 array already
    frozen = frames.copy()
    frozen.flags.writeable = False
    for bad in (frozen, list(frames), frames.astype(np.int8), frames[::2]):
        with pytest.raises(AssertionError):
            eng.fill_host(bad, offsets, lengths)
    assert len(eng.lib.calls) == 2


def test_segment_host(eng):
    sends = np.zeros(2, dtype=SEND_DTYPE)
    payload = np.arange(700, dtype=np.uint32).astype(np.uint8)
    frames, offsets, lengths, out, status = eng.segment_host(sends, payload, 1500, FCS_APPEND, 8)
    layout, build = eng.lib.calls  # fs_segment_layout goes first
    assert layout[0] == "fs_segment_layout" and len(layout[1]) == 6
    assert [plain(a) for a in layout[1][:4]] == [sends.ctypes.data, 2, FCS_APPEND, 8]
    check_call(build, "fs_segment_batch_host",
               [eng._ctx.value, sends, 2, payload, 700, 1500, FCS_APPEND, 8, frames, LAYOUT[1], offsets, lengths, out,
                status])
    assert frames.dtype == np.uint8 and frames.shape == (LAYOUT[1],)
    assert offsets.dtype == np.uint64 and lengths.dtype == np.uint32 and out.dtype == DIGEST_DTYPE
    assert offsets.shape == lengths.shape == out.shape == status.shape == (LAYOUT[0],)
    mine = np.zeros(5000, dtype=np.uint8)
    assert eng.segment_host(sends, payload, frames=mine)[0] is mine
    assert eng.lib.calls[3][0] == "fs_segment_batch_host"  # the defaults: mtu 0, flags 0, align 4
    assert [plain(a) for a in eng.lib.calls[3][1][5:10]] == [0, 0, 4, mine.ctypes.data, 5000]


def test_coalesce_host(eng):
    frames, offsets, lengths = batch()
    payload, runs, run_of, totals, out, status = eng.coalesce_host(frames, offsets, lengths, 1500, 1)
    (call,) = eng.lib.calls
    assert plain(call[1][12]) != 0
    check_call(call, "fs_coalesce_batch_host",
               [eng._ctx.value, frames, frames.nbytes, offsets, lengths, 3, 1500, 1, payload, 60 + 61 + 1514, runs,
                run_of, plain(call[1][12]), out, status])
    assert payload.dtype == np.uint8 and payload.shape == (60 + 61 + 1514,)
    assert runs.dtype == RUN_DTYPE and runs.shape == (TOTALS["n_runs"],)  # cut to the runs written
    assert run_of.dtype == np.uint32 and run_of.shape == (3,)
    assert totals.dtype == TOTALS_DTYPE and totals.shape == ()  # the record the stand-in wrote
    assert int(totals["payload_bytes"]) == TOTALS["payload_bytes"] and int(totals["n_runs"]) == TOTALS["n_runs"]
    assert out.dtype == DIGEST_DTYPE and out.shape == (3,) and status.shape == (3,)
    mine = np.zeros(100, dtype=np.uint8)
    assert eng.coalesce_host(frames, offsets, lengths, payload=mine)[0] is mine
    args = eng.lib.calls[1][1]
    assert [plain(a) for a in args[6:10]] == [0, 0, mine.ctypes.data, 100]


def test_coalesce_flows_host(eng):
    frames, offsets, lengths = batch()
    payload, runs, flows, order, run_of, totals, out, status = eng.coalesce_flows_host(frames, offsets, lengths, 1500)
    (call,) = eng.lib.calls
    check_call(call, "fs_coalesce_flows_batch_host",
               [eng._ctx.value, frames, frames.nbytes, offsets, lengths, 3, 1500, 0, payload, 60 + 61 + 1514, runs, flows,
                order, run_of, plain(call[1][14]), out, status])
    assert runs.dtype == RUN_DTYPE and runs.shape == (TOTALS["n_runs"],)
    assert flows.dtype == FLOW_DTYPE and flows.shape == (TOTALS["n_flows"],)
    assert order.dtype == np.uint32 and order.shape == (TOTALS["n_accepted"],)
    assert run_of.dtype == np.uint32 and run_of.shape == (3,)
    assert totals.dtype == FLOW_TOTALS_DTYPE and totals.shape == ()
    assert [int(totals[f]) for f in ("payload_bytes", "n_runs", "n_flows", "n_accepted")] == \
        [TOTALS[f] for f in ("payload_bytes", "n_runs", "n_flows", "n_accepted")]
    assert out.dtype == DIGEST_DTYPE and out.shape == (3,) and status.shape == (3,)


def test_digest_host_multi(standin):
    a, b = Engine(0), Engine(0)
    assert a.lib is b.lib and a._ctx.value != b._ctx.value
    a.lib.calls.clear()
    frames, offsets, lengths = batch()
    out, status = framesum.digest_host_multi([a, b], frames, offsets, lengths, 1500)
    (call,) = a.lib.calls
    assert list(call[1][0]) == [a._ctx.value, b._ctx.value]
    check_call((call[0], call[1][1:]), "fs_digest_batch_multi",
               [2, frames, frames.nbytes, offsets, lengths, 3, 1500, out, status])
    assert out.dtype == DIGEST_DTYPE and out.shape == (3,) and status.dtype == np.uint8 and status.shape == (3,)
    with pytest.raises(AssertionError, match="distinct"):
        framesum.digest_host_multi([a, a], frames, offsets, lengths)
    a.lib.fail["fs_digest_batch_multi"] = -2
    with pytest.raises(FramesumError) as err:
        framesum.digest_host_multi([a, b], frames, offsets, lengths)
    m = MESSAGE.decode()
    assert str(err.value) == f"fs_digest_batch_multi failed (-2): ctx 0: {m}; ctx 1: {m}"


def test_empty_batches(standin):
    a, b = Engine(0), Engine(0)
    a.lib.calls.clear()
    frames = np.zeros(16, dtype=np.uint8)
    none64, none32 = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32)
    # the digest and fill calls return empty results without a C call
    for out, status in (a.digest_host(frames, none64, none32), a.fill_host(frames, none64, none32),
                        framesum.digest_host_multi([a, b], frames, none64, none32)):
        assert out.dtype == DIGEST_DTYPE and out.shape == (0,) and status.dtype == np.uint8 and status.shape == (0,)
    assert a.lib.calls == []
    # the segment and coalesce calls still make theirs
    a.segment_host(np.zeros(0, dtype=SEND_DTYPE), np.zeros(0, dtype=np.uint8))
    a.coalesce_host(frames, none64, none32)
    a.coalesce_flows_host(frames, none64, none32)
    assert [c[0] for c in a.lib.calls] == ["fs_segment_layout", "fs_segment_batch_host", "fs_coalesce_batch_host",
                                           "fs_coalesce_flows_batch_host"]
    assert [plain(c[1][5]) for c in a.lib.calls[2:]] == [0, 0]


@pytest.mark.parametrize("name,call", [
    ("fs_digest_batch_host", lambda e, f, o, l: e.digest_host(f, o, l)),
    ("fs_fill_batch_host", lambda e, f, o, l: e.fill_host(f, o, l)),
    ("fs_segment_layout", lambda e, f, o, l: e.segment_host(np.zeros(1, dtype=SEND_DTYPE), f)),
    ("fs_segment_batch_host", lambda e, f, o, l: e.segment_host(np.zeros(1, dtype=SEND_DTYPE), f)),
    ("fs_coalesce_batch_host", lambda e, f, o, l: e.coalesce_host(f, o, l)),
    ("fs_coalesce_flows_batch_host", lambda e, f, o, l: e.coalesce_flows_host(f, o, l)),
    ("fs_ctx_set_kernel", lambda e, f, o, l: e.set_kernel(4)),
])
def test_failed_call_raises_with_name_status_and_message(eng, name, call):
    eng.lib.fail[name] = -2
    with pytest.raises(FramesumError) as err:
        call(eng, *batch())
    assert str(err.value) == f"{name} failed (-2): {MESSAGE.decode()}"
    # the message is asked of the call's context (of no context for the host-only layout)
    last = eng.lib.calls[-1]
    assert last[0] == "fs_last_error"
    assert plain(last[1][0]) == (None if name == "fs_segment_layout" else eng._ctx.value)


def test_failed_create_raises(standin):
    lib = framesum.load_library()
    lib.fail["fs_ctx_create"] = -4
    with pytest.raises(FramesumError) as err:
        Engine(3)
    assert str(err.value) == f"fs_ctx_create(3) failed (-4): {MESSAGE.decode()}"


def test_close_frees_pinned_then_destroys_once(standin):
    e = Engine(0)
    ctx = e._ctx.value
    e._pinned.add(0x7000)  # as host_empty records an allocation
    e.lib.calls.clear()
    e.close()
    e.close()
    assert [(n, [plain(a) for a in args]) for n, args in e.lib.calls] == [("fs_host_free", [ctx, 0x7000]),
                                                                         ("fs_ctx_destroy", [ctx])]
    assert e._ctx is None and e._pinned == set()
    g = framesum.Group([0, 1])
    g.lib.calls.clear()
    h = g._g
    g.close()
    g.close()
    assert g.lib.calls == [("fs_group_destroy", (h,))] and g._g is None


# ---- the loader ------------------------------------------------------------
def test_load_applies_the_tables(standin):
    lib = framesum.load_library()
    for name, (restype, argtypes) in abi.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
    for name in abi.OPTIONAL_PROTOTYPES:  # absent from this stand-in, as from the product library
        assert not hasattr(lib, name)


def test_load_sets_hooks_where_the_library_has_them(standin, monkeypatch, tmp_path):
    monkeypatch.setattr(standin, "absent", frozenset({"fs_debug_read_stamps"}))
    test_lib = tmp_path / "libframesum_test.so"
    test_lib.write_bytes(b"")
    lib = framesum.load_library(str(test_lib))
    for name, (restype, argtypes) in abi.OPTIONAL_PROTOTYPES.items():
        if name == "fs_debug_read_stamps":
            assert not hasattr(lib, name)
        else:
            assert getattr(lib, name).restype is restype and getattr(lib, name).argtypes == argtypes, name


def test_load_tolerates_only_set_workgroups_absent(standin, monkeypatch):
    monkeypatch.setattr(standin, "absent", standin.absent | {"fs_ctx_set_workgroups"})
    lib = framesum.load_library()
    assert not hasattr(lib, "fs_ctx_set_workgroups") and lib.fs_ctx_set_kernel.argtypes is not None
    monkeypatch.setattr(abi, "_lib", None)
    monkeypatch.setattr(abi, "_libs", {})
    monkeypatch.setattr(standin, "absent", standin.absent | {"fs_deinterleave"})
    with pytest.raises(AttributeError, match="fs_deinterleave"):
        framesum.load_library()


def test_load_caches_one_handle_per_path(standin, tmp_path):
    other = tmp_path / "other.so"
    other.write_bytes(b"")
    product = framesum.load_library()
    assert framesum.load_library() is product and framesum.load_library(framesum.lib_path()) is product
    second = framesum.load_library(str(other))
    assert second is not product and framesum.load_library(str(other)) is second
    assert framesum.load_library() is product
    assert [l.path for l in standin.loaded] == [framesum.lib_path(), str(other)]
    with pytest.raises(FramesumError, match="is missing"):
        framesum.load_library(str(tmp_path / "absent.so"))
