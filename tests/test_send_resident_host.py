"""The resident ring send (fs_send_rings_resident) without a GPU: the arithmetic of
seqs_amd/csrc/framesum_send_resident.h, and of the rule header as the device path uses it, under ASan +
UBSan (a stand-alone program run as a child process); the tenth header against the binding's table, record
layout and constants; and what the call rejects before it needs a device."""
import ctypes
import os
import re
import subprocess

import numpy as np

from seqs_amd import abi, framesum
from seqs_amd.framesum import TX_TOTALS_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tests", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
HEADER = open(os.path.join(ROOT, "include", "framesum_send_resident.h")).read()
BODY = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
NAMES = ["fs_send_rings_resident"]


def test_resident_arithmetic_under_asan_ubsan():
    out = os.path.join(CSRC, "build", "test_send_resident")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *SAN, "-o", out, os.path.join(CSRC, "test_send_resident.cpp")],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "send resident checks OK" in r.stdout


def test_resident_prototype_is_the_headers():
    assert re.findall(r"^fs_status\s+(fs_\w+)\s*\(", BODY, flags=re.M) == list(abi.SEND_RESIDENT_PROTOTYPES) == NAMES
    others = [abi.PROTOTYPES, abi.DELIVER_PROTOTYPES, abi.SEND_RINGS_PROTOTYPES, abi.RECV_PROTOTYPES, abi.ARP_PROTOTYPES]
    assert not any(set(NAMES) & set(t) for t in others)
    assert '#include "framesum_send.h"' in HEADER and '#include "framesum_recv.h"' in HEADER
    restype, argtypes = abi.SEND_RESIDENT_PROTOTYPES[NAMES[0]]
    params = BODY[BODY.index(NAMES[0] + "(") + len(NAMES[0]) + 1 :]
    params = [p.strip() for p in params[: params.index(")")].split(",")]
    assert restype is ctypes.c_int32 and len(params) == len(argtypes) == 22
    for p, t in zip(params, argtypes):
        want = ctypes.c_void_p if "*" in p else {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}[p.split()[0]]
        assert t is want, p
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "ctx", "socks", "n_socks", "rx_socks_out", "rx_snd_out", "rx_index", "n_rx", "rings", "rings_bytes", "mtu", "flags",
        "align", "frames", "frames_bytes", "frames_cap", "offsets", "lengths", "out", "status", "socks_out", "totals", "stream"]
    lib = framesum.load_library()
    assert lib.fs_send_rings_resident.restype is restype and lib.fs_send_rings_resident.argtypes == argtypes
    out = subprocess.run(["nm", "-D", "--defined-only", framesum.lib_path()], capture_output=True, text=True, check=True)
    assert set(NAMES) <= {l.split()[-1] for l in out.stdout.splitlines() if l.strip()}


def test_totals_dtype_and_constants_are_the_headers():
    body = BODY[BODY.index("typedef struct fs_tx_totals") : BODY.index("} fs_tx_totals;")]
    fields = [(c, nm.strip()) for c, names in re.findall(r"(uint\d+_t)\s+([a-z_, ]+);", body) for nm in names.split(",")]
    assert [nm for _, nm in fields] == list(TX_TOTALS_DTYPE.names) == ["n_frames", "frames_bytes", "data_bytes", "n_built",
                                                                       "n_idle", "n_deferred", "n_invalid"]
    at = 0
    for ctype, nm in fields:
        assert TX_TOTALS_DTYPE.fields[nm][1] == at, nm
        at += int(ctype[4:-2]) // 8
    assert at == TX_TOTALS_DTYPE.itemsize == 40 and "40 bytes, no padding" in HEADER
    defines = {k: int(v, 0) for k, v in re.findall(r"#define (FS_TX_\w+) (\w+)u", HEADER)}
    assert defines.pop("FS_TX_WRITEBACK") == abi.TX_WRITEBACK and defines.pop("FS_TX_NO_RX") == abi.TX_NO_RX
    assert (defines.pop("FS_TX_DEFERRED"), defines.pop("FS_TX_INVALID")) == (abi.TX_DEFERRED, abi.TX_INVALID)
    bad = {k[len("FS_"):]: v for k, v in defines.items()}
    assert list(bad.values()) == list(range(1, 13)) and all(getattr(abi, k) == v for k, v in bad.items())
    assert all(getattr(framesum, k) == v for k, v in bad.items())  # (the public module has them too)
    # the outcomes and the call flag share no bit with what they are or-ed with
    assert not (abi.TX_DEFERRED | abi.TX_INVALID) & (abi.TX_ACK | abi.TX_FIN | abi.TX_PSH) and not abi.TX_WRITEBACK & abi.FCS_APPEND


def test_a_null_context_is_rejected_before_anything_else():
    lib = framesum.load_library()
    some = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(4096)))
    assert lib.fs_send_rings_resident(None, some, 1, None, None, None, 0, some, 4096, 0, 0, 1, some, 4096, 8, None, None, None,
                                      None, some, some, None) == -1


def test_tx_socks_tensor_is_the_records():
    import torch

    recs = np.zeros(3, dtype=abi.TX_SOCK_DTYPE)
    recs["mss"], recs["flags"], recs["hdr"][:, 53] = [1, 2, 3], 7, 9
    t = framesum.tx_socks_tensor(recs, torch.device("cpu"))
    assert t.shape == (3, 104) and t.dtype == torch.uint8 and t.is_contiguous()
    assert np.array_equal(framesum._records(t, abi.TX_SOCK_DTYPE), recs)
    outs, tot = np.zeros(3, dtype=abi.TX_SOCK_OUT_DTYPE), np.zeros(1, dtype=TX_TOTALS_DTYPE)
    tot["n_frames"], outs["sent"] = 5, abi.TX_DEFERRED
    a, b, c = framesum.split_tx(torch.from_numpy(outs.view(np.uint8).reshape(3, 32)), torch.from_numpy(tot.view(np.uint8)), t)
    assert np.array_equal(a, outs) and int(b["n_frames"]) == 5 and np.array_equal(c, recs)
