"""The Go binding's TX frame build (go/eth/digest_gpu.go SegmentBatch). There is no Go toolchain in
this image, so the file is checked for the surface it must provide, as test_go_binding.py does."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO_ETH = os.path.join(ROOT, "go", "eth", "digest_gpu.go")


def test_go_file_declares_segment_batch():
    eth = open(GO_ETH).read()
    for sym in ("func (g *GPU) SegmentBatch(", "C.fs_segment_batch_host(", "C.fs_segment_layout(", "type Send struct",
                "C.FS_FCS_APPEND"):
        assert sym in eth, sym
    # SegmentBatch stands beside FillBatch, in the same build-tagged file
    assert eth.startswith("//go:build framesum")
    assert eth.index("func (g *GPU) FillBatch(") < eth.index("func (g *GPU) SegmentBatch(")
    # the fields of fs_tx_send it fills are the header's
    hdr = open(os.path.join(ROOT, "include", "framesum.h")).read()
    struct = hdr[hdr.index("typedef struct fs_tx_send"):hdr.index("} fs_tx_send;")]
    for field in re.findall(r"cs\[i\]\.([a-z_]+)", eth):
        assert re.search(r"\b" + field + r"\b", struct), field
