"""seqs_amd/abi.py's PROTOTYPES against the declarations of include/framesum.h: test_abi.py compares
the names, this compares the shapes (one binding type per parameter, of the header type's kind, and
the kind of the return value). No library is loaded."""
import ctypes
import os
import re

import pytest

from seqs_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int}


def header_declarations():
    """[(name, return type, [parameter text, ...])] in the header's order, comments stripped."""
    src = open(os.path.join(ROOT, "include", "framesum.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decls = re.findall(r"((?:const\s+)?\w+\s*\*?)\s*\b(fs_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", src)
    return [(name, " ".join(ret.split()), [p.strip() for p in params.split(",") if p.strip() != "void"])
            for ret, name, params in decls]


DECLS = header_declarations()


def is_pointer_type(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def test_parser_finds_every_declared_function():
    # the same names tests/test_abi.py finds with its looser pattern, each once
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "framesum.h")).read(), flags=re.S)
    names = [d[0] for d in DECLS]
    assert sorted(names) == sorted(set(re.findall(r"\b(fs_[a-z_0-9]+)\s*\(", src)))
    assert len(names) == 30


def test_table_lists_the_header_in_its_order():
    assert list(abi.PROTOTYPES) == [d[0] for d in DECLS]
    assert abi.EXPORTED_SYMBOLS == tuple(abi.PROTOTYPES)
    assert not set(abi.PROTOTYPES) & set(abi.OPTIONAL_PROTOTYPES)


@pytest.mark.parametrize("name,ret,params", DECLS, ids=[d[0] for d in DECLS])
def test_prototype_matches_declaration(name, ret, params):
    restype, argtypes = abi.PROTOTYPES[name]
    assert len(argtypes) == len(params), params
    for text, t in zip(params, argtypes):
        ctype = " ".join(w for w in text.replace("*", " * ").split()[:-1] if w != "const")
        if "*" in text or ctype == "hipStream_t":
            assert is_pointer_type(t), (text, t)
        else:
            assert t is SCALARS[ctype], (text, t)
    if ret in ("fs_status", "int"):
        assert restype in (ctypes.c_int, ctypes.c_int32) and ctypes.sizeof(restype) == 4
    elif ret == "const char*":
        assert restype is ctypes.c_char_p
    else:
        assert restype is SCALARS[ret]
