"""CPU: the reference directory's C-ABI (include/kwok_watch.h): every
entry the header declares is exported, its constants, struct layout and stat names equal
the Python mirror, and a null engine is KWOK_EINVAL with the out parameters reset."""
import ctypes as C
import os
import re

import numpy as np

from kwok_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kwok_watch.h")
ENTRIES = ["kwok_refs_enable", "kwok_refs_bind", "kwok_refs_lookup", "kwok_read_refs", "kwok_refs_stats"]


def header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def enum_names(src, first):
    body = re.search(r"enum\s*\{\s*(%s\b[^}]*)\}" % first, src).group(1)
    return [x for x in (re.sub(r"\s*=.*", "", x).strip() for x in body.split(",")) if x]


def test_header_declares_and_library_exports_the_entries():
    lib = engine.load_engine_lib()
    declared = set(re.findall(r"\b(kwok_[a-z_0-9]+)\s*\(", header()))
    assert sorted(f for f in declared if "refs" in f) == sorted(ENTRIES)
    # the older ABI tests pick their entries by these substrings: the new names carry none of them
    for f in ENTRIES:
        assert not any(w in f for w in ("uid", "echo", "resync", "frame", "list", "watch")), f
    missing = [f for f in declared if not hasattr(lib, f)]
    assert not missing, missing
    for f in ENTRIES:
        assert getattr(lib, f).argtypes is not None, f  # (engine.py declares its signature)


def test_constants_equal_the_python_mirror():
    src = header()
    defs = dict(re.findall(r"#define\s+(KWOK_REFS?_[A-Z_]+)\s+(\d+)", src))
    assert int(defs["KWOK_REF_NS_MAX"]) == abi.REF_NS_MAX == 63
    assert int(defs["KWOK_REF_NAME_MAX"]) == abi.REF_NAME_MAX == 253
    assert int(defs["KWOK_REF_STRIDE"]) == abi.REF_STRIDE == 320 == (63 + 253 + 15) // 16 * 16
    assert int(defs["KWOK_REF_NONE"]) == abi.REF_NONE == 3
    assert int(defs["KWOK_REFS_ANY_SLOT"]) == abi.REFS_ANY_SLOT == 1
    assert abi.REF_NONE not in (abi.OK, abi.NOT_SENT, abi.ECHO)
    lists = enum_names(src, "KWOK_REFS_HEARTBEAT")
    assert lists == ["KWOK_REFS_HEARTBEAT", "KWOK_REFS_NODE_INIT", "KWOK_REFS_POD_PATCH", "KWOK_REFS_DELETE",
                     "KWOK_REFS_LIST_COUNT"]
    assert (abi.REFS_HEARTBEAT, abi.REFS_NODE_INIT, abi.REFS_POD_PATCH, abi.REFS_DELETE) == (0, 1, 2, 3)
    ents = enum_names(src, "KWOK_REFS_STAT_BINDS")
    assert ents[-1] == "KWOK_REFS_STAT_COUNT"
    assert [x[len("KWOK_REFS_STAT_"):].lower() for x in ents[:-1]] == list(abi.REFS_STATS)
    flat = re.sub(r"\s+", " ", src)
    assert "KWOK_REFS_STAT_BINDS = 0" in flat and "KWOK_REFS_HEARTBEAT = 0" in flat


def test_kwok_ref_layout():
    body = re.search(r"typedef struct kwok_ref \{(.*?)\} kwok_ref;", header(), flags=re.S).group(1)
    fields = re.findall(r"\b(\w+)\s*[,;]", body)
    assert fields == ["off", "ns_len", "name_len", "uid_len", "status", "reserved0"] == [f for f, _t in abi.Ref._fields_]
    assert C.sizeof(abi.Ref) == 16 == abi.REF_DTYPE.itemsize
    offs = {f: getattr(abi.Ref, f).offset for f, _t in abi.Ref._fields_}
    assert offs == dict(off=0, ns_len=8, name_len=9, uid_len=10, status=11, reserved0=12)
    assert abi.REF_DTYPE["status"] == np.int8 and abi.REF_DTYPE["off"] == np.uint64


def test_null_engine_is_einval():
    lib = engine.load_engine_lib()
    n = C.c_size_t(7)
    h = (C.c_int32 * 1)(0)
    off, ln = (C.c_uint64 * 1)(0), (C.c_uint32 * 1)(1)
    refs = (abi.Ref * 1)()
    blob = (C.c_uint8 * 64)()
    out = (C.c_uint64 * len(abi.REFS_STATS))()
    p = lambda a: C.cast(a, C.c_void_p)  # noqa: E731
    assert lib.kwok_refs_enable(None) == abi.EINVAL
    assert lib.kwok_refs_bind(None, p(h), C.cast(C.c_char_p(b"n"), C.c_void_p), p(off), p(ln), p(off), p(ln), 1,
                              C.byref(n)) == abi.EINVAL
    assert n.value == 0  # (the out parameters are reset before the checks)
    n.value = 7
    assert lib.kwok_refs_lookup(None, abi.KIND_PODS, p(h), 1, 0, p(refs), p(blob), 64, C.byref(n)) == abi.EINVAL
    assert n.value == 0
    n.value = 7
    assert lib.kwok_read_refs(None, abi.REFS_DELETE, 0, 1, p(refs), p(blob), 64, C.byref(n)) == abi.EINVAL
    assert n.value == 0
    assert lib.kwok_refs_stats(None, out) == abi.EINVAL
