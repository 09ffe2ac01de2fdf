"""CPU: the node uid directory's C-ABI (include/kwok_watch.h): every
entry the header declares is exported and bound, its stat names equal the Python mirror,
and a null engine or null arrays are KWOK_EINVAL with the out parameters reset.

The bind entry is kwok_node_bind, not kwok_node_uid_bind: tests/test_uid_abi.py takes
every declared name that holds "uid" for an entry of the pod uid directory."""
import ctypes as C
import os
import re

from kwok_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kwok_watch.h")
ENTRIES = ["kwok_node_dir_enable", "kwok_node_lookup", "kwok_node_bind", "kwok_node_dir_stats"]


def header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_and_library_exports_the_entries():
    lib = engine.load_engine_lib()
    declared = set(re.findall(r"\b(kwok_[a-z_0-9]+)\s*\(", header()))
    assert sorted(f for f in declared if f.startswith("kwok_node_")) == sorted(ENTRIES)
    # the older ABI tests pick their entries by these substrings: the new names carry none of them
    for f in ENTRIES:
        assert not any(w in f for w in ("uid", "echo", "refs", "resync", "frame", "list", "watch")), f
    missing = [f for f in declared if not hasattr(lib, f)]
    assert not missing, missing
    for f in ENTRIES:
        assert getattr(lib, f).argtypes is not None, f  # (engine.py declares its signature)
    for m in ("node_dir_enable", "node_lookup", "node_bind", "node_dir_stats"):
        assert callable(getattr(engine.Engine, m)), m


def test_constants_and_stat_names_equal_the_python_mirror():
    src = header()
    body = re.search(r"enum\s*\{\s*(KWOK_NODE_DIR_STAT_\w+[^}]*)\}", src).group(1)
    ents = [x for x in (re.sub(r"\s*=.*", "", x).strip() for x in body.split(",")) if x]
    assert ents[-1] == "KWOK_NODE_DIR_STAT_COUNT"
    assert [x[len("KWOK_NODE_DIR_STAT_"):].lower() for x in ents[:-1]] == list(abi.NODE_DIR_STATS)
    assert abi.NODE_DIR_STATS == ("lookups", "hits", "notes", "binds", "unbound", "bytes")
    assert "KWOK_NODE_DIR_STAT_LOOKUPS = 0" in re.sub(r"\s+", " ", src)
    # a node's uid is bounded as a pod's, a looked-up name as a referenced one
    defs = dict(re.findall(r"#define\s+(KWOK_UID_MAX|KWOK_REF_NAME_MAX)\s+(\d+)", src))
    assert int(defs["KWOK_UID_MAX"]) == abi.UID_MAX == 40 and int(defs["KWOK_REF_NAME_MAX"]) == abi.REF_NAME_MAX == 253


def test_null_engine_and_null_arrays_are_einval():
    lib = engine.load_engine_lib()
    n = C.c_size_t(7)
    h = (C.c_int32 * 1)(0)
    off, ln = (C.c_uint64 * 1)(0), (C.c_uint32 * 1)(1)
    out = (C.c_uint64 * len(abi.NODE_DIR_STATS))()
    p = lambda a: C.cast(a, C.c_void_p)  # noqa: E731
    name = C.cast(C.c_char_p(b"n"), C.c_void_p)
    assert lib.kwok_node_dir_enable(None) == abi.EINVAL
    assert lib.kwok_node_lookup(None, name, p(off), p(ln), 1, p(h)) == abi.EINVAL
    assert lib.kwok_node_bind(None, p(h), name, p(off), p(ln), 1, C.byref(n)) == abi.EINVAL
    assert n.value == 0  # (the out parameter is reset before the checks)
    assert lib.kwok_node_dir_stats(None, out) == abi.EINVAL
    # null arrays with n != 0 are refused before the engine is looked at: any non-null pointer stands for it
    fake = C.cast(C.create_string_buffer(8), C.c_void_p)
    assert lib.kwok_node_lookup(fake, name, None, p(ln), 1, p(h)) == abi.EINVAL
    assert lib.kwok_node_lookup(fake, name, p(off), None, 1, p(h)) == abi.EINVAL
    assert lib.kwok_node_lookup(fake, name, p(off), p(ln), 1, None) == abi.EINVAL
    n.value = 7
    assert lib.kwok_node_bind(fake, None, name, p(off), p(ln), 1, C.byref(n)) == abi.EINVAL and n.value == 0
    assert lib.kwok_node_bind(fake, p(h), name, None, p(ln), 1, None) == abi.EINVAL
    assert lib.kwok_node_bind(fake, p(h), name, p(off), None, 1, None) == abi.EINVAL
    assert lib.kwok_node_dir_stats(fake, None) == abi.EINVAL
