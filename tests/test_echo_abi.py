"""CPU: the echo ledger's C-ABI (include/kwok_watch.h): every entry the
header declares is exported, its constants and stat names equal the Python mirror (and
the host yardstick's ECHO_KEEP), and a null engine is KWOK_EINVAL before anything else
is looked at."""
import ctypes as C
import os
import re

from kwok_amd import abi, controller, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kwok_watch.h")
ENTRIES = ["kwok_echo_enable", "kwok_echo_update", "kwok_echo_match", "kwok_ingest_pods_framed_echo",
           "kwok_ingest_nodes_framed_echo", "kwok_echo_stats"]


def header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_and_library_exports_the_entries():
    lib = engine.load_engine_lib()
    declared = set(re.findall(r"\b(kwok_[a-z_0-9]+)\s*\(", header()))
    assert sorted(f for f in declared if "echo" in f) == sorted(ENTRIES)
    missing = [f for f in declared if not hasattr(lib, f)]
    assert not missing, missing


def test_constants_equal_the_python_mirror():
    src = header()
    defs = dict(re.findall(r"#define\s+(KWOK_RV_MAX|KWOK_ECHO_KEEP|KWOK_ECHO|KWOK_NOT_SENT)\s+(\d+)", src))
    assert int(defs["KWOK_RV_MAX"]) == abi.RV_MAX == 24
    assert int(defs["KWOK_ECHO_KEEP"]) == abi.ECHO_KEEP == controller.Echoes.ECHO_KEEP == 8
    assert int(defs["KWOK_ECHO"]) == abi.ECHO == 2 and int(defs["KWOK_NOT_SENT"]) == 1
    flat = re.sub(r"\s+", " ", src)
    assert "enum { KWOK_ECHO_NOTE = 0, KWOK_ECHO_FORGET = 1 }" in flat
    assert (abi.ECHO_NOTE, abi.ECHO_FORGET) == (0, 1)
    body = re.search(r"enum\s*\{\s*(KWOK_ECHO_STAT_\w+[^}]*)\}", src).group(1)
    ents = [re.sub(r"\s*=.*", "", x).strip() for x in body.split(",")]
    ents = [x for x in ents if x]
    assert ents[-1] == "KWOK_ECHO_STAT_COUNT"
    assert [x[len("KWOK_ECHO_STAT_"):].lower() for x in ents[:-1]] == list(abi.ECHO_STATS)
    assert ents[0] + " = 0" in flat


def test_null_engine_is_einval():
    lib = engine.load_engine_lib()
    n, m, k = C.c_size_t(7), C.c_size_t(7), C.c_size_t(7)
    out = (C.c_uint64 * len(abi.ECHO_STATS))()
    h = (C.c_int32 * 1)(0)
    off, ln = (C.c_uint64 * 1)(0), (C.c_uint32 * 1)(1)
    idx = (C.c_uint32 * 1)(0)
    op = (C.c_uint8 * 1)(0)
    p = lambda a: C.cast(a, C.c_void_p)  # noqa: E731
    arena = C.cast(C.c_char_p(b"u1"), C.c_void_p)
    assert lib.kwok_echo_enable(None) == abi.EINVAL
    assert lib.kwok_echo_update(None, p(op), arena, p(off), p(ln), p(off), p(ln), 1, p(h)) == abi.EINVAL
    assert lib.kwok_echo_match(None, arena, p(off), p(ln), p(off), p(ln), p(op), 1, p(op)) == abi.EINVAL
    assert lib.kwok_ingest_pods_framed_echo(None, None, 1, p(idx), 1, p(h), p(h), p(idx), C.byref(n), C.byref(m),
                                            C.byref(k)) == abi.EINVAL
    assert n.value == 0 and m.value == 0 and k.value == 0  # (the out parameters are reset before the checks)
    n, k = C.c_size_t(7), C.c_size_t(7)
    assert lib.kwok_ingest_nodes_framed_echo(None, None, 1, p(idx), 1, p(h), p(h), C.byref(n), C.byref(k)) == abi.EINVAL
    assert n.value == 0 and k.value == 0
    assert lib.kwok_echo_stats(None, out) == abi.EINVAL
