"""CPU: the pod uid directory's C-ABI (include/kwok_watch.h): every
entry the header declares is exported, its constants and stat names equal the Python
mirror, and a null engine is KWOK_EINVAL before anything else is looked at."""
import ctypes as C
import os
import re

from kwok_amd import abi, controller, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kwok_watch.h")
ENTRIES = ["kwok_uid_dir_enable", "kwok_uid_bind", "kwok_uid_lookup", "kwok_ingest_pods_framed_uid", "kwok_uid_stats"]


def header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_and_library_exports_the_entries():
    lib = engine.load_engine_lib()
    declared = set(re.findall(r"\b(kwok_[a-z_0-9]+)\s*\(", header()))
    uid = sorted(f for f in declared if "uid" in f)
    assert uid == sorted(ENTRIES)
    missing = [f for f in declared if not hasattr(lib, f)]
    assert not missing, missing


def test_constants_equal_the_python_mirror():
    src = header()
    defs = dict(re.findall(r"#define\s+(KWOK_UID_MAX|KWOK_NOT_SENT)\s+(\d+)", src))
    assert int(defs["KWOK_UID_MAX"]) == abi.UID_MAX == 40
    assert int(defs["KWOK_NOT_SENT"]) == abi.NOT_SENT == controller.NOT_SENT == 1
    body = re.search(r"enum\s*\{\s*(KWOK_UID_STAT_\w+[^}]*)\}", src).group(1)
    ents = [re.sub(r"\s*=.*", "", x).strip() for x in body.split(",")]
    ents = [x for x in ents if x]
    assert ents[-1] == "KWOK_UID_STAT_COUNT"
    assert [x[len("KWOK_UID_STAT_"):].lower() for x in ents[:-1]] == list(abi.UID_STATS)
    assert ents[0] + " = 0" in re.sub(r"\s+", " ", src)


def test_null_engine_is_einval():
    lib = engine.load_engine_lib()
    n, m = C.c_size_t(7), C.c_size_t(7)
    out = (C.c_uint64 * len(abi.UID_STATS))()
    h = (C.c_int32 * 1)(0)
    off, ln = (C.c_uint64 * 1)(0), (C.c_uint32 * 1)(1)
    idx = (C.c_uint32 * 1)(0)
    p = lambda a: C.cast(a, C.c_void_p)  # noqa: E731
    assert lib.kwok_uid_dir_enable(None) == abi.EINVAL
    assert lib.kwok_uid_bind(None, p(h), C.c_char_p(b"u"), p(off), p(ln), 1, C.byref(n)) == abi.EINVAL
    assert n.value == 0  # (the out parameters are reset before the checks)
    assert lib.kwok_uid_lookup(None, C.c_char_p(b"u"), p(off), p(ln), 1, p(h)) == abi.EINVAL
    assert lib.kwok_ingest_pods_framed_uid(None, None, 1, p(idx), 1, p(h), p(h), p(idx), C.byref(n), C.byref(m)) == abi.EINVAL
    assert n.value == 0 and m.value == 0
    assert lib.kwok_uid_stats(None, out) == abi.EINVAL
