"""CPU: the C-ABI of the node status blob canonicaliser (include/kwok_canon.h): the header
declares its two entries and nothing else, the library exports them, the stat names equal the Python mirror,
a null engine is KWOK_EINVAL, and neither kwok_engine.h (every function there has an oracle twin) nor
kwok_watch.h (the older ABI tests pick its entries by name) declares a function of it."""
import ctypes as C
import os
import re

from kwok_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANON_H = os.path.join(ROOT, "include", "kwok_canon.h")
ENTRIES = ["kwok_canon_enable", "kwok_canon_stats"]


def header(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def declared(path):
    return set(re.findall(r"\b(kwok_[a-z_0-9]+)\s*\(", header(path)))


def test_header_declares_and_library_exports_the_entries():
    lib = engine.load_engine_lib()
    assert sorted(declared(CANON_H)) == ENTRIES
    assert '#include "kwok_engine.h"' in header(CANON_H)
    for f in ENTRIES:
        assert hasattr(lib, f), f
        assert getattr(lib, f).argtypes is not None, f  # (engine.py declares its signature)
    for h in ("kwok_engine.h", "kwok_watch.h", "kwok_response.h"):
        assert not [f for f in declared(os.path.join(ROOT, "include", h)) if "canon" in f], h


def test_stat_names_equal_the_python_mirror():
    src = header(CANON_H)
    body = re.search(r"enum\s*\{\s*(KWOK_CANON_STAT_\w+[^}]*)\}", src).group(1)
    ents = [x for x in (re.sub(r"\s*=.*", "", x).strip() for x in body.split(",")) if x]
    assert ents[-1] == "KWOK_CANON_STAT_COUNT"
    assert [x[len("KWOK_CANON_STAT_"):].lower() for x in ents[:-1]] == list(abi.CANON_STATS)
    assert ents[0] + " = 0" in re.sub(r"\s+", " ", src)
    assert abi.CANON_STATS == ("docs", "blobs", "bytes_in", "bytes_out", "docs_host", "calls")


def test_null_engine_is_einval():
    lib = engine.load_engine_lib()
    out = (C.c_uint64 * len(abi.CANON_STATS))(*([7] * len(abi.CANON_STATS)))
    assert lib.kwok_canon_enable(None, 1) == abi.EINVAL
    assert lib.kwok_canon_enable(None, 0) == abi.EINVAL
    assert lib.kwok_canon_stats(None, C.cast(out, C.c_void_p)) == abi.EINVAL
    assert list(out) == [7] * len(abi.CANON_STATS)
