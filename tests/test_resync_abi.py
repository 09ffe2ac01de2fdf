"""CPU: the relist-with-Replace ABI (include/kwok_watch.h): every
kwok_resync_* function the header declares is exported by the built library,
the Python mirror's enums equal the header's (printed by gcc from the header
itself), and every entry answers a null engine with KWOK_EINVAL."""
import ctypes as C
import os
import re
import subprocess
import tempfile

from kwok_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kwok_watch.h")
EXPECTED = {"kwok_resync_begin", "kwok_resync_mark", "kwok_resync_sweep", "kwok_resync_end", "kwok_resync_stats"}


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(f for f in set(re.findall(r"\b(kwok_[a-z_0-9]+)\s*\(", src)) if f.startswith("kwok_resync_"))


def test_header_declares_the_resync_entries_and_the_library_exports_them():
    fns = declared_functions()
    assert set(fns) == EXPECTED, fns
    lib = engine.load_engine_lib()
    missing = [f for f in fns if not hasattr(lib, f)]
    assert not missing, missing


def test_python_enums_equal_the_header():
    names = ["KWOK_KIND_NODES", "KWOK_KIND_PODS", "KWOK_RESYNC_STAT_SESSIONS", "KWOK_RESYNC_STAT_MARKED",
             "KWOK_RESYNC_STAT_SWEPT_NODES", "KWOK_RESYNC_STAT_SWEPT_PODS", "KWOK_RESYNC_STAT_RELEASED",
             "KWOK_RESYNC_STAT_COUNT"]
    lines = ['#include <stdio.h>', '#include "%s"' % HEADER, "int main(void){"]
    lines += ['printf("%s %%d\\n", (int)%s);' % (n, n) for n in names]
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "e.c")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-o", os.path.join(d, "e"), src])
        out = subprocess.check_output([os.path.join(d, "e")], text=True)
    got = {k: int(v) for k, v in (l.split() for l in out.strip().splitlines())}
    assert (got["KWOK_KIND_NODES"], got["KWOK_KIND_PODS"]) == (abi.KIND_NODES, abi.KIND_PODS)
    assert got["KWOK_RESYNC_STAT_COUNT"] == len(abi.RESYNC_STATS)
    order = ["SESSIONS", "MARKED", "SWEPT_NODES", "SWEPT_PODS", "RELEASED"]
    assert [got["KWOK_RESYNC_STAT_" + k] for k in order] == list(range(len(order)))
    assert [k.upper() for k in abi.RESYNC_STATS] == order


def test_null_engine_is_einval():
    lib = engine.load_engine_lib()
    n = C.c_size_t(7)
    hs = (C.c_int32 * 4)()
    out = (C.c_uint64 * len(abi.RESYNC_STATS))()
    for kind in (abi.KIND_NODES, abi.KIND_PODS):
        assert lib.kwok_resync_begin(None, kind) == abi.EINVAL
        assert lib.kwok_resync_end(None, kind) == abi.EINVAL
        assert lib.kwok_resync_mark(None, kind, hs, 4, C.byref(n)) == abi.EINVAL
        assert n.value == 0
        n.value = 7
        assert lib.kwok_resync_sweep(None, kind, hs, 4, C.byref(n), None, None) == abi.EINVAL
        assert n.value == 0
    assert lib.kwok_resync_stats(None, out) == abi.EINVAL
