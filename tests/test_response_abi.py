"""CPU: the C-ABI of the patch response entries (include/kwok_watch.h, include/kwok_response.h, DESIGN.md
§27): the headers declare them and the library exports them, the stat names equal the Python mirror, and a
null engine is KWOK_EINVAL before anything else is looked at."""
import ctypes as C
import os
import re

from kwok_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WATCH_H = os.path.join(ROOT, "include", "kwok_watch.h")
RESPONSE_H = os.path.join(ROOT, "include", "kwok_response.h")
WATCH_ENTRIES = ["kwok_frame_responses", "kwok_frame_responses_gpu", "kwok_response_stats"]
NOTE_ENTRIES = ["kwok_echo_note_framed"]


def header(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def declared(path):
    return set(re.findall(r"\b(kwok_[a-z_0-9]+)\s*\(", header(path)))


def test_headers_declare_and_library_exports_the_entries():
    lib = engine.load_engine_lib()
    assert sorted(f for f in declared(WATCH_H) if "response" in f) == sorted(WATCH_ENTRIES)
    # the note entry carries the ledger's name, by which the ledger's ABI test picks kwok_watch.h's entries:
    # it is declared in a header of its own
    assert sorted(declared(RESPONSE_H)) == NOTE_ENTRIES
    assert '#include "kwok_watch.h"' in header(RESPONSE_H)
    for f in WATCH_ENTRIES + NOTE_ENTRIES:
        assert hasattr(lib, f), f
        assert getattr(lib, f).argtypes is not None, f  # (engine.py declares its signature)
    for f in WATCH_ENTRIES:  # the older ABI tests pick their entries by these substrings
        assert not any(w in f for w in ("uid", "echo", "refs", "resync", "list", "watch", "kwok_node_")), f


def test_constants_equal_the_python_mirror():
    src = header(WATCH_H)
    body = re.search(r"enum\s*\{\s*(KWOK_RESP_STAT_\w+[^}]*)\}", src).group(1)
    ents = [x for x in (re.sub(r"\s*=.*", "", x).strip() for x in body.split(",")) if x]
    assert ents[-1] == "KWOK_RESP_STAT_COUNT"
    assert [x[len("KWOK_RESP_STAT_"):].lower() for x in ents[:-1]] == list(abi.RESP_STATS)
    assert ents[0] + " = 0" in re.sub(r"\s+", " ", src)
    # the stats of the watch framer and of the ledger are what they were
    assert abi.WATCH_STATS == ("frames", "host_frames", "stream_bytes", "framed_ingests")
    assert len(abi.ECHO_STATS) == 9
    defs = dict(re.findall(r"#define\s+(KWOK_RV_MAX|KWOK_UID_MAX)\s+(\d+)", src))
    assert int(defs["KWOK_RV_MAX"]) == abi.RV_MAX and int(defs["KWOK_UID_MAX"]) == abi.UID_MAX


def test_null_engine_is_einval():
    lib = engine.load_engine_lib()
    frames = (abi.WatchFrame * 1)()
    off, ln = (C.c_uint64 * 1)(0), (C.c_uint32 * 1)(2)
    idx = (C.c_uint32 * 1)(0)
    st = (C.c_int32 * 1)(7)
    out = (C.c_uint64 * len(abi.RESP_STATS))()
    p = lambda a: C.cast(a, C.c_void_p)  # noqa: E731
    buf = C.cast(C.c_char_p(b"{}"), C.c_void_p)
    nh, sid = C.c_size_t(7), C.c_uint64(7)
    assert lib.kwok_frame_responses_gpu(None, buf, 2, p(off), p(ln), 1, p(frames), C.byref(nh), C.byref(sid)) == abi.EINVAL
    assert nh.value == 0 and sid.value == 0  # (the out parameters are reset before the checks)
    assert lib.kwok_echo_note_framed(None, 1, p(idx), 1, p(st)) == abi.EINVAL
    assert st[0] == 7
    assert lib.kwok_response_stats(None, out) == abi.EINVAL
    # the host framer takes no engine: null arrays with n > 0, a null buffer with len > 0
    assert lib.kwok_frame_responses(buf, 2, None, p(ln), 1, p(frames)) == abi.EINVAL
    assert lib.kwok_frame_responses(None, 2, p(off), p(ln), 1, p(frames)) == abi.EINVAL
    assert lib.kwok_frame_responses(buf, 2, p(off), p(ln), 1, p(frames)) == 0
    assert frames[0].type == abi.WATCH_MODIFIED and frames[0].doc_len == 2
