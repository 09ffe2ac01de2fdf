"""The host watch-stream framer (kwok_frame_watch, codec.cpp) against a Python
framer written from the rules of include/kwok_watch.h (json.loads per line,
first key wins, depth <= 64): all five event types, `object` ahead of `type`,
inner whitespace, blank and \\r\\n lines, an unterminated tail (consumed),
the empty stream, escaped uid / name (flag bits, raw spans), duplicated keys,
lines that are no object, unknown types, a missing or non-object `object`,
depth 64..67, a frames array that is too small and the length guard.
Reference: the watch.Event switch of pod_controller.go:272-343 and
node_controller.go:225-279 (client-go's "got invalid watch event type")."""
import ctypes as C

import numpy as np
import pytest

import watch_frames as wf
from kwok_amd import abi
from kwok_amd.codec import frame_watch
from kwok_amd.engine import KwokError, load_engine_lib

CASES = wf.cases()


def test_frame_record_layout():
    assert C.sizeof(abi.WatchFrame) == 48 and abi.WATCH_FRAME_DTYPE.itemsize == 48
    assert abi.WatchFrame.uid.offset == 16 and abi.WatchFrame.namespace_.offset == 40
    assert abi.WATCH_TILE % 1024 == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_framer_equals_the_rules(name):
    stream, _ = CASES[name]
    want, consumed = wf.py_frames(stream)
    got, used = frame_watch(stream)
    assert used == consumed == stream.rfind(b"\n") + 1, name
    wf.assert_frames_equal(got, wf.frames_array(want), name)


def test_known_answers():
    """a few frames spelled out, so that the two framers cannot agree on a wrong rule"""
    s, _ = CASES["all_types"]
    f, used = frame_watch(s)
    assert list(f["type"]) == [abi.WATCH_ADDED, abi.WATCH_MODIFIED, abi.WATCH_DELETED, abi.WATCH_BOOKMARK, abi.WATCH_ERROR]
    assert list(f["status"]) == [0] * 5 and used == len(s)
    r = f[0]
    assert s[r["doc_off"]:r["doc_off"] + r["doc_len"]] == s[len(b'{"type":"ADDED","object":'):s.index(b"\n") - 1]
    text = lambda r, k: s[r[k]["off"]:r[k]["off"] + r[k]["len"]]
    assert (text(r, "uid"), text(r, "resource_version"), text(r, "name"), text(r, "namespace_")) == \
        (b"u-pod-0", b"41", b"pod-0", b"default")
    s, _ = CASES["blank_lines"]
    f, used = frame_watch(s)
    assert list(f["type"]) == [abi.WATCH_NONE, abi.WATCH_MODIFIED, abi.WATCH_NONE, abi.WATCH_NONE, abi.WATCH_ADDED,
                               abi.WATCH_NONE] and list(f["status"]) == [0] * 6
    s, _ = CASES["unterminated_tail"]
    f, used = frame_watch(s)
    assert len(f) == 2 and s[used:] == wf.wrap(wf.POD)[:40]
    assert frame_watch(b"")[1] == 0 and len(frame_watch(b"")[0]) == 0
    f, used = frame_watch(CASES["only_tail"][0])
    assert len(f) == 0 and used == 0
    s, _ = CASES["escaped_uid_name"]
    f, _ = frame_watch(s)
    assert f[0]["flags"] == abi.FRAME_ESC_UID | abi.FRAME_ESC_NAME and f[0]["status"] == 0
    assert text(f[0], "uid") == b'u\\\\-\\"q\\"' and text(f[0], "name") == b"caf\\u00e9"
    s, _ = CASES["duplicate_type"]
    f, _ = frame_watch(s)
    assert f[0]["type"] == abi.WATCH_ADDED and f[0]["status"] == 0 and s[f[0]["doc_off"]] == ord("{")
    for name in ("non_object_lines", "unknown_type", "missing_object", "object_array"):
        f, _ = frame_watch(CASES[name][0])
        assert list(f["status"]) == [abi.EINVAL] * len(f) and not f["doc_len"].any(), name
    f, _ = frame_watch(CASES["depth"][0])
    assert list(f["status"]) == [0, 0, abi.EINVAL, abi.EINVAL]


def test_cap_too_small_reports_the_line_count():
    s, _ = CASES["all_types"]
    with pytest.raises(KwokError) as ei:
        frame_watch(s, cap=4)
    assert ei.value.code == abi.EINVAL and ei.value.n_frames == 5
    f, _ = frame_watch(s, cap=5)
    assert len(f) == 5


def test_length_guard_returns_before_reading():
    """len above the 32-bit limit over a 16-byte buffer: KWOK_EINVAL, no byte read"""
    lib = load_engine_lib()
    buf = C.create_string_buffer(b"0123456789abcde\n", 16)
    frames = np.zeros(4, abi.WATCH_FRAME_DTYPE)
    nf, used = C.c_size_t(7), C.c_size_t(7)
    for n in (0xFFFFFFF1, 1 << 32, (1 << 40) + 5):
        rc = lib.kwok_frame_watch(buf, n, frames.ctypes.data, 4, C.byref(nf), C.byref(used))
        assert rc == abi.EINVAL and nf.value == 0 and used.value == 0
