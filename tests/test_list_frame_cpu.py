"""The host framer of List bodies (kwok_frame_list, codec.cpp) against the Python
framer of list_bodies.py on every named case, a few known answers spelled out,
the cap and length guards, every prefix of a two-item body, the structs' sizes.
Reference: pod_controller.go:357-368, node_controller.go:282-296 (the typed
decode of the List response this replaces)."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import list_bodies as lb
import watch_frames as wf
from kwok_amd import abi
from kwok_amd.codec import frame_list, list_text
from kwok_amd.engine import KwokError, load_engine_lib


def host(body):
    """(status, frames, info as a dict) by the host framer"""
    try:
        frames, info = frame_list(body)
    except KwokError as err:
        assert err.code == abi.EINVAL and err.n_frames == 0
        return abi.EINVAL, np.zeros(0, abi.WATCH_FRAME_DTYPE), None
    return abi.OK, frames, lb.info_dict(info)


@pytest.mark.parametrize("name", list(lb.cases()))
def test_host_framer_equals_the_python_framer(name):
    body = lb.cases()[name][0]
    want_st, want_frames, want_info = lb.py_list(body)
    st, frames, info = host(body)
    assert st == want_st, name
    if st == abi.OK:
        wf.assert_frames_equal(frames, lb.frames_array(want_frames), name)
        assert info == want_info, name


def test_outcomes_of_the_cases():
    ok = {n for n, (b, _h, _w) in lb.cases().items() if host(b)[0] == abi.OK}
    bad = set(lb.cases()) - ok
    assert {"pod_list", "items_absent", "items_null", "items_empty", "duplicate_items", "two_root_arrays", "depth_64",
            "depth_65", "escaped_items_key", "root_array_not_items", "brackets_in_strings"} <= ok
    assert {"depth_66", "depth_67", "item_number", "item_then_number", "item_nested_array", "item_trailing_comma",
            "items_no_comma", "items_object", "items_string", "body_array", "body_empty", "trailing_garbage",
            "bad_item_inside", "mismatched_close"} <= bad


def test_known_answers():
    body = (b'{"kind":"PodList","metadata":{"resourceVersion":"12","continue":"a\\u003d"},"items":['
            b'{"metadata":{"name":"p0","namespace":"ns","uid":"u0","resourceVersion":"5"}},'
            b' {"metadata":{"uid":"a\\"}{","name":""},"x":"]"}]}')
    frames, info = frame_list(body)
    assert len(frames) == 2
    i0 = body.index(b'{"metadata":{"name":"p0"')
    f = wf.as_dict(frames[0])
    assert f == dict(line_off=i0, doc_off=i0, doc_len=76, type=abi.WATCH_ADDED, flags=0, status=0,
                     uid=(body.index(b'"u0"') + 1, 2), resource_version=(body.index(b'"5"') + 1, 1), name=(body.index(b"p0"), 2),
                     namespace_=(body.index(b"ns"), 2))
    assert body[i0 + 76:i0 + 78] == b", "
    i1 = i0 + 78
    g = wf.as_dict(frames[1])
    assert g == dict(line_off=i1, doc_off=i1, doc_len=len(body) - 2 - i1, type=abi.WATCH_ADDED, flags=abi.FRAME_ESC_UID,
                     status=0, uid=(body.index(b'a\\"}{'), 5), resource_version=(0, 0), name=(0, 0), namespace_=(0, 0))
    assert lb.info_dict(info) == dict(kind=(9, 7), resource_version=(body.index(b'"12"') + 1, 2),
                                      continue_=(body.index(b"a\\u003d"), 7), items=(body.index(b"["), len(body) - 1 - body.index(b"[")),
                                      flags=abi.LIST_ESC_CONTINUE)
    assert list_text(body, info.continue_, True) == "a=" and list_text(body, info.kind) == "PodList"


def test_cap_and_length_guard():
    lib = load_engine_lib()
    body = lb.cases()["pod_list"][0]
    frames = np.zeros(8, abi.WATCH_FRAME_DTYPE)
    nf, info = C.c_size_t(), abi.ListInfo()
    call = lambda n, cap: lib.kwok_frame_list(body, n, frames.ctypes.data, cap, C.byref(nf), C.byref(info))
    assert call(len(body), 2) == abi.EINVAL and nf.value == 3 and info.kind.len == 0
    assert call(1 << 32, 8) == abi.EINVAL and nf.value == 0  # (before any byte is read)
    assert call(len(body), 3) == 0 and nf.value == 3 and info.kind.len == 7
    with pytest.raises(KwokError) as ei:
        frame_list(body, cap=1)
    assert ei.value.code == abi.EINVAL and ei.value.n_frames == 3
    bad = lb.cases()["item_then_number"][0]  # a body that is no list is judged before cap is
    assert lib.kwok_frame_list(bad, len(bad), frames.ctypes.data, 0, C.byref(nf), C.byref(info)) == abi.EINVAL and nf.value == 0


def test_every_prefix_is_invalid():
    body = lb.PREFIX_BODY
    assert 300 <= len(body) <= 500
    st, frames, _ = host(body)
    assert st == abi.OK and len(frames) == 2
    for k in range(len(body)):
        assert host(body[:k])[0] == abi.EINVAL, k
    assert host(body + b" \n")[0] == abi.OK


def test_struct_sizes_match_the_header():
    hdr = (pathlib.Path(__file__).resolve().parents[1] / "include" / "kwok_watch.h").read_text()
    assert C.sizeof(abi.ListInfo) == 40 == abi.LIST_INFO_DTYPE.itemsize
    assert C.sizeof(abi.WatchFrame) == 48
    m = re.search(r"typedef struct kwok_list_info \{(.*?)\} kwok_list_info;", hdr, re.S)
    fields = re.findall(r"(\w+)[,;]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [n for n, _ in abi.ListInfo._fields_]
    stats = re.findall(r"KWOK_LIST_STAT_(\w+)", re.search(r"enum \{\s*KWOK_LIST_STAT_BODIES.*?\};", hdr, re.S).group(0))
    assert [s for s in dict.fromkeys(stats) if s != "COUNT"] == ["BODIES", "ITEMS", "HOST_ITEMS", "HOST_BODIES", "BYTES"]
    assert len(abi.LIST_STATS) == 5
    assert (abi.LIST_ESC_KIND, abi.LIST_ESC_RV, abi.LIST_ESC_CONTINUE) == (1, 2, 4)
