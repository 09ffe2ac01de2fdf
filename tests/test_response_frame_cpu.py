"""CPU: the host framer of patch response bodies (kwok_frame_responses, codec.cpp) against two
oracles (tests/response_bodies.py): the watch framer over the same object in a MODIFIED envelope - status,
flags, doc_len and the four spans, offsets rebased to the body - and a Python restatement of the rules for
what the envelope cannot express (bad spans, blank bodies, the depth limit counted from the body's root)."""
import ctypes as C

import numpy as np

import response_bodies as rb
import watch_frames as wf
from kwok_amd import abi, engine
from kwok_amd.codec import frame_responses


def check(buf, offs, lens, oracles, where):
    got = frame_responses(buf, offs, lens)
    assert len(got) == len(offs)
    for i, (o, n) in enumerate(zip(offs.tolist(), lens.tolist())):
        g = wf.as_dict(got[i])
        assert got[i]["reserved0"] == 0
        if oracles[i] & rb.W:
            assert g == rb.envelope_frame(buf, o, n), (where, i, "envelope")
        if oracles[i] & rb.P:
            assert g == rb.python_frame(buf, o, n), (where, i, "python")
    return got


def test_every_case_alone_and_all_in_one_buffer():
    cs = rb.cases()
    for name, body, _nh, oracles in cs:
        for lead in (b"", b"\x00" * 5):  # at offset 0, and behind bytes no span covers
            buf = lead + body + b"#"
            check(buf, np.array([len(lead)], np.uint64), np.array([len(body)], np.uint32), [oracles], name)
    buf, offs, lens = rb.pack([c[1] for c in cs])
    got = check(buf, offs, lens, [c[3] for c in cs], "all cases")
    ok = got[(got["status"] == abi.OK) & (got["type"] == abi.WATCH_MODIFIED)]
    assert len(ok) > 40 and (got["status"] == abi.EINVAL).sum() >= 14 and (got["type"] == abi.WATCH_NONE).sum() >= 16
    assert (ok["line_off"] == offs[(got["status"] == abi.OK) & (got["type"] == abi.WATCH_MODIFIED)]).all()


def test_named_expectations():
    """what the issue states about single cases, read from the frames themselves"""
    cs = {c[0]: c[1] for c in rb.cases()}

    def one(name):
        b = cs[name]
        f = frame_responses(b, [0], [len(b)])[0]
        text = lambda k: b[int(f[k]["off"]):int(f[k]["off"]) + int(f[k]["len"])]  # noqa: E731
        return f, text

    f, text = one("pretty")
    assert f["status"] == abi.OK and text("uid") and text("name") and b"\n" in cs["pretty"][:f["doc_len"]]
    assert cs["pretty"][f["doc_off"] + f["doc_len"] - 1:] == b"}\n"
    f, text = one("duplicate_metadata")
    assert (text("name"), text("uid"), text("resource_version")) == (b"first", b"u1", b"")
    f, text = one("duplicate_uid")
    assert (text("uid"), text("name")) == (b"first", b"a")
    f, text = one("deeper_metadata_only")
    assert f["status"] == abi.OK and f["type"] == abi.WATCH_MODIFIED and not text("uid") and not text("name")
    f, text = one("deeper_metadata_too")
    assert text("uid") == b"outer"
    f, text = one("uid_number")
    assert not text("uid") and text("resource_version") == b"12" and f["flags"] == 0
    f, text = one("escaped_uid_name")
    assert f["flags"] == abi.FRAME_ESC_UID | abi.FRAME_ESC_NAME
    f, text = one("escaped_rv_ns")
    assert f["flags"] == abi.FRAME_ESC_RV | abi.FRAME_ESC_NS and text("resource_version") == b"4\\u0031"
    f, text = one("escaped_key_uid")
    assert f["status"] == abi.OK and text("uid") == b"u" and text("name") == b"n"  # (compared as decoded text)
    f, text = one("status_error")
    assert f["status"] == abi.OK and f["type"] == abi.WATCH_MODIFIED and f["uid"]["len"] == 0
    for name in ("invalid_%d" % k for k in range(13)):
        assert one(name)[0]["status"] == abi.EINVAL, name
    for name in ("empty", "whitespace"):
        f, _ = one(name)
        assert f["status"] == abi.OK and f["type"] == abi.WATCH_NONE
    assert one("depth_65")[0]["status"] == abi.OK and one("depth_66")[0]["status"] == abi.EINVAL
    assert [rb.escaped_routed_key(c[1]) for c in rb.cases()] == [bool(c[2]) for c in rb.cases()]


def test_bad_spans_fail_their_frame_only():
    pod = rb.compact(rb.golden_docs()[0])
    buf = pod + b"\n" + pod
    n = len(buf)
    offs = np.array([0, n, n, n - 3, 0xFFFFFFFF, len(pod) + 1, 1 << 40, 0], np.uint64)
    lens = np.array([len(pod), 1, 0, 4, 2, len(pod), 1, n + 1], np.uint32)
    got = check(buf, offs, lens, [rb.W | rb.P, rb.P, rb.P, rb.P, rb.P, rb.W | rb.P, rb.P, rb.P], "bad spans")
    assert got["status"].tolist() == [abi.OK, abi.EINVAL, abi.OK, abi.EINVAL, abi.EINVAL, abi.OK, abi.EINVAL, abi.EINVAL]
    assert got[2]["type"] == abi.WATCH_NONE  # an empty span at the buffer's end holds no byte outside it
    assert got[5]["doc_off"] == len(pod) + 1 and got[5]["doc_len"] == len(pod)
    for i in (1, 3, 4, 6, 7):
        assert got[i].tobytes() == rb.wf.frames_array([rb.zero_frame(abi.EINVAL)])[0].tobytes()


def test_length_guard_and_empty_calls():
    lib = engine.load_engine_lib()
    frames = np.zeros(2, abi.WATCH_FRAME_DTYPE)
    frames["status"] = 5
    off, ln = np.zeros(1, np.uint64), np.ones(1, np.uint32)
    buf = b"{}"
    call = lambda n_bytes, n: lib.kwok_frame_responses(buf, n_bytes, off.ctypes.data, ln.ctypes.data, n,  # noqa: E731
                                                       frames.ctypes.data)
    assert call(0xFFFFFFF1, 1) == abi.EINVAL and frames["status"][0] == 5  # (before any byte is read)
    assert call(1 << 32, 1) == abi.EINVAL
    assert call(2, 0) == 0 and frames["status"][0] == 5                    # n = 0: nothing written
    assert lib.kwok_frame_responses(None, 0, None, None, 0, None) == 0
    assert len(frame_responses(b"", [], [])) == 0
    f = frame_responses(b"", [0], [0])  # an empty buffer, an empty span
    assert f[0]["status"] == abi.OK and f[0]["type"] == abi.WATCH_NONE
    assert call(2, 1) == 1 and frames["status"][0] == abi.EINVAL  # "{" alone
    assert C.sizeof(abi.WatchFrame) == 48
