"""GPU: patch responses on the device (include/kwok_watch.h, include/kwok_response.h).

1. kwok_frame_responses_gpu (json.hip k_resp_parse) against the host framer, frame for frame: the CPU file's
   cases plus seeded mutations of the golden documents, 130 documents a call (json_block gives 64-thread blocks
   here: two full blocks and a partial one), buffer lengths with len % 16 in {0, 1, 15} and the last document
   ending exactly at len; n_host equals the documents with an escaped routed key, counted on the CPU.
2. kwok_echo_note_framed (echo.hip k_echo_key_note_frames) on one engine against kwok_echo_update with the
   same (uid, rv) text on another: the per-record statuses of the header's table, then identical
   kwok_echo_match answers and kwok_echo_stats.
3. The response buffer as THE resident stream: kwok_ingest_pods_framed_uid over response frames against
   kwok_frame_watch_gpu over the same objects in MODIFIED envelopes on a second engine."""
import ctypes as C
import json
import random

import numpy as np
import pytest

import response_bodies as rb
import watch_frames as wf
from kwok_amd import abi
from kwok_amd.codec import Codec, frame_responses
from kwok_amd.engine import Engine, KwokError, make_config
from test_json_fuzz_gpu import dup_first, escape_some, mutate

pytestmark = pytest.mark.gpu

KW = dict(cidr="10.0.0.1/16", buckets=64, node_slots_per_bucket=16, pod_slots_per_bucket=128)


@pytest.fixture(scope="module")
def eng():
    e = Engine(make_config(**KW))
    yield e
    e.close()


# ---- 1. framer parity ------------------------------------------------------------------
def corpus():
    rng = random.Random(2027)
    docs = rb.golden_docs()
    out = [c[1] for c in rb.cases()]
    for _ in range(200):
        text = json.dumps(mutate(rng.choice(docs), rng), indent=rng.choice([None, None, 1]), ensure_ascii=rng.random() < 0.5)
        r = rng.random()
        if r < 0.15:
            text = dup_first(text, rng)
        elif r < 0.40:
            text = escape_some(text, rng)
        elif r < 0.48:
            text = text[:rng.randrange(1, len(text))]  # cut short
        elif r < 0.55:
            text = rng.choice(["[%s]", "%s x", "%s%s"]).replace("%s", text)
        out.append(rng.choice([b"", b" ", b"\n\t"]) + text.encode() + rng.choice([b"", b"\n", b" \r\n"]))
    rng.shuffle(out)
    return out


def test_frames_equal_the_host_framer(eng):
    bodies = corpus()
    assert len(bodies) > 260
    s0 = eng.response_stats()
    total = listed = n_bytes = 0
    want_all = []
    for k, lo in enumerate(range(0, len(bodies), 130)):
        part = bodies[lo:lo + 130]
        if not part[-1]:
            part = part[::-1]  # (the last document holds a byte, so that it ends AT len)
        buf, offs, lens = rb.pack(part, pad_to=(16, (0, 1, 15)[k % 3]))
        assert len(buf) % 16 == (0, 1, 15)[k % 3] and int(offs[-1]) + int(lens[-1]) == len(buf) and lens[-1] > 0
        want = frame_responses(buf, offs, lens)
        esc = sum(rb.escaped_routed_key(b) for b in part)  # the host framer alone decides these, and only these
        got, n_host, sid = eng.frame_responses(buf, offs, lens)
        assert sid != 0
        wf.assert_frames_equal(got, want, "call %d" % k)
        assert n_host == esc, (k, n_host, esc)
        total, listed, n_bytes = total + len(part), listed + esc, n_bytes + len(buf)
        want_all.append(want)
    assert len(bodies) % 130 not in (0,) and len(bodies) // 130 >= 2  # whole calls of 130 and a smaller one
    want = np.concatenate(want_all)
    ok = (want["status"] == abi.OK) & (want["type"] == abi.WATCH_MODIFIED)
    assert ok.sum() > 150 and (want["status"] != abi.OK).sum() > 30 and listed >= 10
    s1 = eng.response_stats()
    assert (s1["frames"] - s0["frames"], s1["host_frames"] - s0["host_frames"], s1["bytes"] - s0["bytes"]) == (
        total, listed, n_bytes)


def test_bad_spans_guards_and_empty_calls(eng):
    pod = rb.compact(rb.golden_docs()[0])
    buf = pod + b"\n" + pod
    n = len(buf)
    offs = np.array([0, n, n, n - 3, 0xFFFFFFFF, len(pod) + 1, 1 << 40, 0], np.uint64)
    lens = np.array([len(pod), 1, 0, 4, 2, len(pod), 1, n + 1], np.uint32)
    got, n_host, sid = eng.frame_responses(buf, offs, lens)
    wf.assert_frames_equal(got, frame_responses(buf, offs, lens), "bad spans")
    assert n_host == 0 and got["status"].tolist() == [0, abi.EINVAL, 0, abi.EINVAL, abi.EINVAL, 0, abi.EINVAL, abi.EINVAL]
    # len > 0xFFFFFFF0: KWOK_EINVAL before any byte is read, no stream left resident
    frames = np.zeros(1, abi.WATCH_FRAME_DTYPE)
    data = np.frombuffer(buf, np.uint8)
    nh, s2 = C.c_size_t(), C.c_uint64(5)
    rc = eng._lib.kwok_frame_responses_gpu(eng._h, data.ctypes.data, 0xFFFFFFF1, offs.ctypes.data, lens.ctypes.data, 1,
                                           frames.ctypes.data, C.byref(nh), C.byref(s2))
    assert rc == abi.EINVAL and s2.value == 0
    # n = 0 and an empty buffer: a resident stream without frames
    got, n_host, sid0 = eng.frame_responses(b"", [], [])
    assert len(got) == 0 and n_host == 0 and sid0 != 0 and sid0 != sid
    with pytest.raises(KwokError):
        eng.ingest_pods_framed(Codec(manage_all_nodes=True), sid, [0], [-1])  # the earlier stream is stale


# ---- 2. notes parity ---------------------------------------------------------------------
def body(uid, rv, raw=False):
    """a pod response whose metadata spells uid and rv (raw: JSON text inside the quotes, as given)"""
    q = (lambda s: s) if raw else (lambda s: json.dumps(s)[1:-1])
    return ('{"kind":"Pod","metadata":{"name":"p","namespace":"default","uid":"%s","resourceVersion":"%s"},"status":{}}'
            % (q(uid), q(rv))).encode()


def note_records():
    """[(body, uid text, rv text, expected status)] in call order"""
    R = []
    for k in range(600):  # three uids over three 256-thread blocks: the per-uid order decides what eight stay
        R.append(("u-%d" % (k % 3), str(5000 + k), abi.OK))
    R += [("evict", "e%d" % k, abi.OK) for k in range(9)]        # nine notes of one uid in one call
    R += [("twice", "77", abi.OK), ("twice", "77", abi.OK)]      # one rv noted twice is held twice
    R += [("empty-rv", "", abi.OK), ("", "12", abi.OK)]          # ignored
    R += [("U" * abi.UID_MAX, "1", abi.OK), ("U" * (abi.UID_MAX + 1), "1", abi.EDOMAIN)]
    R += [("rv-max", "9" * abi.RV_MAX, abi.OK), ("rv-over", "9" * (abi.RV_MAX + 1), abi.EDOMAIN)]
    return [(body(u, r), u, r, s) for u, r, s in R]


def test_notes_equal_echo_update():
    a, b, c = (Engine(make_config(**KW)) for _ in range(3))
    try:
        a.echo_enable()
        b.echo_enable()
        recs = note_records()
        bodies = [r[0] for r in recs]
        # frames that are no plain note: escaped uid / rv (EDOMAIN), a bad document, a blank one (EINVAL)
        extra = [(body("esc\\u0041", "3", raw=True), abi.EDOMAIN), (body("esc-rv", "4\\u0031", raw=True), abi.EDOMAIN),
                 (b'{"metadata":', abi.EINVAL), (b" \n", abi.EINVAL)]
        buf, offs, lens = rb.pack(bodies + [x[0] for x in extra])
        frames, n_host, sid = a.frame_responses(buf, offs, lens)
        assert n_host == 0 and frames["flags"][len(recs)] == abi.FRAME_ESC_UID and frames["flags"][len(recs) + 1] == abi.FRAME_ESC_RV
        idx = list(range(len(frames))) + [len(frames), 0xFFFFFFFF]  # ... and two indices out of range
        want = [r[3] for r in recs] + [x[1] for x in extra] + [abi.EINVAL, abi.EINVAL]
        st = a.echo_note_framed(sid, idx)
        assert st.tolist() == want
        # b: the same pairs as text, in the same order (the records a refused stay out: nothing was stored for them)
        good = [r for r in recs if r[3] == abi.OK]
        stb = b.echo_update([abi.ECHO_NOTE] * len(recs), [r[1] for r in recs], [r[2] for r in recs])
        assert stb.tolist() == [r[3] for r in recs]
        sa, sb = a.echo_stats(), b.echo_stats()
        assert sa == sb and sa["evictions"] == 3 * (200 - abi.ECHO_KEEP) + 1 and sa["live_uids"] == 3 + 4
        assert sa["notes"] == len([r for r in good if r[1] and r[2]])
        rs = a.response_stats()
        assert (rs["note_calls"], rs["notes"]) == (1, sa["notes"])
        # the probe set: every noted pair twice, pairs never noted
        probes = [(r[1], r[2]) for r in recs] * 2 + [("u-0", "1"), ("nobody", "5000"), ("evict", "e0"), ("esc-rv", "41"), ("escA", "3")]
        us, rvs = [p[0] for p in probes], [p[1] for p in probes]
        da, db = a.echo_match(us, rvs, [0] * len(probes)), b.echo_match(us, rvs, [0] * len(probes))
        assert da.tolist() == db.tolist() and 0 < da.sum() < len(probes)
        assert a.echo_stats() == b.echo_stats()
        # n = 0; a stale stream_id; the ledger not enabled
        assert len(a.echo_note_framed(sid, [])) == 0
        _f, _nh, sid2 = a.frame_responses(buf, offs, lens)
        with pytest.raises(KwokError) as err:
            a.echo_note_framed(sid, [0])
        assert err.value.code == abi.EINVAL
        assert a.echo_note_framed(sid2, [len(recs) - 2]).tolist() == [abi.OK]
        _f, _nh, sid3 = c.frame_responses(buf, offs, lens)
        with pytest.raises(KwokError) as err:
            c.echo_note_framed(sid3, [0])
        assert err.value.code == abi.EINVAL and c.response_stats()["note_calls"] == 0
    finally:
        for x in (a, b, c):
            x.close()


def test_notes_in_a_forced_table_are_refused_whole(monkeypatch):
    """KWOK_EFULL as kwok_echo_update: a table forced to 16 entries takes 15 uids; nothing of the call is stored"""
    monkeypatch.setenv("KWOK_ECHO_TAB_LOG2", "4")
    a = Engine(make_config(**KW))
    try:
        a.echo_enable()
        buf, offs, lens = rb.pack([body("full-%d" % k, "1") for k in range(20)])
        _f, _nh, sid = a.frame_responses(buf, offs, lens)
        assert not a.echo_note_framed(sid, np.arange(10)).any()
        with pytest.raises(KwokError) as err:
            a.echo_note_framed(sid, np.arange(10, 20))
        assert err.value.code == abi.EFULL and a.echo_stats()["notes"] == 10
        assert not a.echo_note_framed(sid, np.arange(10, 15)).any() and a.echo_stats()["live_uids"] == 15
    finally:
        a.close()


# ---- 3. the response buffer as the resident stream -----------------------------------------
def pod(k, **status):
    d = {"apiVersion": "v1", "kind": "Pod",
         "metadata": {"name": "pod-%d" % k, "namespace": "default", "uid": "u-pod-%d" % k, "resourceVersion": str(100 + k),
                      "creationTimestamp": "2024-01-01T00:00:00Z"},
         "spec": {"nodeName": "node-%d" % (k % 3), "containers": [{"name": "c", "image": "img"}]}, "status": status}
    return json.dumps(d, separators=(",", ":")).encode()


def test_framed_ingest_runs_on_response_frames():
    codec = Codec(manage_all_nodes=True)
    a, b = Engine(make_config(**KW)), Engine(make_config(**KW))
    try:
        nodes = b"".join(wf.wrap(json.dumps({"apiVersion": "v1", "kind": "Node", "metadata": {"name": "node-%d" % k, "uid": "n%d" % k},
                                              "spec": {}, "status": {}}).encode(), "ADDED") for k in range(3))
        adds = b"".join(wf.wrap(pod(k), "ADDED") for k in range(40))
        for x in (a, b):
            x.uid_dir_enable()
            x.register_pod_spec([("c", "img")], [], [])
            f, _u, _nh, sid = x.frame_watch(nodes)
            assert not x.ingest_nodes_framed(codec, sid, np.arange(len(f)))[1].any()
            f, _u, _nh, sid = x.frame_watch(adds)
            assert not x.ingest_pods_framed_uid(codec, sid, np.arange(len(f)))[1].any()
            x.tick(1704067230, read=False)
        # the responses of the tick's patches: the pods as patched (a phase, addresses), some without a podIP
        mods = [pod(k, **({"phase": "Running", "hostIP": "196.168.0.1", "podIP": "10.0.%d.%d" % (k // 200, 2 + k % 200)} if k % 4
                          else {"phase": "Running"})) for k in range(40)]
        mods.append(pod(99, phase="Pending"))  # a pod the engine does not hold: created, as a MODIFIED watch event would
        buf, offs, lens = rb.pack(mods, gap=b"\n")
        fa, nh, sa = a.frame_responses(buf, offs, lens)
        stream = b"".join(wf.wrap(m) for m in mods)
        fb, _u, _nhb, sb = b.frame_watch(stream)
        assert nh == 0 and (fa["type"] == abi.WATCH_MODIFIED).all() and len(fa) == len(fb)
        order = np.arange(len(mods))[::-1].copy()  # (any order: the frames are addressed by index)
        ra = a.ingest_pods_framed_uid(codec, sa, order)
        rbb = b.ingest_pods_framed_uid(codec, sb, order)
        for x, y in zip(ra, rbb):
            assert np.array_equal(x, y)
        assert not ra[1].any() and (ra[0] >= 0).all()
        n_slots = KW["buckets"] * KW["pod_slots_per_bucket"]
        for now in (1704067260, 1704067290):
            oa, ob = a.tick(now), b.tick(now)
            assert list(oa.heartbeat_nodes) == list(ob.heartbeat_nodes)
            assert oa.node_inits == ob.node_inits and oa.pod_patches == ob.pod_patches and oa.deletes == ob.deletes
            assert oa.counters == ob.counters
            for p, q in zip(a.dump_pods(0, n_slots), b.dump_pods(0, n_slots)):
                assert (p == q).all()
        assert a.uid_lookup(["u-pod-%d" % k for k in (0, 7, 99)]).tolist() == b.uid_lookup(["u-pod-%d" % k for k in (0, 7, 99)]).tolist()
        # a watch framing afterwards replaces the response stream
        _f, _u, _nh, sw = a.frame_watch(wf.wrap(pod(3)))
        assert sw != sa
        with pytest.raises(KwokError) as err:
            a.ingest_pods_framed_uid(codec, sa, [0])
        assert err.value.code == abi.EINVAL
        ws = a.watch_stats()
        assert ws["frames"] == 3 + 40 + 1  # the response frames are counted by kwok_response_stats alone
        assert a.response_stats()["frames"] == len(mods)
    finally:
        a.close()
        b.close()
        codec.close()
