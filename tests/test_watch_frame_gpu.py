"""GPU: the watch-stream framer on the device (kwok_frame_watch_gpu: json.hip
k_frame_count / k_frame_scan / k_frame_emit / k_frame_parse) against the host
framer (kwok_frame_watch, codec.cpp), record for record and byte for byte, and
the framed ingests (kwok_ingest_pods_framed / kwok_ingest_nodes_framed) against
kwok_ingest_pods_json / kwok_ingest_nodes_json over the same documents.
  (a) the cases of test_watch_frame_cpu.py; the lines with an escaped type or
      routed key are the host's (n_host)
  (b) boundary sweeps of the line split: newlines on every residue mod 16, on
      both sides of a 1024-byte wave step, a block step and a tile; total lengths
      0, 1, 15, 16, 17, tile +- 1, 2 tiles + 5
  (c) one stream of more tiles than a scan step covers (~100 lines of 1 MiB)
  (d) 8k fuzzed frames: the golden documents mutated as JSON values
      (test_json_fuzz_gpu.py's mutators) inside mutated envelopes
Then every golden trace as watch streams through the framer and the framed
ingests, the stream uploaded once for a batch ingested in two runs, and the
rejections (a stale stream_id, BOOKMARK, a bad frame: a status, nothing applied).
Reference: pod_controller.go:272-343, node_controller.go:225-279."""
import json
import random

import numpy as np
import pytest

import harness
import watch_frames as wf
from harness import DISREGARD, MANAGE, node_doc, pod_doc
from kwok_amd import abi
from kwok_amd.codec import Codec, frame_watch
from kwok_amd.engine import Engine, KwokError, make_config
from test_json_fuzz_gpu import dup_first, escape_some, golden_nodes, golden_pods, mutate, rand_value

pytestmark = pytest.mark.gpu

TILE = abi.WATCH_TILE


@pytest.fixture(scope="module")
def eng():
    e = Engine(make_config(buckets=64, node_slots_per_bucket=16, pod_slots_per_bucket=128))
    yield e
    e.close()


def compare(e, stream, want_host=None, where=""):
    """the device's frames == the host framer's; returns them"""
    want, consumed = frame_watch(stream)
    got, used, n_host, sid = e.frame_watch(stream)
    assert used == consumed, (where, used, consumed)
    assert sid != 0
    wf.assert_frames_equal(got, want, where)
    if want_host is not None:
        assert n_host == want_host, (where, n_host, want_host)
    return got


# ---- (a) ---------------------------------------------------------------------
def test_cpu_cases_equal_the_host_framer(eng):
    for name, (stream, n_host) in wf.cases().items():
        compare(eng, stream, n_host, name)
    stream, n_host = wf.stream_of_cases()
    f = compare(eng, stream, n_host, "all cases in one stream")
    assert (f["status"] == 0).sum() > 20 and (f["status"] != 0).sum() > 10


def test_cap_and_length_guard(eng):
    import ctypes as C
    s, _ = wf.cases()["all_types"]
    buf = np.frombuffer(s, np.uint8)
    frames = np.zeros(8, abi.WATCH_FRAME_DTYPE)
    nf, used, nh, sid = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_uint64()
    call = lambda n, cap: eng._lib.kwok_frame_watch_gpu(eng._h, buf.ctypes.data, n, frames.ctypes.data, cap, C.byref(nf),
                                                        C.byref(used), C.byref(nh), C.byref(sid))
    assert call(len(s), 4) == abi.EINVAL and nf.value == 5 and sid.value == 0
    assert call(1 << 32, 8) == abi.EINVAL and nf.value == 0  # (before any byte is read)
    assert call(len(s), 5) == 0 and nf.value == 5 and sid.value != 0


# ---- (b) ---------------------------------------------------------------------
def line(n, rng):
    """one line of exactly n bytes, newline included: a frame when it fits, else blanks or garbage"""
    small = b'{"type":"ADDED","object":{"metadata":{"name":"x"}}}\n'
    if n >= len(small):
        return small[:25] + b" " * (n - len(small)) + small[25:]
    return (b" " if rng.random() < 0.5 else b"x") * (n - 1) + b"\n"


def sweep_streams():
    rng = random.Random(11)
    out = []
    for s in range(16):  # newlines on every residue mod 16, from every starting residue
        out.append(b"".join([line(s + 1, rng)] + [line(60 + k, rng) for k in range(17)]))
    for edge in (16, 1024, 2048, 4096, TILE, 2 * TILE):  # a window, a wave step, a block step, a tile
        for d in (-2, -1, 0, 1):
            p = edge + d  # a newline at offset p ...
            out.append(line(p + 1, rng) + line(70, rng) + b"tail")
            out.append(line(p, rng) + b"\n" + line(70, rng))        # ... after another newline (a blank line)
            out.append(line(max(1, p - 80), rng) + line(81, rng) + line(TILE + 3, rng))
    for total in (0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 5):
        for tail in (0, 1, 7):
            s, left = b"", total - min(tail, total)
            while left:
                n = min(left, rng.choice([1, 2, 55, 64, 100])) if left > 120 else left
                s += line(n, rng)
                left -= n
            s += b"t" * min(tail, total)
            assert len(s) == total
            out.append(s)
    for _ in range(150):  # random line lengths over up to three tiles
        s = b"".join(line(rng.choice([1, 2, 15, 16, 17, rng.randint(1, 400), rng.randint(1, 3000)]), rng)
                     for _ in range(rng.randint(1, 60)))
        out.append(s[:3 * TILE] + (b"" if rng.random() < 0.5 else b"\n"))
    out.append(b"x" * (2 * TILE + 5))  # zero newlines
    out.append(b"\n" * (TILE + 17))    # nothing but newlines
    return out


def test_line_split_boundaries(eng):
    streams = sweep_streams()
    assert 200 <= len(streams) <= 400
    for k, s in enumerate(streams):
        got = compare(eng, s, 0, "sweep %d (%d bytes)" % (k, len(s)))
        assert len(got) == s.count(b"\n")


# ---- (c) ---------------------------------------------------------------------
def test_more_tiles_than_one_scan_step(eng):
    pad = b" " * (1 << 20)
    parts = []
    for k in range(100):
        parts.append(b'{"type":"MODIFIED",' + pad[:len(pad) // 2] + b'"object":{"metadata":{"name":"big-%d",' % k +
                     pad[:len(pad) // 2] + b'"uid":"u-%d"},"spec":{}}}\n' % k)
        parts.append(wf.wrap(wf.POD, "ADDED") if k % 3 else b"\r\n")
    stream = b"".join(parts)
    n_tiles = (len(stream) + TILE - 1) // TILE
    assert n_tiles > abi.WATCH_SCAN_TILES and n_tiles % abi.WATCH_SCAN_TILES  # several scan steps, the last one partial
    got = compare(eng, stream, 0, "big stream")
    assert len(got) == 200 and not got["status"].any()
    r = got[198]
    assert stream[r["name"]["off"]:r["name"]["off"] + r["name"]["len"]] == b"big-99"


# ---- (d) ---------------------------------------------------------------------
def envelope(doc, rng):
    """one watch line around a document's text, the envelope mutated too"""
    typ = rng.choice(["ADDED", "MODIFIED", "DELETED", "MODIFIED", "ADDED", "BOOKMARK", "ERROR"])
    t, o = '"type":"%s"' % typ, '"object":' + doc
    r = rng.random()
    if r < 0.45:
        body = "{%s,%s}" % (t, o)
    elif r < 0.55:
        body = "{ %s ,\t%s }\r" % (o, t)                        # object first, inner whitespace
    elif r < 0.62:
        body = rng.choice(['{%s,"type":"BOGUS",%s}', '{%s,%s,"object":[1]}', '{"type":7,%s,%s}',
                           '{"object":null,%s,%s}']) % (t, o)    # a repeated key: the first wins
    elif r < 0.70:
        body = rng.choice(['{"ty\\u0070e":"%s",%s}' % (typ, o), '{%s,"\\u006fbject":%s}' % (t, doc),
                           '{"type":"%s\\u0044",%s}' % (typ[:-1], o), '{%s,"x\\u0041":1,%s}' % (t, o)])
    elif r < 0.76:
        body = '{"type":%s,%s}' % (json.dumps(rng.choice(["added", "", "PATCH", 1, None, ["ADDED"]])), o)
    elif r < 0.82:
        body = '{%s,"object":%s}' % (t, json.dumps(rand_value(rng)))
    elif r < 0.88:
        body = "{%s,%s}" % (t, o)
        body = body[:rng.randrange(1, len(body))]               # cut short
    elif r < 0.93:
        body = rng.choice(["{%s}" % t, "{%s}" % o, "[{%s,%s}]" % (t, o), "{%s,%s} x" % (t, o), ""])
    else:
        body = '{"kind":"x",%s,"extra":{"object":{"metadata":{"uid":"no"}}},%s}' % (t, o)
    return body.encode() + b"\n"


def fuzz_stream(n, seed):
    rng = random.Random(seed)
    docs = golden_pods() + golden_nodes()
    for d in docs:
        d["metadata"].setdefault("uid", "u-" + d["metadata"]["name"])
        d["metadata"]["resourceVersion"] = str(rng.randint(1, 10 ** 6))
    lines = []
    for _ in range(n):
        d = mutate(rng.choice(docs), rng)
        text = json.dumps(d, indent=rng.choice([None, None, 1]), ensure_ascii=rng.random() < 0.5).replace("\n", " ")
        r = rng.random()
        if r < 0.15:
            text = dup_first(text, rng).replace("\n", " ")
        elif r < 0.3:
            text = escape_some(text, rng)
        lines.append(envelope(text, rng))
    return b"".join(lines)


def test_fuzzed_frames(eng):
    stream = fuzz_stream(8000, 77)
    want, _ = frame_watch(stream)
    assert len(want) == 8000
    ok = (want["status"] == 0) & (want["type"] != abi.WATCH_NONE)
    bad = want["status"] != 0
    assert ok.mean() >= 0.4 and bad.mean() >= 0.1, (ok.mean(), bad.mean())  # neither outcome is rare
    got, used, n_host, _sid = eng.frame_watch(stream)
    assert used == len(stream)
    assert (got["status"] == want["status"]).all()
    wf.assert_frames_equal(got, want, "fuzzed frames")
    assert 100 < n_host < 2000  # the escaped routed keys, and only lines like them


# ---- end to end ----------------------------------------------------------------
def _typ(ev, seen):
    if ev["op"] == "delete":
        return "DELETED"
    return "MODIFIED" if seen else "ADDED"


@pytest.mark.parametrize("name", harness.TRACES)
def test_golden_trace_as_watch_streams(name):
    """per tick one stream holding the node watch's lines and the pod watch's:
    framed once, ingested by kwok_ingest_nodes_framed and kwok_ingest_pods_framed;
    handles and statuses equal kwok_ingest_*_json's over the same documents (a twin
    engine), every tick's outputs equal the fixture"""
    fx = harness.load_trace(name)
    e, twin = Engine(harness.config_for(fx)), Engine(harness.config_for(fx))
    codec = Codec(manage_all_nodes=False, manage_nodes_with_annotation_selector=MANAGE,
                  disregard_status_with_annotation_selector=DISREGARD)
    last, seen = {}, set()
    for ti, t in enumerate(fx["ticks"]):
        ndocs, lines = [], []
        for ev in t["node_events"]:
            if ev["op"] == "delete":
                d = last.get(ev["name"]) or {"metadata": {"name": ev["name"]}}
            else:
                d = last[ev["name"]] = node_doc(ev)
            ndocs.append(json.dumps(d).encode())
            lines.append(wf.wrap(ndocs[-1], _typ(ev, ev["name"] in seen)))
            seen.add(ev["name"])
        lines.append(b'{"type":"BOOKMARK","object":{"kind":"Node","metadata":{"resourceVersion":"9"}}}\n')
        pdocs = [json.dumps(pod_doc(ev)).encode() for ev in t["pod_events"]]
        lines += [wf.wrap(d, _typ(ev, ev.get("handle", -1) >= 0)) for d, ev in zip(pdocs, t["pod_events"])]
        stream = b"".join(lines)
        frames, used, n_host, sid = e.frame_watch(stream)
        assert used == len(stream) and n_host == 0 and not frames["status"].any()
        nn, npod = len(ndocs), len(pdocs)
        ops = lambda evs: np.array([abi.OP_DELETE if ev["op"] == "delete" else abi.OP_UPSERT for ev in evs], np.uint8)
        if nn:
            hs, st, _nh = e.ingest_nodes_framed(codec, sid, np.arange(nn))
            arena, offs, lens = Engine._docs(ndocs)
            hs2, st2, _ = twin.ingest_nodes_json(codec, arena, offs, lens, ops(t["node_events"]))
            assert list(st) == list(st2) == [0] * nn, (ti, list(st))
            assert list(hs) == list(hs2), ti
        if npod:
            handles = np.array([ev.get("handle", -1) for ev in t["pod_events"]], np.int32)
            hs, st, rel, _nh = e.ingest_pods_framed(codec, sid, np.arange(nn + 1, nn + 1 + npod), handles)
            arena, offs, lens = Engine._docs(pdocs)
            hs2, st2, rel2, _ = twin.ingest_pods_json(codec, arena, offs, lens, ops(t["pod_events"]), handles)
            assert list(st) == list(st2) == [0] * npod, (ti, list(st))
            assert list(hs) == list(hs2) == [ev["expect_handle"] for ev in t["pod_events"]], ti
            assert list(rel) == list(rel2), ti
        harness.compare_tick(fx["name"], ti, t["expect"], e.tick(t["now"]))
        twin.tick(t["now"])
    e.close()
    twin.close()


def _pod_lines(n, first=0):
    ev = dict(node="node-0", disregard=False, deleting=False, finalizers=0, creation=1704067140, phase="Pending",
              status_nonempty=False, conforms=False, hostIP="", podIP="",
              spec={"containers": [["c", "img"]], "init": [], "gates": []})
    return [wf.wrap(pod_doc(dict(ev, key="pod-%d" % k)), "ADDED") for k in range(first, first + n)]


def test_two_runs_upload_the_stream_once(eng):
    codec = Codec(manage_all_nodes=True)
    stream = b"".join(_pod_lines(40))
    before = eng.watch_stats()
    frames, _used, _nh, sid = eng.frame_watch(stream)
    h1, s1, _r, _ = eng.ingest_pods_framed(codec, sid, np.arange(0, 25), np.full(25, -1, np.int32))
    h2, s2, _r, _ = eng.ingest_pods_framed(codec, sid, np.arange(25, 40), np.full(15, -1, np.int32))
    after = eng.watch_stats()
    assert not s1.any() and not s2.any() and len(set(h1) | set(h2)) == 40
    assert after["stream_bytes"] - before["stream_bytes"] == len(stream)
    assert after["framed_ingests"] - before["framed_ingests"] == 2
    assert after["frames"] - before["frames"] == 40 and after["host_frames"] == before["host_frames"]
    # (the same frames again as MODIFIED of the known pods: still no upload)
    h3, s3, _r, _ = eng.ingest_pods_framed(codec, sid, np.arange(0, 25), h1)
    assert not s3.any() and list(h3) == list(h1)
    assert eng.watch_stats()["stream_bytes"] == after["stream_bytes"]


def test_rejections_are_statuses(eng):
    codec = Codec(manage_all_nodes=True)
    used0 = int(eng.dump_pods(0, 64 * 128)[0].sum())
    lines = _pod_lines(3, first=1000)
    stream = (lines[0] + b'{"type":"BOOKMARK","object":{"metadata":{"resourceVersion":"5"}}}\n' +
              b'{"type":"ADDED","object":[]}\n' + b"\r\n" + lines[1] +
              b'{"type":"ERROR","object":{"kind":"Status","code":410}}\n' + lines[2])
    frames, _used, _nh, sid = eng.frame_watch(stream)
    assert list(frames["status"]) == [0, 0, abi.EINVAL, 0, 0, 0, 0]
    idx = np.array([0, 1, 2, 3, 4, 5, 6, 7, 4000000000], np.uint32)  # (7 and the last: no such frame)
    hs, st, _rel, _ = eng.ingest_pods_framed(codec, sid, idx, np.full(len(idx), -1, np.int32))
    E = abi.EINVAL
    assert list(st) == [0, E, E, E, 0, E, 0, E, E]
    assert int(eng.dump_pods(0, 64 * 128)[0].sum()) == used0 + 3
    hs, st, _ = eng.ingest_nodes_framed(codec, sid, np.array([1, 2, 3, 5, 9], np.uint32))
    assert list(st) == [E] * 5 and eng.node_size() == 0
    stale = sid
    _f, _u, _n, sid2 = eng.frame_watch(lines[0])
    assert sid2 != stale
    for bad in (stale, 0, sid2 + 1):
        with pytest.raises(KwokError) as ei:
            eng.ingest_pods_framed(codec, bad, np.array([0], np.uint32), np.array([-1], np.int32))
        assert ei.value.code == abi.EINVAL
        with pytest.raises(KwokError) as ei:
            eng.ingest_nodes_framed(codec, bad, np.array([0], np.uint32))
        assert ei.value.code == abi.EINVAL
    assert int(eng.dump_pods(0, 64 * 128)[0].sum()) == used0 + 3
