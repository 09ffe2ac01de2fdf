"""GPU: the List body framer on the device (kwok_frame_list_gpu: json.hip
k_list_quotes / k_list_pick / k_list_split / k_list_range / k_list_parse with
k_frame_scan between them) against the host framer (kwok_frame_list, codec.cpp),
record for record and info for info, and the framed ingests over a resident
body against kwok_ingest_*_json over the same documents.
  (a) the named cases of list_bodies.py and every prefix of one body, with the
      items the host framed and the bodies it framed whole asserted per case
  (b) boundary sweeps of the split: quotes, backslash runs of 1..5, braces and
      the items `[` on every residue mod 16 and on both sides of a wave step, a
      block step and a tile; a string of brackets longer than two tiles; an item
      over three tiles; five opens to a window; lengths 2..2 tiles + 5
  (c) one body of more tiles than a scan step covers (~22 MiB: four huge items, 18k small)
  (d) 4k fuzzed items (test_json_fuzz_gpu.py's mutators) packed into lists
  (e) 1.5k byte-mutated and truncated bodies; a failed call leaves no stream
  (f) every golden trace's starting fleet as a NodeList and a PodList
Reference: pod_controller.go:357-368, node_controller.go:282-296."""
import json
import random

import numpy as np
import pytest

import harness
import list_bodies as lb
import watch_frames as wf
from harness import DISREGARD, MANAGE, node_doc, pod_doc
from kwok_amd import abi
from kwok_amd.codec import Codec, frame_list
from kwok_amd.engine import Engine, KwokError, make_config
from test_json_fuzz_gpu import dup_first, escape_some, golden_nodes, golden_pods, mutate

pytestmark = pytest.mark.gpu

TILE = abi.WATCH_TILE


@pytest.fixture(scope="module")
def eng():
    e = Engine(make_config(buckets=64, node_slots_per_bucket=16, pod_slots_per_bucket=128))
    yield e
    e.close()


def host(body):
    try:
        frames, info = frame_list(body)
    except KwokError as err:
        assert err.code == abi.EINVAL
        return abi.EINVAL, None, None
    return abi.OK, frames, lb.info_dict(info)


def compare(e, body, want_host=None, want_whole=None, where=""):
    """the device's status, frames and info == the host framer's; returns (status, frames)"""
    want_st, want, want_info = host(body)
    before = e.list_stats()
    try:
        got, info, n_host, sid = e.frame_list(body)
        st = abi.OK
    except KwokError as err:
        assert err.code == abi.EINVAL and err.n_frames == 0, (where, err)
        st, got, n_host, sid = abi.EINVAL, None, 0, 0
    after = e.list_stats()
    assert st == want_st, (where, st, want_st)
    assert after["bodies"] - before["bodies"] == 1 and after["body_bytes"] - before["body_bytes"] == len(body)
    if st == abi.OK:
        assert sid != 0
        wf.assert_frames_equal(got, want, where)
        assert lb.info_dict(info) == want_info, where
        assert after["items"] - before["items"] == len(got) and after["host_items"] - before["host_items"] == n_host
    if want_host is not None:
        assert n_host == want_host, (where, n_host, want_host)
    if want_whole is not None:
        assert after["host_bodies"] - before["host_bodies"] == want_whole, (where, want_whole)
    return st, got


# ---- (a) ---------------------------------------------------------------------
def test_named_cases_equal_the_host_framer(eng):
    n_ok = 0
    for name, (body, n_host, whole) in lb.cases().items():
        st, _ = compare(eng, body, n_host, whole, name)
        n_ok += st == abi.OK
    assert 25 <= n_ok <= len(lb.cases()) - 15  # neither outcome is rare


def test_every_prefix_equals_the_host_framer(eng):
    body = lb.PREFIX_BODY
    for k in range(1, len(body)):
        st, _ = compare(eng, body[:k], 0, None, "prefix %d" % k)
        assert st == abi.EINVAL
    st, got = compare(eng, body, 0, 0, "the whole body")
    assert st == abi.OK and len(got) == 2


def test_cap_and_length_guard(eng):
    import ctypes as C
    body = lb.cases()["pod_list"][0]
    buf = np.frombuffer(body, np.uint8)
    frames = np.zeros(8, abi.WATCH_FRAME_DTYPE)
    nf, nh, sid, info = C.c_size_t(), C.c_size_t(), C.c_uint64(), abi.ListInfo()
    call = lambda n, cap: eng._lib.kwok_frame_list_gpu(eng._h, buf.ctypes.data, n, frames.ctypes.data, cap, C.byref(nf),
                                                       C.byref(info), C.byref(nh), C.byref(sid))
    assert call(len(body), 2) == abi.EINVAL and nf.value == 3 and sid.value == 0 and info.kind.len == 0
    assert call(1 << 32, 8) == abi.EINVAL and nf.value == 0  # (before any byte is read)
    assert call(len(body), 3) == 0 and nf.value == 3 and sid.value != 0 and info.kind.len == 7
    bad = np.frombuffer(lb.cases()["item_then_number"][0], np.uint8)  # judged before cap is, as the host does
    assert eng._lib.kwok_frame_list_gpu(eng._h, bad.ctypes.data, len(bad), frames.ctypes.data, 0, C.byref(nf), C.byref(info),
                                        C.byref(nh), C.byref(sid)) == abi.EINVAL and nf.value == 0 and sid.value == 0


# ---- (b) ---------------------------------------------------------------------
def test_split_boundaries(eng):
    bodies = lb.sweep_bodies()
    assert 150 <= len(bodies) <= 400
    for k, b in enumerate(bodies):
        st, got = compare(eng, b, 0, 0, "sweep %d (%d bytes)" % (k, len(b)))
        assert st == abi.OK and len(got) >= 1, k
    st, got = compare(eng, b"{}", 0, 1, "length 2")  # (no array under the root: the host's)
    assert st == abi.OK and len(got) == 0


# ---- (c) ---------------------------------------------------------------------
def test_more_tiles_than_one_scan_step(eng):
    huge = lambda k: (b'{"metadata":{"uid":"huge-%d"},"blob":"' % k + b'}{[]\\"\\\\' * (4 * 1024 * 1024 // 8) +
                      b'","deep":{"a":[{"b":{}}]}}')
    small = [lb.pod(k) for k in range(18000)]
    items = [huge(0)] + small[:9000] + [huge(1), huge(2)] + small[9000:] + [huge(3)]
    body = lb.body_of(items, sep=b",\n")
    n_tiles = (len(body) + TILE - 1) // TILE
    assert n_tiles > abi.WATCH_SCAN_TILES and n_tiles % abi.WATCH_SCAN_TILES  # several scan steps, the last one partial
    assert len(body) < 24 << 20
    st, got = compare(eng, body, 0, 0, "big body")
    assert st == abi.OK and len(got) == 18004
    r = got[-1]
    assert body[r["uid"]["off"]:r["uid"]["off"] + r["uid"]["len"]] == b"huge-3"
    r = got[-2]
    assert body[r["name"]["off"]:r["name"]["off"] + r["name"]["len"]] == b"pod-17999"


# ---- (d) ---------------------------------------------------------------------
def fuzz_bodies(n, seed):
    rng = random.Random(seed)
    docs = golden_pods() + golden_nodes()
    for d in docs:
        d["metadata"].setdefault("uid", "u-" + d["metadata"]["name"])
        d["metadata"]["resourceVersion"] = str(rng.randint(1, 10 ** 6))
    ws = lambda: rng.choice(["", "", " ", "\n", " \t\r\n", "  "])
    bodies, left = [], n
    while left:
        k = min(left, rng.choice([1, 2, 3, 5, 17, 40, 100, 300]))
        left -= k
        texts = []
        for _ in range(k):
            text = json.dumps(mutate(rng.choice(docs), rng), indent=rng.choice([None, None, 1]), ensure_ascii=rng.random() < 0.5)
            r = rng.random()
            if r < 0.15:
                text = dup_first(text, rng)
            elif r < 0.3:
                text = escape_some(text, rng)
            texts.append(text)
        head = '{%s"kind":"PodList",%s"metadata":{"resourceVersion":"%d"},%s"items"%s:%s[%s' % (
            ws(), ws(), rng.randint(1, 9999), ws(), ws(), ws(), ws())
        bodies.append((head + (ws() + "," + ws()).join(texts) + ws() + "]" + ws() + "}" + ws()).encode())
    return bodies


def test_fuzzed_items(eng):
    bodies = fuzz_bodies(4000, 78)
    before = eng.list_stats()
    n_items = n_host = n_ok = 0
    for k, b in enumerate(bodies):
        want_st, want, _ = host(b)
        st, got = compare(eng, b, None, 0, "fuzzed body %d" % k)
        if st == abi.OK:
            n_ok += 1
            n_items += len(got)
    after = eng.list_stats()
    assert after["host_bodies"] == before["host_bodies"]
    assert n_ok >= len(bodies) // 2 and n_items >= 1500, (n_ok, len(bodies), n_items)
    n_host = after["host_items"] - before["host_items"]
    assert 0 < n_host < n_items // 4  # the escaped routed keys, and only items like them


# ---- (e) ---------------------------------------------------------------------
def test_byte_mutated_bodies(eng):
    codec = Codec(manage_all_nodes=True)
    bodies = lb.mutated_bodies(1500, 5)
    n_bad = 0
    for k, b in enumerate(bodies):
        st, _ = compare(eng, b, None, None, "mutated body %d" % k)
        if st != abi.OK:
            n_bad += 1
            if n_bad % 50 == 1:  # a failed call leaves no stream resident: no id can name one
                for sid in (0, 1, 2 ** 40):
                    with pytest.raises(KwokError) as ei:
                        eng.ingest_pods_framed(codec, sid, np.array([0], np.uint32), np.array([-1], np.int32))
                    assert ei.value.code == abi.EINVAL
    assert 300 <= n_bad <= 1300, n_bad


def test_failed_call_leaves_no_stream(eng):
    codec = Codec(manage_all_nodes=True)
    good = lb.cases()["pod_list"][0]
    _f, _i, _n, sid = eng.frame_list(good)
    with pytest.raises(KwokError):
        eng.frame_list(good[:-1])
    for s in (sid, sid + 1, 0):  # (neither the replaced body's id nor the one the failed call would have had)
        with pytest.raises(KwokError) as ei:
            eng.ingest_pods_framed(codec, s, np.array([0], np.uint32), np.array([-1], np.int32))
        assert ei.value.code == abi.EINVAL
        with pytest.raises(KwokError) as ei:
            eng.ingest_nodes_framed(codec, s, np.array([0], np.uint32))
        assert ei.value.code == abi.EINVAL


# ---- (f) ---------------------------------------------------------------------
@pytest.mark.parametrize("name", harness.TRACES)
def test_golden_fleet_as_lists(name):
    """the first tick's node and pod events - the fleet that exists at Start - as
    a NodeList and a PodList: framed, ingested from the resident bodies; a twin
    engine takes the same documents through kwok_ingest_*_json; handles, statuses
    and the tick's outputs are identical"""
    fx = harness.load_trace(name)
    e, twin = Engine(harness.config_for(fx)), Engine(harness.config_for(fx))
    codec = Codec(manage_all_nodes=False, manage_nodes_with_annotation_selector=MANAGE,
                  disregard_status_with_annotation_selector=DISREGARD)
    t = fx["ticks"][0]
    nev = [ev for ev in t["node_events"]]
    pev = [ev for ev in t["pod_events"]]
    assert all(ev["op"] != "delete" for ev in nev + pev), "the first tick adds the fleet"
    ndocs = [json.dumps(node_doc(ev)).encode() for ev in nev]
    pdocs = [json.dumps(pod_doc(ev)).encode() for ev in pev]
    up = lambda n: np.full(n, abi.OP_UPSERT, np.uint8)
    if ndocs:
        frames, info, n_host, sid = e.frame_list(lb.body_of(ndocs, kind="NodeList", rv="10"))
        assert len(frames) == len(ndocs) and n_host == 0
        hs, st, _nh = e.ingest_nodes_framed(codec, sid, np.arange(len(ndocs)))
        arena, offs, lens = Engine._docs(ndocs)
        hs2, st2, _ = twin.ingest_nodes_json(codec, arena, offs, lens, up(len(ndocs)))
        assert list(st) == list(st2) == [0] * len(ndocs)
        assert list(hs) == list(hs2)
    if pdocs:
        body = lb.body_of(pdocs, rv="11", cont="next")
        frames, info, n_host, sid = e.frame_list(body)
        assert len(frames) == len(pdocs) and n_host == 0 and body[info.continue_.off:][:info.continue_.len] == b"next"
        handles = np.array([ev.get("handle", -1) for ev in pev], np.int32)
        hs, st, rel, _nh = e.ingest_pods_framed(codec, sid, np.arange(len(pdocs)), handles)
        arena, offs, lens = Engine._docs(pdocs)
        hs2, st2, rel2, _ = twin.ingest_pods_json(codec, arena, offs, lens, up(len(pdocs)), handles)
        assert list(st) == list(st2) == [0] * len(pdocs)
        assert list(hs) == list(hs2) == [ev["expect_handle"] for ev in pev]
        assert list(rel) == list(rel2)
    out, out2 = e.tick(t["now"]), twin.tick(t["now"])
    harness.compare_tick(fx["name"], 0, t["expect"], out)
    harness.compare_tick(fx["name"], 0, t["expect"], out2)
    e.close()
    twin.close()


def test_two_runs_upload_the_body_once(eng):
    codec = Codec(manage_all_nodes=True)
    ev = dict(node="node-0", disregard=False, deleting=False, finalizers=0, creation=1704067140, phase="Pending",
              status_nonempty=False, conforms=False, hostIP="", podIP="",
              spec={"containers": [["c", "img"]], "init": [], "gates": []})
    body = lb.body_of([json.dumps(pod_doc(dict(ev, key="lpod-%d" % k))).encode() for k in range(40)])
    before, wbefore = eng.list_stats(), eng.watch_stats()
    frames, _info, _nh, sid = eng.frame_list(body)
    assert (frames["type"] == abi.WATCH_ADDED).all() and (frames["line_off"] == frames["doc_off"]).all()
    h1, s1, _r, _ = eng.ingest_pods_framed(codec, sid, np.arange(0, 25), np.full(25, -1, np.int32))
    h2, s2, _r, _ = eng.ingest_pods_framed(codec, sid, np.arange(25, 40), np.full(15, -1, np.int32))
    after, wafter = eng.list_stats(), eng.watch_stats()
    assert not s1.any() and not s2.any() and len(set(h1) | set(h2)) == 40
    assert after["body_bytes"] - before["body_bytes"] == len(body) and after["bodies"] - before["bodies"] == 1
    assert after["items"] - before["items"] == 40 and after["host_items"] == before["host_items"]
    assert wafter["stream_bytes"] == wbefore["stream_bytes"] and wafter["framed_ingests"] - wbefore["framed_ingests"] == 2
    # a watch stream replaces the body, a body the watch stream
    _f, _u, _n, wsid = eng.frame_watch(wf.wrap(wf.POD, "ADDED"))
    assert wsid != sid
    with pytest.raises(KwokError):
        eng.ingest_pods_framed(codec, sid, np.arange(0, 1), np.full(1, -1, np.int32))
