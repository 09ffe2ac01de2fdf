"""GPU: time values at the edges of the supported domain,
through the device's parser (json.hip jtime), its formatter (kernels.hip
format_ts: build_hb_template, hb_fill_delta, emit_phase1, emit_job_tab, the fused
emission of k_pod_jobs) and the 32-bit word a creation time travels in between
(S.pod_ctime, kwok_pod_rec.creation, kwok_pod_rec12.value).  The domain is
0 <= t <= 2^32 - 1, 1970-01-01T00:00:00Z to 2106-02-07T06:28:15Z.

Everything is bit-exact.  Python's datetime / calendar.timegm is the yardstick
(tests/test_time_cpu.py builds every document and constant from it, and runs
the host codec and the oracle over the same values); where patch bytes are
compared, the oracle is the yardstick as well.  Every case asserts that it took
the path it names: n_host == 0, a patch count, ticks_hb_delta,
ticks_once_stream.

 1. device parse: the CPU file's documents, accepted and rejected, four renderings
 2. round trip: a document's creationTimestamp text comes back in its pod's patch
 3. every emission path over creation times of the whole domain, clocks at its end
 4. the 32-bit word in kwok_pod_rec / kwok_pod_rec12: a creation time is no podIP
 5. clocks: the delta heartbeat stream over pairs of clocks that differ in one
    position, in almost all, and at the domain's edges; the times refused"""
import json
from datetime import datetime

import numpy as np
import pytest

import test_hb_delta_gpu as hbd
import test_once_stream_gpu as ons
import watch_frames as wf
from gpu_common import EMIT_PATHS, Driver, compare, compare_state, compare_tick, new_pods
from kwok_amd import abi, engine
from kwok_amd.codec import Codec
from kwok_amd.engine import Engine, KwokError, make_config
from oracle.oracle import Oracle
from test_json_gpu import compare as compare_with_host
from test_time_cpu import (LAST, ORDER, PROBE, SPEC, accepted, at, far, patch_times, pod_document, rejected, rfc3339, secs,
                           stamp)

pytestmark = pytest.mark.gpu

KW = dict(cidr="10.0.0.1/16", node_ip="196.168.0.1", buckets=64, node_slots_per_bucket=16, pod_slots_per_bucket=128)
N_SLOTS = 64 * 128

# the seconds on both sides of everything a 32-bit word or a civil date can get wrong: built
# from datetime, and their properties asserted, in tests/test_time_cpu.py
EDGES = PROBE


def node_events(n):
    ar = abi.Arena()
    ev = np.zeros(n, abi.NODE_EVENT_DTYPE)
    ev["op"], ev["managed"], ev["lockable"] = abi.OP_UPSERT, 1, 1
    for i in range(n):
        ev[i]["name"] = ar.ref("node-%d" % i)
    return ev, bytes(ar.buf)


# ---- 1. device parse ----------------------------------------------------------
@pytest.mark.parametrize("indent,order,echo", [(None, ORDER, False), (1, ORDER, True),
                                               (None, ("status", "metadata", "spec", "kind", "apiVersion"), True),
                                               (2, ("metadata", "status", "spec"), False)],
                         ids=["compact", "indented-echo", "status-first-echo", "status-before-spec"])
def test_device_parse(indent, order, echo):
    """every document of tests/test_time_cpu.py, decided on the device (n_host == 0):
    the host codec's status and record bytes (test_json_gpu.compare), and
    creation_unix == calendar.timegm.  echo: the status is the template's own, so
    the no-op test compares its times with the creationTimestamp (KWOK_POD_CONFORMS);
    with the status first that is the device's second pass"""
    e = Engine(make_config(**KW))
    codec = Codec()
    ok, no = accepted() + far(), rejected()
    docs = [pod_document(s, k, indent=indent, order=order, echo=echo) for k, (s, _) in enumerate(ok + no)]
    compare_with_host(e, codec, docs, want_host=0, where="time documents")
    ev, _names, _keys, st, n_host = e.decode_pods_gpu(codec, docs)
    assert n_host == 0
    assert (st[:len(ok)] == abi.OK).all() and (st[len(ok):] == abi.EDOMAIN).all(), (
        [ok[i][0] for i in np.nonzero(st[:len(ok)])[0]], [no[i] for i in np.nonzero(st[len(ok):] != abi.EDOMAIN)[0]])
    want = np.array([t for _, t in ok], np.int64)
    bad = np.nonzero(ev["creation_unix"][:len(ok)] != want)[0]
    assert not len(bad), (ok[bad[0]], int(ev["creation_unix"][bad[0]]))
    assert (ev["creation_unix"][len(ok):] == 0).all()
    assert ((ev["flags"][:len(ok)] & abi.POD_CONFORMS) != 0).all() == echo
    assert ((ev["flags"][:len(ok)] & abi.POD_CONFORMS) != 0).any() == echo
    e.close()


# ---- 2. round trip --------------------------------------------------------------
def test_document_to_patch_round_trip():
    """creates through kwok_ingest_pods_json and through kwok_frame_watch_gpu +
    kwok_ingest_pods_framed, one tick: startTime, every lastTransitionTime and every
    startedAt / finishedAt of a pod's patch are the bytes of its document's
    creationTimestamp (no oracle).  0001-01-01 and 9999-12-31 decode and are refused
    by the ingest with KWOK_EDOMAIN"""
    e = Engine(make_config(**KW))
    codec = Codec()
    nev, nar = node_events(40)
    _, st = e.ingest_nodes_raw(nev, nar)
    assert (st == 0).all()
    e.register_pod_spec(*SPEC)  # (a document with a spec not seen before is listed for the host to register it)
    ok, out_of = accepted(), far()
    docs = [pod_document(s, k, node="node-%d" % (k % 40)) for k, (s, _) in enumerate(ok + out_of)]
    arena, offs, lens = Engine._docs(docs)
    hs, st, _rel, n_host = e.ingest_pods_json(codec, arena, offs, lens, np.full(len(docs), abi.OP_UPSERT, np.uint8),
                                              np.full(len(docs), -1, np.int32))
    assert n_host == 0 and (st[:len(ok)] == abi.OK).all() and (hs[:len(ok)] >= 0).all()
    assert list(st[len(ok):]) == [abi.EDOMAIN] * 2 and list(hs[len(ok):]) == [-1, -1]
    text = {int(h): s for h, (s, _) in zip(hs, ok)}
    framed = [(rfc3339(t), t) for t in EDGES]
    stream = b"".join(wf.wrap(pod_document(s, 90000 + k, node="node-%d" % k), "ADDED") for k, (s, _) in enumerate(framed))
    frames, used, n_host, sid = e.frame_watch(stream)
    assert used == len(stream) and n_host == 0 and len(frames) == len(framed) and not frames["status"].any()
    hs2, st2, _rel, n_host = e.ingest_pods_framed(codec, sid, np.arange(len(framed)), np.full(len(framed), -1, np.int32))
    assert n_host == 0 and (st2 == abi.OK).all()
    text.update({int(h): s for h, (s, _) in zip(hs2, framed)})
    assert len(text) == len(ok) + len(framed) == int(e.dump_pods(0, N_SLOTS)[0].sum())
    out = e.tick(secs(datetime(2024, 1, 1, 0, 0, 30)))
    assert sorted(h for h, _ in out.pod_patches) == sorted(text)
    for h, patch in out.pod_patches:
        start, rest = patch_times(patch)
        assert start == text[h] and len(rest) == 8 and set(rest) == {text[h]}, (h, text[h], patch)
    e.close()


# ---- 3. every emission path -----------------------------------------------------
# "mixed" here: the cap on table units (KWOK_EMIT_TAB_UNITS) that tables the first of the
# two default specs and not the second.  A spec's tables take EMIT_SHAPES x U units
# (templates.cpp build_unit_tables), U = its longest possible patch (both IPs 15 characters
# wide) in 16-byte units: with L the longest patch seen, ceil(L / 16) <= U <= ceil(L / 16) + 1.
# engine.cpp registers a spec's tables while the running total stays within the cap; the test
# asserts from its own patches that the cap lies between the first spec's most and the two
# specs' least (at tests/test_emit_paths_gpu.py's 20000 both would be tabled: no mix)
EMIT_SHAPES = 82
MIXED_CAP = 4000


@pytest.mark.parametrize("emit_path", list(EMIT_PATHS))
def test_emission_over_the_whole_domain(emit_path, monkeypatch):
    """600 pods of two specs on 40 nodes, half of them created at the edge seconds,
    half uniformly over [0, 2^32); start_time 2^31 + 5; ticks at 2^32 - 61, - 31 and
    - 1, each compared with the oracle (Driver.tick), each patch's startTime with
    datetime"""
    for k, v in EMIT_PATHS[emit_path].items():
        monkeypatch.setenv(k, str(MIXED_CAP) if emit_path == "mixed" else v)
    d = Driver(dict(KW, start_time=2 ** 31 + 5), 2106)
    nh, st = d.nodes(["node-%05d" % i for i in range(40)], managed=1, lockable=1)
    assert (st == 0).all()
    n = 600
    ev, ar = new_pods(d.rng, nh, n, d.spec, 0.05, (0x0A000000, 0x0A00FFFF), host_ips=["1.2.3.4", "196.168.0.1"],
                      host_ip_frac=0.3)
    ev["flags"] &= ~np.uint8(abi.POD_DISREGARD)  # (every pod is patched by the first tick)
    ev["creation_unix"][:n // 2] = np.resize(np.array(EDGES, np.int64), n // 2)
    ev["creation_unix"][n // 2:] = d.rng.integers(0, 2 ** 32, n - n // 2)
    assert (ev["creation_unix"] >= 2 ** 31).sum() > 200 and set(EDGES) <= set(ev["creation_unix"].tolist())
    hs, st, _ = d.pods(ev, ar)
    assert (st == 0).all()
    d.now = 2 ** 32 - 61
    patched = set()
    for k in range(3):
        assert d.now == (2 ** 32 - 61, 2 ** 32 - 31, 2 ** 32 - 1)[k]
        out = d.tick("%s tick %d" % (emit_path, k))
        assert len(out.heartbeat_nodes) == 40 and rfc3339(d.now - 30).encode() in out.heartbeat_body(0)
        if k == 0:
            assert len(out.pod_patches) == n and out.counters["node_init"] == 40
            units = [-(-max(len(p) for h, p in out.pod_patches if d.spec_of[h] == s) // 16) for s in d.spec]
            assert EMIT_SHAPES * (units[0] + 1) <= MIXED_CAP < EMIT_SHAPES * (units[0] + units[1]), units
        for h, patch in out.pod_patches:
            assert json.loads(patch)["status"]["startTime"] == rfc3339(d.ctime_of[h]), (h, int(d.ctime_of[h]))
            patched.add(h)
    assert patched == set(hs.tolist())
    d.e.close()
    d.o.close()


# ---- 4. the 32-bit word in the packed forms -------------------------------------
def test_creation_word_is_never_a_pod_ip():
    """creates through kwok_ingest_pods_packed, kwok_ingest_pods_packed12 and
    kwok_ingest_pods_packed12_tick whose creation words are the edge seconds, words
    that read as podIPs of the engine's CIDR, and 2024 times; then a non-create
    rec12 update of every pod whose value word is a podIP (some of them also 2024
    times) with a status that does not conform.  The next tick's patch carries the
    creation time as startTime and the update's podIP: oracle and datetime"""
    d = Driver(KW, 7, specs=[Driver.DEFAULT_SPECS[1]])
    nh, st = d.nodes(["node-%d" % i for i in range(8)], managed=1, lockable=1)
    assert (st == 0).all()
    node_ip = d.e.node_ip
    ip_like = [abi.ip4(s) for s in ("10.0.1.5", "10.0.0.2", "10.0.255.254", "10.0.7.77")]
    assert ip_like[0] == 0x0A000105 and all((w & 0xFFFF0000) == abi.ip4("10.0.0.0") for w in ip_like)
    assert all(at(w).year == 1975 for w in ip_like)  # (as times they are in the domain too)
    in_2024 = [secs(datetime(2024, 1, 1)), secs(datetime(2024, 6, 15, 12, 30, 45)), secs(datetime(2024, 12, 31, 23, 59, 59))]
    words = EDGES + ip_like + in_2024
    n = len(words)
    now = secs(datetime(2024, 1, 1, 0, 0, 30))

    def creates(k):
        r = np.zeros(n, abi.POD_REC_DTYPE)
        r["op"] = abi.OP_UPSERT | abi.REC_NEW
        r["target"] = nh[(np.arange(n) + k) % len(nh)]
        r["spec_id"] = d.spec[0]
        r["flags"] = abi.POD_STATUS_NONEMPTY | (abi.PHASE_PENDING << abi.REC_PHASE_SHIFT)
        r["creation"] = words
        return r

    ctime = {}
    # kwok_pod_rec
    r = creates(0)
    (h1, s1, _), (h2, s2, _) = d.e.ingest_pods_packed(r), d.o.ingest_pods_packed(r)
    assert (s1 == 0).all() and (s2 == 0).all() and (h1 == h2).all()
    ctime.update(zip(h1.tolist(), words))
    # kwok_pod_rec12
    r12 = abi.pack12(creates(1), node_ip)
    assert r12["value"].tolist() == words
    (h1, s1, _), (h2, s2, _) = d.e.ingest_pods_packed12(r12), d.o.ingest_pods_packed12(r12)
    assert (s1 == 0).all() and (s2 == 0).all() and (h1 == h2).all()
    ctime.update(zip(h1.tolist(), words))
    # kwok_pod_rec12 with the tick behind it
    r12 = abi.pack12(creates(2), node_ip)
    h1, s1, _ = d.e.ingest_pods_packed12(r12, tick_now=now)
    h2, s2, _ = d.o.ingest_pods_packed12(r12)
    assert (s1 == 0).all() and (s2 == 0).all() and (h1 == h2).all()
    ctime.update(zip(h1.tolist(), words))
    assert len(ctime) == 3 * n
    eo, oo = d.e.tick_collect(), d.o.tick(now)
    compare(eo, oo, "creates")
    compare_state(d.e, d.o, N_SLOTS, "creates")
    assert sorted(h for h, _ in eo.pod_patches) == sorted(ctime)
    for h, patch in eo.pod_patches:
        start, rest = patch_times(patch)
        assert start == rfc3339(ctime[h]) and set(rest) == {start}, (h, ctime[h], patch)
    # the updates: value = a podIP; the pods whose podIP reads as a 2024 time first
    handles = np.array(sorted(ctime), np.int32)
    m = len(handles)
    pod_ip = np.where(np.arange(m) % 2 == 0, secs(datetime(2024, 3, 1)) + 3601 * np.arange(m),
                      abi.ip4("10.0.64.1") + np.arange(m)).astype(np.uint32)
    assert len(set(pod_ip.tolist())) == m and all(at(int(w)).year == 2024 for w in pod_ip[0::2])
    assert all((int(w) & 0xFFFF0000) == abi.ip4("10.0.0.0") for w in pod_ip[1::2])
    u = np.zeros(m, abi.POD_REC_DTYPE)
    u["op"], u["target"], u["spec_id"] = abi.OP_UPSERT, handles, d.spec[0]
    u["flags"] = abi.POD_STATUS_NONEMPTY | (abi.PHASE_PENDING << abi.REC_PHASE_SHIFT)
    u["host_ip"], u["pod_ip"] = node_ip, pod_ip
    u12 = abi.pack12(u, node_ip)
    assert (u12["value"] == pod_ip).all() and not (u12["op"] & abi.REC_NEW).any()
    (_, s1, _), (_, s2, _) = d.e.ingest_pods_packed12(u12), d.o.ingest_pods_packed12(u12)
    assert (s1 == 0).all() and (s2 == 0).all()
    eo, oo = d.e.tick(now + 30), d.o.tick(now + 30)
    compare(eo, oo, "updates")
    compare_state(d.e, d.o, N_SLOTS, "updates")
    assert sorted(h for h, _ in eo.pod_patches) == handles.tolist()
    ip_of = dict(zip(handles.tolist(), pod_ip.tolist()))
    for h, patch in eo.pod_patches:
        start, rest = patch_times(patch)
        assert start == rfc3339(ctime[h]) and set(rest) == {start}, (h, ctime[h], patch)
        assert json.loads(patch)["status"]["podIP"] == abi.ip4s(ip_of[h]), (h, patch)
    d.e.close()
    d.o.close()


def test_creation_outside_the_domain_is_refused_per_record():
    """kwok_ingest_pods with creation_unix of -1, 2^32 and -2^31 (as a word: 2^31)
    beside 0, 2^32 - 1 and 2^31: KWOK_EDOMAIN per record on both sides, the records
    beside them applied and patched with their own times"""
    d = Driver(KW, 8, specs=[Driver.DEFAULT_SPECS[0]])
    nh, _ = d.nodes(["node-0", "node-1"], managed=1, lockable=1)
    ev, ar = new_pods(d.rng, nh, 6, d.spec)
    ev["flags"] &= ~np.uint8(abi.POD_DISREGARD)
    ev["creation_unix"] = [-1, 0, 2 ** 32, LAST, -2 ** 31, 2 ** 31]
    hs, st, _ = d.pods(ev, ar)  # (asserts that engine and oracle agree)
    E = abi.EDOMAIN
    assert list(st) == [E, 0, E, 0, E, 0] and [h >= 0 for h in hs] == [False, True, False, True, False, True]
    out = d.tick("after the refusals")
    assert len(out.pod_patches) == 3
    assert {json.loads(p)["status"]["startTime"] for _, p in out.pod_patches} == {rfc3339(t) for t in (0, LAST, 2 ** 31)}
    d.e.close()
    d.o.close()


# ---- 5. clocks and the delta stream ---------------------------------------------
# position of the 20 bytes -> two clocks whose strings differ there and nowhere else
ONE_POSITION = {1: (datetime(2006, 1, 1), datetime(2106, 1, 1)),
                2: (datetime(2037, 5, 6, 7, 8, 9), datetime(2087, 5, 6, 7, 8, 9)),
                3: (datetime(2100, 2, 28, 23, 59, 59), datetime(2104, 2, 28, 23, 59, 59)),
                5: (datetime(2024, 1, 30), datetime(2024, 11, 30)),
                6: (datetime(1999, 12, 31, 23, 59, 59), datetime(1999, 10, 31, 23, 59, 59)),
                8: (datetime(2000, 2, 9), datetime(2000, 2, 29)), 9: (datetime(2100, 2, 28), datetime(2100, 2, 21)),
                11: (datetime(2038, 1, 19, 3, 14, 7), datetime(2038, 1, 19, 23, 14, 7)),
                12: (datetime(2106, 2, 7, 6, 28, 15), datetime(2106, 2, 7, 0, 28, 15)),
                14: (datetime(1970, 1, 1, 0, 0, 1), datetime(1970, 1, 1, 0, 50, 1)),
                15: (datetime(2024, 2, 29, 12, 30, 0), datetime(2024, 2, 29, 12, 39, 0)),
                17: (datetime(2099, 12, 31, 23, 59, 59), datetime(2099, 12, 31, 23, 59, 9)),
                18: (datetime(2105, 7, 4, 1, 2, 3), datetime(2105, 7, 4, 1, 2, 4))}
ALMOST_ALL = [(datetime(2099, 12, 31, 23, 59, 59), datetime(2100, 1, 1)),
              (datetime(1999, 12, 31, 23, 59, 59), datetime(2000, 1, 1))]


def differing(a, b):
    return [k for k in range(20) if stamp(a)[k] != stamp(b)[k]]


def one_position_clocks():
    return [secs(dt) for k in sorted(ONE_POSITION) for dt in ONE_POSITION[k]]


def clock_steps():
    """the clocks after a first full tick, in order.  Every step is a delta tick but
    the one after clock 0: the kernels take a previous clock of 0 for "no previous
    body" and write everything (is_delta)"""
    c = one_position_clocks()
    for a, b in ALMOST_ALL:
        c += [secs(a), secs(b), secs(a)]                                   # forwards and backwards
    c += [secs(datetime(2100, 2, 28, 23, 59, 59)), secs(datetime(2100, 3, 1))]
    c += [2 ** 31 - 1, 2 ** 31, 2 ** 32 - 31, 2 ** 32 - 1, 2 ** 32 - 1]       # (the same clock twice)
    c += [0, 30, 60]
    return c


def test_the_clocks_are_what_they_are_chosen_for():
    assert sorted(ONE_POSITION) == [1, 2, 3, 5, 6, 8, 9, 11, 12, 14, 15, 17, 18]  # the 13 of the 14 digit positions
    for k, (a, b) in ONE_POSITION.items():
        assert differing(a, b) == [k] and 0 <= secs(a) <= LAST and 0 <= secs(b) <= LAST, (k, stamp(a), stamp(b))
    # position 0 cannot differ alone: no two years of the domain are 1000 apart
    years = range(at(0).year, at(LAST).year + 1)
    assert (years[0], years[-1]) == (1970, 2106) and not any(y + 1000 in years for y in years)
    for a, b in ALMOST_ALL:
        assert secs(b) - secs(a) == 1
    # every digit but the day's unit (31 -> 01), and in 2099 -> 2100 the year's thousands
    assert differing(*ALMOST_ALL[0]) == [1, 2, 3, 5, 6, 8, 11, 12, 14, 15, 17, 18]
    assert differing(*ALMOST_ALL[1]) == [0, 1, 2, 3, 5, 6, 8, 11, 12, 14, 15, 17, 18]
    assert secs(datetime(2100, 3, 1)) - secs(datetime(2100, 2, 28, 23, 59, 59)) == 1
    steps = clock_steps()
    assert steps[-3:] == [0, 30, 60] and steps.count(0) == 1 and steps[-5] == steps[-4] == LAST
    assert all(0 <= t <= LAST for t in steps)


def is_delta(prev):
    """a tick whose slot holds the bodies of the clock prev"""
    return prev != 0


@pytest.mark.parametrize("n,nt,share", [(5, 1, 512), (1027, 0, None)])
def test_clock_steps_blocking(n, nt, share, monkeypatch):
    """every step is a delta tick (ticks_hb_delta, Trio.tick), every body of every
    tick equals the oracle's and the region equals the KWOK_HB_DELTA=0 engine's.
    The tick at clock 0 is a delta tick against the clock before it; the tick at 30
    that follows reports no delta tick (ticks_hb_delta does not move): it wrote every
    byte, and its bytes are compared like every other tick's"""
    t = hbd.Trio(monkeypatch, nt, share)
    t.nodes(["node-%07d" % i for i in range(n)])
    prev = hbd.T0
    _, got, _, _ = t.tick(prev, "first tick", delta=False)
    assert got == n
    deltas = 0
    for k, now in enumerate(clock_steps()):
        E, got, st, ln = t.tick(now, "step %d: %s -> %s (n=%d)" % (k, rfc3339(prev), rfc3339(now), n), delta=is_delta(prev))
        assert got == n and bytes(E["arena"][:ln]).count(rfc3339(now).encode()) >= 4
        deltas += is_delta(prev)
        prev = now
    assert t.delta_ticks() == deltas == len(clock_steps()) - 1
    t.close()


def test_clock_steps_queued_two_deep(monkeypatch):
    """test_hb_delta_gpu.run_queued's shape: tick k+1 is submitted before tick k is
    collected, so each slot's previous clock is two ticks back"""
    n = 1027
    t = hbd.Trio(monkeypatch, 0)
    t.nodes(["node-%07d" % i for i in range(n)])
    clocks = [hbd.T0, hbd.T0 + 30] + clock_steps()
    for x in (t.e, t.f):
        x.tick_submit(clocks[0])
    deltas = 0
    for k, now in enumerate(clocks):
        for x in (t.e, t.f):
            if k + 1 < len(clocks):
                x.tick_submit(clocks[k + 1])
            x.tick_collect(read=False)
        t.o.tick(now, read=False)
        deltas += k >= 2 and is_delta(clocks[k - 2])
        assert t.delta_ticks() == deltas, "queued tick %d" % k
        _, got, _, _ = t.check(now, "queued tick %d: %s -> %s" % (k, rfc3339(clocks[max(0, k - 2)]), rfc3339(now)))
        assert got == n
    assert deltas == len(clocks) - 2 - 1  # (all but the one two ticks after clock 0)
    t.close()


def test_clock_steps_once_stream(monkeypatch):
    """the same steps as quiet ticks through k_once_stream (ticks_once_stream moves
    with every one, test_once_stream_gpu.Trio.tick), against a KWOK_ONCE_STREAM=0
    engine and the oracle"""
    n = 1027
    t = ons.Trio(monkeypatch, ons.fleet_env(1, 3, None))
    t.nodes(["node-%07d" % i for i in range(n)])
    prev = ons.T0
    t.tick(prev, "first tick", once=False, delta=False)
    for k, now in enumerate(clock_steps()):
        _, got = t.tick(now, "step %d: %s -> %s" % (k, rfc3339(prev), rfc3339(now)), once=True, delta=is_delta(prev))
        assert got == n
        prev = now
    p = t.paths()
    assert p["ticks_once_stream"] == len(clock_steps()) and p["ticks_hb_delta"] == len(clock_steps()) - 1
    t.close()


def test_clock_steps_heartbeat_once_engine():
    """KWOK_CFG_HEARTBEAT_ONCE: one body per tick, never a delta; the oracle's body"""
    e, o = Engine(make_config(heartbeat_once=True, **KW)), Oracle(make_config(**KW))
    nev, nar = node_events(37)
    assert (e.ingest_nodes_raw(nev, nar)[0] == o.ingest_nodes_raw(nev, nar)[0]).all()
    for k, now in enumerate([hbd.T0] + clock_steps()):
        e.tick(now, read=False)
        o.tick(now, read=False)
        compare_tick(e, o, "heartbeat-once tick %d at %s" % (k, rfc3339(now)), once=True)
        E = e.read_arrays(heartbeat_once=True)
        body = bytes(E["arena"][E["heartbeat_off"]:E["heartbeat_off"] + E["heartbeat_len"]])
        assert len(E["heartbeat_nodes"]) == 37 and body.count(rfc3339(now).encode()) >= 4
    assert e.stats()["ticks_hb_delta"] == 0
    e.close()
    o.close()


def test_one_position_clocks_custom_heartbeat_template(monkeypatch):
    """heartbeat_a.tpl (79 units per slot) over the 13 single-position pairs.  No
    oracle: the body of a clock is the host template compiler's body of a reference
    clock with rfc3339(now) in place of that clock's six Now values"""
    from test_template_cpu import tpl
    htext = tpl("heartbeat_a.tpl")
    n, start, ref = 5, 1704067200, hbd.T0
    ref_body = engine.heartbeat_template_patch(htext, start, "196.168.0.1", ref)
    assert ref_body.count(rfc3339(ref).encode()) == 6 == ref_body.count(rfc3339(start).encode())
    t = hbd.Trio(monkeypatch, 1, oracle=False, node_heartbeat_template=htext)
    t.body = lambda now: ref_body.replace(rfc3339(ref).encode(), rfc3339(now).encode())
    t.nodes(["node-%07d" % i for i in range(n)])
    _, got, st, ln = t.tick(ref, "first tick", delta=False)
    assert got == n and ln == len(ref_body) and st // 16 == 79
    prev = ref
    for k, now in enumerate(one_position_clocks()):
        assert now != 0 and t.body(now).count(rfc3339(now).encode()) == 6
        t.tick(now, "custom step %d: %s -> %s" % (k, rfc3339(prev), rfc3339(now)), delta=True)
        prev = now
    assert t.delta_ticks() == 26
    t.close()


def test_clocks_outside_the_domain_are_refused():
    """the code each entry returns: KWOK_EDOMAIN from kwok_tick and kwok_tick_submit at
    -1 and 2^32 and from kwok_ingest_pods_packed12_tick at 2^32 (before the batch is
    touched), KWOK_EINVAL from the latter at -1 (a negative tick_now is no clock);
    a start_time of -1 or 2^32 fails the engine's creation with KWOK_EDOMAIN.  The
    oracle refuses the same (tests/test_time_cpu.py)"""
    d = Driver(KW, 9, specs=[Driver.DEFAULT_SPECS[0]])
    nh, _ = d.nodes(["node-0", "node-1"], managed=1, lockable=1)
    r = np.zeros(4, abi.POD_REC_DTYPE)
    r["op"], r["target"], r["spec_id"] = abi.OP_UPSERT | abi.REC_NEW, nh[0], d.spec[0]
    r["flags"] = abi.POD_STATUS_NONEMPTY | (abi.PHASE_PENDING << abi.REC_PHASE_SHIFT)
    r["creation"] = [0, 2 ** 31, LAST, 1]
    r12 = abi.pack12(r, d.e.node_ip)
    for now in (-1, 2 ** 32):
        for what, call in (("tick", lambda: d.e.tick(now)), ("tick_submit", lambda: d.e.tick_submit(now)),
                           ("packed12_tick", lambda: d.e.ingest_pods_packed12(r12, tick_now=now)),
                           ("oracle tick", lambda: d.o.tick(now))):
            with pytest.raises(KwokError) as ei:
                call()
            assert ei.value.code == (abi.EINVAL if (what, now) == ("packed12_tick", -1) else abi.EDOMAIN), (what, now)
    assert int(d.e.dump_pods(0, N_SLOTS)[0].sum()) == 0  # (no refused call applied its batch)
    # nothing is queued, and the engine goes on: the batch, its tick at the domain's last second
    h1, s1, _ = d.e.ingest_pods_packed12(r12, tick_now=LAST)
    h2, s2, _ = d.o.ingest_pods_packed12(r12)
    assert (s1 == 0).all() and (h1 == h2).all()
    eo, oo = d.e.tick_collect(), d.o.tick(LAST)
    compare(eo, oo, "after the refused clocks")
    assert len(eo.pod_patches) == 4 and rfc3339(LAST).encode() in eo.heartbeat_body(0)
    d.e.close()
    d.o.close()
    for start in (-1, 2 ** 32):
        with pytest.raises(KwokError) as ei:
            Engine(make_config(start_time=start, **KW))
        assert ei.value.code == abi.EDOMAIN, start
    e = Engine(make_config(start_time=LAST, **KW))  # (the domain's last second is inside)
    e.close()
