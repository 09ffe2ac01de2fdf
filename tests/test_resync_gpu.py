"""GPU: relist with Replace at the engine level (include/kwok_watch.h, DESIGN.md
§22; resync.hip: k_seen_mark_*, k_sweep_count, k_sweep_emit; the apply is the
ingest's own event switch).

Three backends run in lockstep (Trio): engine `a` sweeps; engine `b` is fed the
same upserts and the absent objects as kwok_pod_rec / kwok_node_event DELETE
records; the oracle `o` gets them as Deleted events carrying the podIP the pod
holds (pod_controller.go:320-343, node_controller.go:265-269).  Every later tick
of `a` equals the oracle's output for output; against `b` also the pod state,
kwok_node_size, kwok_engine_stats tick by tick (which tick kernel ran: a sweep
must leave the engine in the quiet-Use regime exactly when the deletes do), the
handles later creates receive, and the swept handle list in the records' order."""
import json

import numpy as np
import pytest

import watch_frames as wf
from gpu_common import compare
from harness import MANAGE, node_doc, pod_doc
from kwok_amd import abi
from kwok_amd.codec import Codec
from kwok_amd.engine import Engine, KwokError, make_config
from oracle.oracle import Oracle
from test_once_gpu import compare_once

pytestmark = pytest.mark.gpu

T0 = 1704067230
NODES, PODS = abi.KIND_NODES, abi.KIND_PODS
KW = dict(cidr="10.0.0.1/16", node_ip="196.168.0.1", buckets=64, node_slots_per_bucket=32, pod_slots_per_bucket=512)
SPECS = [([("fake-pod", "fake")], [], []),
         ([("a", "img-a"), ("b", "img/b:v2")], [("init", "busybox")], ["g.io/x"])]
KEEP_FLAGS = abi.POD_DISREGARD | abi.POD_HAS_FINALIZERS


class Trio:
    def __init__(self, once=False, seed=5, **geom):
        self.kw = dict(KW, **geom)
        self.once = once
        self.a = Engine(make_config(heartbeat_once=once, **self.kw))
        self.b = Engine(make_config(heartbeat_once=once, **self.kw))
        self.o = Oracle(make_config(**self.kw))
        self.all = (self.a, self.b, self.o)
        ids = [[x.register_pod_spec(*s) for s in SPECS] for x in self.all]
        assert ids[0] == ids[1] == ids[2]
        self.spec = ids[0]
        self.stride = self.kw.get("pod_handle_stride") or self.kw["pod_slots_per_bucket"]
        self.n_slots = self.kw["buckets"] * self.stride
        self.meta = {}  # pod handle -> (spec, creation, DISREGARD | HAS_FINALIZERS, node handle)
        self.now = T0
        self.rng = np.random.default_rng(seed)

    def close(self):
        for x in self.all:
            x.close()

    def nodes(self, names, managed=1, lockable=1, op=abi.OP_UPSERT):
        ar = abi.Arena()
        ev = np.zeros(len(names), abi.NODE_EVENT_DTYPE)
        ev["op"] = op
        ev["managed"] = managed
        ev["lockable"] = lockable
        for i, n in enumerate(names):
            ev[i]["name"] = ar.ref(n)
        got = [x.ingest_nodes_raw(ev, bytes(ar.buf)) for x in self.all]
        for h, s in got[1:]:
            assert (h == got[0][0]).all() and (s == got[0][1]).all()
        return got[0]

    def pods(self, ev, arena=b""):
        got = [x.ingest_pods_raw(ev, arena) for x in self.all]
        for h, s, r in got[1:]:
            assert (h == got[0][0]).all() and (s == got[0][1]).all() and (r == got[0][2]).all()
        h, s, r = got[0]
        for i in np.nonzero((ev["op"] == abi.OP_UPSERT) & (ev["handle"] < 0) & (s == 0))[0]:
            self.meta[int(h[i])] = (int(ev[i]["spec_id"]), int(ev[i]["creation_unix"]), int(ev[i]["flags"]) & KEEP_FLAGS,
                                    int(ev[i]["node_handle"]))
        return h, s, r

    def create(self, node_handles, flags=abi.POD_STATUS_NONEMPTY, phase=abi.PHASE_PENDING, pod_ip=None):
        n = len(node_handles)
        ar = abi.Arena()
        ev = np.zeros(n, abi.POD_EVENT_DTYPE)
        ev["op"] = abi.OP_UPSERT
        ev["handle"] = -1
        ev["node_handle"] = node_handles
        ev["spec_id"] = self.rng.choice(self.spec, n)
        ev["creation_unix"] = T0 - 30 - self.rng.integers(0, 10 ** 6, n)
        ev["phase"] = phase
        ev["flags"] = flags
        if pod_ip:
            for i in range(n):
                ev[i]["pod_ip"] = ar.ref(pod_ip[i])
        h, s, _ = self.pods(ev, bytes(ar.buf))
        assert (s == 0).all(), list(s)
        return h

    def live(self):
        used, phase, hip, pip = self.o.dump_pods(0, self.n_slots)
        idx = np.nonzero(used)[0].astype(np.int32)
        return idx, phase[idx], hip[idx], pip[idx]

    def reupsert(self, handles):
        """the List items of pods the engine holds: Modified-like upserts that restate their state"""
        idx, phase, hip, pip = self.live()
        handles = np.asarray(handles, np.int32)
        pos = np.searchsorted(idx, handles)
        ar = abi.Arena()
        ev = np.zeros(len(handles), abi.POD_EVENT_DTYPE)
        ev["op"] = abi.OP_UPSERT
        ev["handle"] = handles
        ev["node_handle"] = -1
        ev["phase"] = phase[pos]
        for i, h in enumerate(handles):
            spec, ctime, fl, _node = self.meta[int(h)]
            ev[i]["spec_id"] = spec
            ev[i]["creation_unix"] = ctime
            if phase[pos[i]] == abi.PHASE_RUNNING:
                fl |= abi.POD_CONFORMS | abi.POD_STATUS_NONEMPTY
            elif phase[pos[i]] == abi.PHASE_PENDING:
                fl |= abi.POD_STATUS_NONEMPTY
            ev[i]["flags"] = fl
            if hip[pos[i]]:
                ev[i]["host_ip"] = ar.ref(abi.ip4s(int(hip[pos[i]])))
            if pip[pos[i]]:
                ev[i]["pod_ip"] = ar.ref(abi.ip4s(int(pip[pos[i]])))
        return ev, bytes(ar.buf)

    def sweep_pods(self, absent, where):
        """a sweeps; b gets the absent pods as kwok_pod_rec DELETE records, o as Deleted events"""
        absent = np.sort(np.asarray(absent, np.int32))
        idx, _phase, _hip, pip = self.live()
        held = pip[np.searchsorted(idx, absent)] if len(absent) else np.zeros(0, np.uint32)
        swept, rel, nd = self.a.resync_sweep(PODS)
        assert list(swept) == list(absent), where + " swept handles"
        assert list(nd) == [self.meta[int(h)][3] for h in absent], where + " node handles"
        if len(absent):
            recs = np.zeros(len(absent), abi.POD_REC_DTYPE)
            recs["op"] = abi.OP_DELETE
            recs["target"] = absent
            recs["pod_ip"] = held
            hb, sb, rb = self.b.ingest_pods_packed(recs)
            assert not sb.any() and list(hb) == list(absent)
            assert list(rel) == list(rb), where + " released (DELETE records)"
            ar = abi.Arena()
            ev = np.zeros(len(absent), abi.POD_EVENT_DTYPE)
            ev["op"] = abi.OP_DELETE
            ev["handle"] = absent
            for i in range(len(absent)):
                if held[i]:
                    ev[i]["pod_ip"] = ar.ref(abi.ip4s(int(held[i])))
            ho, so, ro = self.o.ingest_pods_raw(ev, bytes(ar.buf))
            assert not so.any()
            assert list(rel) == list(ro), where + " released (oracle)"
        for h in absent:
            del self.meta[int(h)]
        self.state(where)
        return swept, rel, nd

    def sweep_nodes(self, absent_names, handle_of, where):
        swept, _rel, _nd = self.a.resync_sweep(NODES)
        want = sorted(handle_of[n] for n in absent_names)
        assert list(swept) == want, where + " swept node handles"
        if absent_names:
            names = sorted(absent_names, key=lambda n: handle_of[n])
            ar = abi.Arena()
            ev = np.zeros(len(names), abi.NODE_EVENT_DTYPE)
            ev["op"] = abi.OP_DELETE
            for i, n in enumerate(names):
                ev[i]["name"] = ar.ref(n)
            for x in (self.b, self.o):
                h, s = x.ingest_nodes_raw(ev, bytes(ar.buf))
                assert not s.any() and list(h) == want
        self.state(where)
        return swept

    def state(self, where):
        da, db, do = (x.dump_pods(0, self.n_slots) for x in self.all)
        for k, what in enumerate(("used", "phase", "hostIP", "podIP")):
            assert (da[k] == do[k]).all(), "%s: pod %s differs from the oracle" % (where, what)
            assert (da[k] == db[k]).all(), "%s: pod %s differs from the DELETE-record engine" % (where, what)
        assert self.a.node_size() == self.b.node_size() == self.o.node_size(), where + " node_size"

    def tick(self, where):
        for x in self.all:
            x.tick(self.now, read=False)
        self.now += 30
        return self.outputs(where)

    def outputs(self, where):
        """the collected tick of all three"""
        ao, bo = (x.read_outputs(heartbeat_once=self.once) for x in (self.a, self.b))
        oo = self.o.read_outputs()
        (compare_once if self.once else compare)(ao, oo, where)
        assert list(ao.heartbeat_nodes) == list(bo.heartbeat_nodes), where + " heartbeat handles (a / b)"
        assert ao.node_inits == bo.node_inits and ao.pod_patches == bo.pod_patches and ao.deletes == bo.deletes, where
        assert ao.counters == bo.counters, where
        assert self.a.stats() == self.b.stats(), "%s: tick kernels %r vs %r" % (where, self.a.stats(), self.b.stats())
        self.state(where)
        return ao


def fleet(t, n_nodes=24, n_pods=300):
    """managed and unmanaged nodes; Pending pods spread over them, pods on unmanaged nodes, pods holding an
    address outside the CIDR, disregarded pods; one tick (addresses assigned) and a steady one; then pods
    created after it (Pending, no address yet) and delete-pending pods with finalizers"""
    names = ["node-%03d" % i for i in range(n_nodes)] + ["plain-%d" % i for i in range(4)]
    managed = np.array([1] * n_nodes + [0] * 4, np.uint8)
    nh, st = t.nodes(names, managed)
    assert not st.any()
    t.node_handle = dict(zip(names, (int(h) for h in nh)))
    man, plain = nh[:n_nodes], nh[n_nodes:]
    t.create(t.rng.choice(man, n_pods))
    t.create(t.rng.choice(plain, 12))
    t.create(t.rng.choice(man, 5), pod_ip=["192.168.7.%d" % (i + 2) for i in range(5)])
    t.create(t.rng.choice(man, 6), flags=abi.POD_STATUS_NONEMPTY | abi.POD_DISREGARD)
    t.tick("initial")
    t.tick("steady")
    late = t.create(t.rng.choice(man, 6))
    idx, phase, _hip, _pip = t.live()
    running = idx[phase == abi.PHASE_RUNNING]
    dying = np.sort(t.rng.choice(running, 6, replace=False)).astype(np.int32)
    ev, ar = t.reupsert(dying)
    ev["flags"] |= abi.POD_DELETING | abi.POD_HAS_FINALIZERS
    t.pods(ev, ar)
    for h in dying:
        sp, ct, fl, nd = t.meta[int(h)]
        t.meta[int(h)] = (sp, ct, fl | abi.POD_HAS_FINALIZERS, nd)
    return nh, late, dying


def _absent(kind, t, live):
    b = live // t.stride
    if kind == "none":
        return live[:0]
    if kind == "all":
        return live
    if kind == "every_other":
        return live[::2]
    big = int(np.bincount(b).argmax())
    if kind == "lo_hi":
        mine = live[b == big]
        return np.array([mine[0], mine[-1]], np.int32)
    return live[b == big]  # one_bucket


@pytest.mark.parametrize("once", [True, False], ids=["heartbeat-once", "full-body"])
@pytest.mark.parametrize("kind", ["none", "all", "every_other", "lo_hi", "one_bucket"])
def test_absent_sets(kind, once):
    t = Trio(once=once)
    nh, late, dying = fleet(t)
    live, *_ = t.live()
    absent = _absent(kind, t, live)
    if kind == "every_other":  # every kind of pod is among the absent ones
        assert set(absent) & set(late) and set(absent) & set(dying)
    t.a.resync_begin(PODS)
    keep = np.setdiff1d(live, absent)
    if len(keep):
        t.pods(*t.reupsert(keep))
    swept, rel, _nd = t.sweep_pods(absent, kind)
    s = t.a.resync_stats()
    assert s["sessions"] == 1 and s["marked"] == len(keep) and s["swept_pods"] == len(absent)
    assert s["released"] == int((rel != 0).sum())
    for k in range(2):  # new creates take the lowest released addresses (the oracle's)
        t.create(t.rng.choice(nh[:24], 40))
        t.tick("%s after %d" % (kind, k))
    t.tick(kind + " quiet")
    with pytest.raises(KwokError) as ei:  # the sweep closed the session
        t.a.resync_sweep(PODS)
    assert ei.value.code == abi.EINVAL
    t.close()


@pytest.mark.parametrize("r", [0, 5, 16])
def test_compaction_boundaries(r):
    """survivors at slot residue r mod 17; a bucket past one tile (2048 slots), buckets whose fill mark ends
    around a 16-slot window (15 and 17 pods), empty buckets between full ones"""
    t = Trio(buckets=16, node_slots_per_bucket=8, pod_slots_per_bucket=4096)
    names = ["n%d" % i for i in range(5)]
    nh, _ = t.nodes(names)
    t.create(np.full(2100, nh[0], np.int32))
    t.create(np.full(15, nh[1], np.int32))
    t.create(np.full(17, nh[2], np.int32))
    t.create(np.full(600, nh[3], np.int32))
    t.tick("initial")
    live, *_ = t.live()
    assert len(set(live // t.stride)) < 16  # (some bucket is empty)
    keep = live[(live % t.stride) % 17 == r]
    t.a.resync_begin(PODS)
    t.pods(*t.reupsert(keep))
    t.sweep_pods(np.setdiff1d(live, keep), "residue %d" % r)
    t.create(np.full(30, nh[0], np.int32))
    t.tick("after")
    t.close()


def test_more_tiles_than_one_scan_step():
    """4096 buckets (one tile each, four steps of the scan over the tile counts): a thin fleet over all of
    them, one pod in three absent"""
    t = Trio(once=True, buckets=4096, node_slots_per_bucket=16, pod_slots_per_bucket=640)
    assert 4096 > abi.WATCH_SCAN_TILES
    nh, _ = t.nodes(["node-%05d" % i for i in range(3000)])
    t.create(t.rng.choice(nh, 4000))
    t.tick("initial")
    live, *_ = t.live()
    assert len(set(live // t.stride)) > 1500
    absent = live[::3]
    t.a.resync_begin(PODS)
    t.pods(*t.reupsert(np.setdiff1d(live, absent)))
    t.sweep_pods(absent, "thin")
    t.tick("after")
    t.close()


def test_explicit_marks_and_session_rules():
    t = Trio()
    nh, _late, _dying = fleet(t, n_pods=120)
    t.tick("delete-pending pods gone")  # (so that the tick drained below removes no pod)
    live, *_ = t.live()
    a = t.a
    # no session: EINVAL, nothing changes
    for call in (lambda: a.resync_sweep(PODS), lambda: a.resync_mark(PODS, live[:3]), lambda: a.resync_sweep(NODES)):
        with pytest.raises(KwokError) as ei:
            call()
        assert ei.value.code == abi.EINVAL
    t.state("no session")
    # resync_end deletes nothing; marks of an ended session do not exist
    a.resync_begin(PODS)
    assert a.resync_mark(PODS, live[:50]) == 0
    a.resync_end(PODS)
    t.state("ended")
    # begin twice clears
    a.resync_begin(PODS)
    assert a.resync_mark(PODS, live[:50]) == 0
    a.resync_begin(PODS)
    free = int(np.setdiff1d(np.arange(t.stride * 3, t.stride * 3 + 512), live)[0])
    bad = np.array([-1, t.n_slots + 5, 2 ** 31 - 1, free], np.int32)
    assert a.resync_mark(PODS, np.concatenate([live[50:], bad])) == len(bad)
    # a node session open at the same time is independent: every node marked, none swept
    a.resync_begin(NODES)
    assert a.resync_mark(NODES, np.concatenate([nh, np.array([-1, 64 * 32, int(nh.max()) + 1], np.int32)])) == 3
    # a tick submitted and not collected is drained by the sweep; cap one below the count is refused
    for x in (t.a, t.b):
        x.tick_submit(t.now)
    with pytest.raises(KwokError) as ei:
        a.resync_sweep(PODS, cap=49)
    assert ei.value.code == abi.EINVAL and ei.value.n_swept == 50
    for x in (t.a, t.b):
        x.tick_collect(read=False)
    t.o.tick(t.now, read=False)
    t.now += 30
    t.outputs("drained tick, sweep refused")  # (nothing removed: the state equals both yardsticks')
    t.sweep_pods(live[:50], "retry")
    assert list(a.resync_sweep(NODES)[0]) == []
    s = a.resync_stats()
    assert s["sessions"] == 4 and s["swept_pods"] == 50 and s["swept_nodes"] == 0
    t.tick("after")
    t.close()


def test_growth_inside_a_session():
    t = Trio(buckets=64, node_slots_per_bucket=8, pod_slots_per_bucket=16, pod_handle_stride=8192)
    nh, _ = t.nodes(["node-%07d" % i for i in range(40)])
    old = t.create(np.full(14, nh[0], np.int32))
    other = t.create(t.rng.choice(nh[1:], 60))
    t.tick("initial")
    t.a.resync_begin(PODS)
    t.pods(*t.reupsert(np.sort(old[:10])))
    new = t.create(np.full(300, nh[0], np.int32))  # grows the bucket inside the session
    live, *_ = t.live()
    absent = np.setdiff1d(live, np.concatenate([old[:10], new]))
    assert set(absent) == set(old[10:]) | set(other)
    t.sweep_pods(absent, "grown")
    t.tick("after")
    t.close()


@pytest.mark.parametrize("once", [True, False], ids=["heartbeat-once", "full-body"])
def test_nodes(once):
    t = Trio(once=once)
    names = ["node-%03d" % i for i in range(20)]
    nh, _ = t.nodes(names)
    hof = dict(zip(names, (int(h) for h in nh)))
    with_pods = names[:10]
    t.create(np.repeat(nh[:10], 8))
    t.tick("initial")
    t.tick("steady")
    # the list holds nodes 0-4 and 12-19: 5-9 (with pods) become zombies, 10-11 (without) free their entries
    t.a.resync_begin(NODES)
    kept = names[:5] + names[12:]
    t.nodes(kept)
    absent = names[5:12]
    size0 = t.a.node_size()
    t.sweep_nodes(absent, hof, "nodes")
    assert t.a.node_size() == size0 - len(absent)
    assert t.a.resync_stats()["swept_nodes"] == len(absent)
    out = t.tick("after nodes")
    assert not set(hof[n] for n in absent) & set(int(h) for h in out.heartbeat_nodes)
    # a new node takes the lowest free index of its bucket; a swept name comes back
    h2, s2 = t.nodes(["fresh-%d" % i for i in range(12)] + [names[10], names[6]])
    assert not s2.any()
    t.tick("after re-add")
    # sweeping every pod frees the zombies
    live, *_ = t.live()
    t.a.resync_begin(PODS)
    t.sweep_pods(live, "all pods")
    t.tick("after pods")
    t.tick("quiet")
    t.close()


# ---- every ingest entry marks ---------------------------------------------------------
def _ev(key, node, **kw):
    return dict(dict(key=key, node=node, disregard=False, deleting=False, finalizers=0, creation=T0 - 90, phase="Pending",
                     status_nonempty=False, conforms=False, hostIP="", podIP="",
                     spec={"containers": [["fake-pod", "fake"]], "init": [], "gates": []}), **kw)


def _nev(name):
    return dict(name=name, managed=True, lockable=True, phase="", addresses=None, allocatable=None, capacity=None, nodeInfo={})


def test_every_ingest_entry_marks():
    e = Engine(make_config(**KW))
    spec = e.register_pod_spec(*SPECS[0])
    codec = Codec(manage_all_nodes=False, manage_nodes_with_annotation_selector=MANAGE)
    ops = lambda n: np.full(n, abi.OP_UPSERT, np.uint8)  # noqa: E731
    # nodes: one touched through each node entry, each with an untouched twin
    entries = ("raw", "json", "framed", "json-host")
    nnames = ["%s-%s" % (k, w) for k in entries for w in ("seen", "twin")]
    ndocs = [json.dumps(node_doc(_nev(n))).encode() for n in nnames]
    arena, offs, lens = Engine._docs(ndocs)
    nh, st, _ = e.ingest_nodes_json(codec, arena, offs, lens, ops(len(nnames)))
    assert not st.any()
    nhof = dict(zip(nnames, (int(h) for h in nh)))
    # pods: two per entry (touched, twin), all on one node
    pentries = ("raw", "packed", "packed12", "packed12_tick", "json", "json-host", "framed", "rejected")
    keys = ["%s-%s" % (k, w) for k in pentries for w in ("seen", "twin")]
    pdocs = [json.dumps(pod_doc(_ev(k, "raw-seen"))).encode() for k in keys]
    arena, offs, lens = Engine._docs(pdocs)
    ph, st, _rel, _nhost = e.ingest_pods_json(codec, arena, offs, lens, ops(len(keys)), np.full(len(keys), -1, np.int32))
    assert not st.any()
    hof = dict(zip(keys, (int(h) for h in ph)))
    e.tick(T0)
    e.resync_begin(NODES)
    e.resync_begin(PODS)
    m0 = e.resync_stats()["marked"]

    # -- nodes
    ar = abi.Arena()
    ev = np.zeros(1, abi.NODE_EVENT_DTYPE)
    ev["op"], ev["managed"], ev["lockable"] = abi.OP_UPSERT, 1, 1
    ev[0]["name"] = ar.ref("raw-seen")
    assert not e.ingest_nodes_raw(ev, bytes(ar.buf))[1].any()
    arena, offs, lens = Engine._docs([ndocs[nnames.index("json-seen")]])
    assert not e.ingest_nodes_json(codec, arena, offs, lens, ops(1))[1].any()
    host_doc = node_doc(_nev("json-host-seen"))
    host_doc["status"]["addresses"] = [{"type": "InternalIP", "address": "10.9.9.9"}]  # a status the host completes
    arena, offs, lens = Engine._docs([json.dumps(host_doc).encode()])
    _h, st, nhost = e.ingest_nodes_json(codec, arena, offs, lens, ops(1))
    assert not st.any() and nhost == 1
    stream = wf.wrap(ndocs[nnames.index("framed-seen")], "MODIFIED")
    _frames, _used, _n, sid = e.frame_watch(stream)
    assert not e.ingest_nodes_framed(codec, sid, np.array([0], np.uint32))[1].any()

    # -- pods
    def doc(k, **kw):
        return json.dumps(pod_doc(_ev(k, "raw-seen", **kw))).encode()

    pe = np.zeros(1, abi.POD_EVENT_DTYPE)
    pe["op"], pe["handle"], pe["node_handle"], pe["spec_id"] = abi.OP_UPSERT, hof["raw-seen"], -1, spec
    pe["phase"], pe["creation_unix"] = abi.PHASE_PENDING, T0 - 90
    assert not e.ingest_pods_raw(pe, b"")[1].any()
    rec = np.zeros(1, abi.POD_REC_DTYPE)
    rec["op"], rec["spec_id"], rec["target"], rec["creation"] = abi.OP_UPSERT, spec, hof["packed-seen"], T0 - 90
    rec["flags"] = abi.PHASE_PENDING << 5
    assert not e.ingest_pods_packed(rec)[1].any()
    for k, tick_now in (("packed12", None), ("packed12_tick", T0 + 30)):
        r12 = np.zeros(1, abi.POD_REC12_DTYPE)  # not a create: marked by its target
        r12["op"], r12["spec_id"], r12["target"] = abi.OP_UPSERT, spec, hof[k + "-seen"]
        r12["flags"] = abi.PHASE_PENDING << 5
        assert not e.ingest_pods_packed12(r12, tick_now=tick_now)[1].any()
        if tick_now:
            e.tick_collect(read=False)
    for k in ("json", "json-host"):  # json-host: a pod spec not registered yet, which the host codec completes
        d = doc(k + "-seen", **(dict(spec={"containers": [["late", "img:2"]], "init": [], "gates": []}) if k == "json-host" else {}))
        arena, offs, lens = Engine._docs([d])
        _h, st, _r, nhost = e.ingest_pods_json(codec, arena, offs, lens, ops(1), np.array([hof[k + "-seen"]], np.int32))
        assert (int(st[0]), nhost) == (abi.OK, 1 if k == "json-host" else 0), (k, int(st[0]), nhost)
    stream = wf.wrap(doc("framed-seen"), "MODIFIED")
    _frames, _used, _n, sid = e.frame_watch(stream)
    assert not e.ingest_pods_framed(codec, sid, np.array([0], np.uint32), np.array([hof["framed-seen"]], np.int32))[1].any()
    # a rejected record (a phase out of range) marks nothing: both "rejected" pods go
    rec["target"], rec["flags"] = hof["rejected-seen"], 7 << 5
    assert e.ingest_pods_packed(rec)[1][0] == abi.EINVAL

    assert e.resync_stats()["marked"] - m0 == 4 + 7
    swept_n, _r, _d = e.resync_sweep(NODES)
    assert sorted(swept_n) == sorted(nhof[k + "-twin"] for k in entries)
    swept, _rel, nd = e.resync_sweep(PODS)
    want = sorted([hof[k + "-twin"] for k in pentries] + [hof["rejected-seen"]])
    assert list(swept) == want
    assert set(nd) == {nhof["raw-seen"]}
    used = e.dump_pods(0, 64 * 512)[0]
    assert sorted(np.nonzero(used)[0]) == sorted(hof[k + "-seen"] for k in pentries if k != "rejected")
    e.close()
