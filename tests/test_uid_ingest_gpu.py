"""GPU: kwok_ingest_pods_framed_uid against the host path, record for record
(include/kwok_watch.h; uid.hip: k_uid_resolve, k_uid_claim, k_uid_cut,
k_uid_note, k_uid_fix).

Three backends in lockstep: engine `a` takes every batch with one by-uid call; engine
`b` takes it through controller.ingest_pod_runs over kwok_ingest_pods_framed with a
uid -> handle dict (the yardstick); the oracle `o` is fed b's records (the documents
through the host codec, op and handle as b sent them).  After every batch: handles,
statuses, released addresses and the run count; after every tick: every output list,
the counters, kwok_engine_stats and the pod state."""
import json

import numpy as np
import pytest

import watch_frames as wf
from gpu_common import compare
from harness import pod_doc
from kwok_amd import abi
from kwok_amd.codec import Codec
from kwok_amd.controller import NOT_SENT, ingest_pod_runs
from kwok_amd.engine import Engine, KwokError, make_config
from oracle.oracle import Oracle
from test_once_gpu import compare_once

pytestmark = pytest.mark.gpu

T0 = 1704067230
KW = dict(cidr="10.0.0.1/16", node_ip="196.168.0.1", buckets=64, node_slots_per_bucket=32, pod_slots_per_bucket=512)
SPECS = [([("fake-pod", "fake")], [], []),
         ([("a", "img-a"), ("b", "img/b:v2")], [("init", "busybox")], ["g.io/x"])]
BOOKMARK = b'{"type":"BOOKMARK","object":{"kind":"Pod","metadata":{"resourceVersion":"9"}}}\n'


def spec_of(k):
    c, i, g = SPECS[k]
    return {"containers": [list(x) for x in c], "init": [list(x) for x in i], "gates": list(g)}


class Lock:
    def __init__(self, once=False, seed=7, enable_cni=False, **geom):
        self.kw = dict(KW, **geom)
        self.once = once
        self.a = Engine(make_config(heartbeat_once=once, enable_cni=enable_cni, **self.kw))
        self.b = Engine(make_config(heartbeat_once=once, enable_cni=enable_cni, **self.kw))
        self.o = Oracle(make_config(enable_cni=enable_cni, **self.kw))
        self.all = (self.a, self.b, self.o)
        ids = [[x.register_pod_spec(*s) for s in SPECS] for x in self.all]
        assert ids[0] == ids[1] == ids[2]
        self.spec_id = {s: ids[0][k] for k, s in enumerate(self.canon(*s) for s in SPECS)}
        self.codec = Codec(manage_all_nodes=True)
        self.a.uid_dir_enable()
        self.stride = self.kw.get("pod_handle_stride") or self.kw["pod_slots_per_bucket"]
        self.n_slots = self.kw["buckets"] * self.stride
        self.by_uid = {}      # b's map
        self.meta = {}        # uid -> doc()'s arguments (a relist restates the pod)
        self.node_handle = {}
        self.now = T0
        self.rng = np.random.default_rng(seed)

    @staticmethod
    def canon(c, i, g):
        return (tuple(tuple(x) for x in c), tuple(tuple(x) for x in i), tuple(g))

    def close(self):
        for x in self.all:
            x.close()
        self.codec.close()

    def nodes(self, names, managed=1):
        ar = abi.Arena()
        ev = np.zeros(len(names), abi.NODE_EVENT_DTYPE)
        ev["op"], ev["managed"], ev["lockable"] = abi.OP_UPSERT, managed, 1
        for i, n in enumerate(names):
            ev[i]["name"] = ar.ref(n)
        got = [x.ingest_nodes_raw(ev, bytes(ar.buf)) for x in self.all]
        for h, s in got[1:]:
            assert (h == got[0][0]).all() and (s == got[0][1]).all()
        assert not got[0][1].any()
        self.node_handle.update(zip(names, (int(h) for h in got[0][0])))
        return got[0][0]

    # ---- one batch: lines = [(type, document bytes)] ---------------------------------
    def batch(self, lines, where, as_list=False, want_runs=None, want_domain=0):
        docs = [d for _t, d in lines]
        if as_list:
            assert all(t == "ADDED" for t, _d in lines)
            stream = b'{"kind":"PodList","apiVersion":"v1","metadata":{"resourceVersion":"7"},"items":[' + b",".join(docs) + b"]}"
            fa, _ia, _nha, sa = self.a.frame_list(stream)
            fb, _ib, _nhb, sb = self.b.frame_list(stream)
        else:
            stream = b"".join(d if t == "RAW" else wf.wrap(d, t) for t, d in lines)
            fa, _ua, _nha, sa = self.a.frame_watch(stream)
            fb, _ub, _nhb, sb = self.b.frame_watch(stream)
        assert fa.tobytes() == fb.tobytes() and len(fa) == len(lines)
        n = len(fa)
        # a: one call
        ha, sta, rela, nha, runs_a = self.a.ingest_pods_framed_uid(self.codec, sa, np.arange(n))
        # b: the host path.  Frames the controller never sends are answered here by the rules of kwok_watch.h
        hb = np.full(n, -1, np.int32)
        stb = np.full(n, abi.EINVAL, np.int32)
        relb = np.zeros(n, np.uint32)
        keep, uids, deleted = [], [], []
        for i, f in enumerate(fb):
            if f["status"] != abi.OK or f["type"] not in (abi.WATCH_ADDED, abi.WATCH_MODIFIED, abi.WATCH_DELETED):
                continue
            ul = int(f["uid"]["len"])
            if (f["flags"] & abi.FRAME_ESC_UID) or ul == 0 or ul > abi.UID_MAX:
                stb[i] = abi.EDOMAIN
                continue
            keep.append(i)
            uids.append(bytes(stream[int(f["uid"]["off"]):int(f["uid"]["off"]) + ul]))
            deleted.append(f["type"] == abi.WATCH_DELETED)
        keep = np.array(keep, np.int64)
        rel_keep = np.zeros(len(keep), np.uint32)
        n_host_b = [0]
        dec = self.codec.decode_pods([docs[i] for i in keep], strict=False) if len(keep) else None

        def send(idx, ops, hv):
            h1, s1, r1, nh = self.b.ingest_pods_framed(self.codec, sb, keep[idx].astype(np.uint32), hv.astype(np.int32))
            n_host_b[0] += nh
            rel_keep[idx] = r1
            # the oracle: the same records, decoded by the host codec
            recs = np.zeros(len(idx), abi.POD_EVENT_DTYPE)
            for q, k in enumerate(idx):
                assert dec.status[k] == abi.OK
                d = dec.pods[k]
                recs[q] = np.frombuffer(bytes(d.ev), abi.POD_EVENT_DTYPE)[0]
                if ops[q] == abi.OP_UPSERT:
                    sp = self.canon([(dec.text(c.name), dec.text(c.image)) for c in d.containers[:d.n_containers]],
                                    [(dec.text(c.name), dec.text(c.image)) for c in d.init_containers[:d.n_init_containers]],
                                    [dec.text(g) for g in d.readiness_gates[:d.n_readiness_gates]])
                    recs[q]["spec_id"] = self.spec_id[sp]
                recs[q]["node_handle"] = -1
            recs["op"], recs["handle"] = ops, hv
            h2, s2, r2 = self.o.ingest_pods_raw(recs, bytes(dec.buf))
            assert list(h2) == list(h1) and list(s2) == list(s1) and list(r2) == list(r1), where + " (b / oracle)"
            return h1, s1

        if len(keep):
            hk, sk, runs_b = ingest_pod_runs(self.b, self.by_uid, np.empty(len(keep)), uids, deleted, None, sender=send)
            hb[keep], stb[keep], relb[keep] = hk, sk, rel_keep
        else:
            runs_b = 0
        assert list(sta) == list(stb), "%s statuses\n%r\n%r" % (where, list(sta), list(stb))
        assert list(ha) == list(hb), "%s handles\n%r\n%r" % (where, list(ha), list(hb))
        assert list(rela) == list(relb), where + " released"
        assert runs_a == runs_b, "%s runs %d vs %d" % (where, runs_a, runs_b)
        assert nha == n_host_b[0], where + " documents the host decided"
        wa, wb = self.a.watch_stats(), self.b.watch_stats()
        assert wa == wb, "%s watch stats %r vs %r" % (where, wa, wb)
        if want_runs is not None:
            assert runs_a == want_runs, "%s: %d runs" % (where, runs_a)
        assert int((sta == abi.EDOMAIN).sum()) == want_domain, "%s: %r" % (where, list(sta))
        # the directory answers as b's map does (which names every handle once: the batches keep it coherent)
        assert len(set(self.by_uid.values())) == len(self.by_uid), where + " b's map"
        us = sorted(set(uids) | set(self.by_uid))
        if us:
            assert list(self.a.uid_lookup(us)) == [self.by_uid.get(u, -1) for u in us], where + " lookups"
        self.state(where)
        return ha, sta, rela

    def forget(self, handles):
        """pods the tick or a sweep removed leave b's map (Controller._tick / _end_resync)"""
        gone = set(int(h) for h in handles)
        for u in [u for u, h in self.by_uid.items() if h in gone]:
            del self.by_uid[u]

    def state(self, where):
        da, db, do = (x.dump_pods(0, self.n_slots) for x in self.all)
        for k, what in enumerate(("used", "phase", "hostIP", "podIP")):
            assert (da[k] == db[k]).all(), "%s: pod %s differs from the host-map engine" % (where, what)
            assert (da[k] == do[k]).all(), "%s: pod %s differs from the oracle" % (where, what)

    def tick(self, where):
        for x in self.all:
            x.tick(self.now, read=False)
        self.now += 30
        ao, bo = (x.read_outputs(heartbeat_once=self.once) for x in (self.a, self.b))
        oo = self.o.read_outputs()
        (compare_once if self.once else compare)(ao, oo, where)
        assert list(ao.heartbeat_nodes) == list(bo.heartbeat_nodes), where
        assert ao.node_inits == bo.node_inits and ao.pod_patches == bo.pod_patches and ao.deletes == bo.deletes, where
        assert ao.counters == bo.counters, where
        assert self.a.stats() == self.b.stats(), "%s: tick kernels %r vs %r" % (where, self.a.stats(), self.b.stats())
        self.forget(h for h, _f in ao.deletes)
        self.state(where)
        return ao

    # ---- documents -----------------------------------------------------------------
    def doc(self, key, node="node-000", spec=0, uid=None, **kw):
        """the pod's document as the apiserver would send it now: the address and phase the engine gave it"""
        ev = dict(key=key, node=node, disregard=False, deleting=False, finalizers=0, creation=T0 - 90, phase="Pending",
                  status_nonempty=False, conforms=False, hostIP="", podIP="",
                  spec=spec if isinstance(spec, dict) else spec_of(spec))
        ukey = ("u-" + key if uid is None else uid).encode()
        self.meta[ukey] = (key, node, spec, uid)
        h = self.by_uid.get(ukey, -1)
        if h >= 0:
            used, phase, hip, pip = self.o.dump_pods(h, 1)
            if used[0] and phase[0] == abi.PHASE_RUNNING:
                ev.update(phase="Running", status_nonempty=True, conforms=True)
            if used[0] and hip[0]:
                ev["hostIP"] = abi.ip4s(int(hip[0]))
            if used[0] and pip[0]:
                ev["podIP"] = abi.ip4s(int(pip[0]))
        ev.update(kw)
        d = pod_doc(ev)
        if uid is not None:
            d["metadata"]["uid"] = uid
        return json.dumps(d, separators=(",", ":")).encode()


def fleet(t, n_nodes=12):
    names = ["node-%03d" % i for i in range(n_nodes)]
    t.nodes(names)
    return names


@pytest.mark.parametrize("once", [True, False], ids=["heartbeat-once", "full-body"])
def test_named_batches(once):
    t = Lock(once=once)
    names = fleet(t)
    node = lambda k: names[k % len(names)]  # noqa: E731
    # creates only; modifies of known pods
    t.batch([("ADDED", t.doc("p%d" % k, node(k), spec=k % 2)) for k in range(60)], "creates", want_runs=1)
    t.tick("creates")
    t.tick("steady")
    t.batch([("MODIFIED", t.doc("p%d" % k, node(k), spec=k % 2)) for k in range(0, 60, 3)], "modifies", want_runs=1)
    # Added + Modified of a new pod: 2 runs
    t.batch([("ADDED", t.doc("am", node(1))), ("MODIFIED", t.doc("am", node(1), status_nonempty=True))], "added+modified",
            want_runs=2)
    t.tick("added+modified")
    # Added + Deleted of a new pod, with its podIP release (a pod that arrives holding an address of the CIDR)
    _h, _s, rel = t.batch([("ADDED", t.doc("ad", node(2), podIP="10.0.200.7", hostIP="196.168.0.1", phase="Running",
                                           status_nonempty=True)),
                           ("DELETED", t.doc("ad", node(2), podIP="10.0.200.7", hostIP="196.168.0.1", phase="Running",
                                             status_nonempty=True))], "added+deleted", want_runs=2)
    assert rel[1] == abi.ip4("10.0.200.7")
    t.tick("added+deleted")
    # X added, X deleted, Y added on one node: Y takes the slot X freed only because the cut is positional
    h, s, _r = t.batch([("ADDED", t.doc("x", node(3))), ("DELETED", t.doc("x", node(3))), ("ADDED", t.doc("y", node(3)))],
                       "slot order", want_runs=2)
    assert not s.any() and h[0] == h[1] == h[2]
    # three new pods repeating at different positions
    seq = ["r0", "r1", "p3", "r1", "r2", "p6", "r0", "r2", "p9", "r2"]
    t.batch([("MODIFIED" if k in seq[:i] or k.startswith("p") else "ADDED", t.doc(k, node(int(k[1:]))))
             for i, k in enumerate(seq)], "repeats", want_runs=3)
    t.tick("repeats")
    # Deleted of an unknown uid: not sent (alone: no run at all), beside others: one run
    h, s, _r = t.batch([("DELETED", t.doc("never", node(0)))], "unknown deleted alone", want_runs=0)
    assert list(s) == [NOT_SENT] and list(h) == [-1]
    h, s, _r = t.batch([("DELETED", t.doc("never", node(0))), ("MODIFIED", t.doc("p1", node(1), spec=1)),
                        ("DELETED", t.doc("never2", node(0)))], "unknown deleted", want_runs=1)
    assert list(s) == [NOT_SENT, 0, NOT_SENT]
    # Deleted then Added of a known uid in one run: both carry its handle (the Added finds the slot freed)
    h, s, _r = t.batch([("DELETED", t.doc("p4", node(4))), ("ADDED", t.doc("p4", node(4)))], "deleted+added known", want_runs=1)
    assert s[0] == 0 and s[1] == abi.ENOTFOUND and h[0] >= 0
    # a create rejected with KWOK_EDOMAIN (a bad IP), then a second event of that uid: new again, no cut needed twice
    h, s, _r = t.batch([("ADDED", t.doc("badip", node(5), podIP="10.0.0.999")), ("MODIFIED", t.doc("badip", node(5))),
                        ("MODIFIED", t.doc("badip", node(5), status_nonempty=True))], "rejected create", want_runs=3, want_domain=1)
    assert list(s) == [abi.EDOMAIN, 0, 0] and h[0] == -1 and h[1] == h[2] >= 0
    # an escaped uid and an empty one: never guessed
    h, s, _r = t.batch([("ADDED", t.doc("esc", node(6), uid="u\\u002desc")), ("ADDED", t.doc("p7", node(7), spec=1)),
                        ("ADDED", t.doc("empty", node(6), uid="")), ("ADDED", t.doc("long", node(6), uid="L" * 41)),
                        ("ADDED", t.doc("max", node(6), uid="M" * 40))], "uids outside the domain", want_runs=1, want_domain=3)
    assert list(s) == [abi.EDOMAIN, 0, abi.EDOMAIN, abi.EDOMAIN, 0]
    # frames that are no pod events: KWOK_EINVAL, as kwok_ingest_pods_framed
    h, s, _r = t.batch([("RAW", BOOKMARK), ("ADDED", t.doc("after-bookmark", node(8))), ("RAW", b'{"type":"ADDED","object":[]}\n'),
                        ("RAW", b"\r\n")], "non-ingestible frames", want_runs=1)
    assert list(s) == [abi.EINVAL, 0, abi.EINVAL, abi.EINVAL]
    t.tick("rejects")
    # a Deleted line for a pod the tick already removed
    t.batch([("MODIFIED", t.doc("p%d" % k, node(k), spec=k % 2, deleting=True)) for k in (10, 11, 13)], "deletion-marked", want_runs=1)
    out = t.tick("tick deletes")
    assert len(out.deletes) == 3
    h, s, _r = t.batch([("DELETED", t.doc("p%d" % k, node(k), spec=k % 2)) for k in (10, 11, 13)], "deleted after the tick",
                       want_runs=0)
    assert list(s) == [NOT_SENT] * 3
    # re-Added after a sweep: a relist that holds every pod but three, which come back as new pods
    live = sorted(t.by_uid.items(), key=lambda kv: kv[1])
    absent = [kv for kv in live if kv[0] in (b"u-p20", b"u-p21", b"u-am")]
    assert len(absent) == 3
    for x in (t.a, t.b):
        x.resync_begin(abi.KIND_PODS)
    def restate(u):
        key, nd, sp, uid = t.meta[u]
        return ("ADDED", t.doc(key, nd, spec=sp, uid=uid))

    t.batch([restate(u) for u, h in live if (u, h) not in absent], "relist", as_list=True, want_runs=1)
    sa, rela, _nd = t.a.resync_sweep(abi.KIND_PODS)
    sb, relb, _nd = t.b.resync_sweep(abi.KIND_PODS)
    assert list(sa) == list(sb) == sorted(h for _u, h in absent) and list(rela) == list(relb)
    ar = abi.Arena()
    ev = np.zeros(len(sa), abi.POD_EVENT_DTYPE)
    ev["op"], ev["handle"] = abi.OP_DELETE, sa
    for i, ip in enumerate(rela):
        if ip:
            ev[i]["pod_ip"] = ar.ref(abi.ip4s(int(ip)))
    assert not t.o.ingest_pods_raw(ev, bytes(ar.buf))[1].any()
    t.forget(sa)
    t.state("swept")
    h, s, _r = t.batch([restate(u) for u, _h in absent], "re-added after the sweep", want_runs=1)
    assert not s.any() and len(set(h)) == 3
    t.tick("after the sweep")
    t.tick("quiet")
    s = t.a.uid_stats()
    assert s["cuts"] >= 7 and s["runs"] >= s["cuts"] and s["unbound"] == 0 and s["hits"] > 0
    t.close()


def test_list_items_and_host_documents():
    """List items through kwok_frame_list_gpu; a pod spec not registered yet, which the host codec completes
    (its handle comes back from the device for it)"""
    t = Lock(once=True)
    names = fleet(t, 6)
    late = {"containers": [["late", "img:2"]], "init": [], "gates": []}
    t.spec_id[Lock.canon([("late", "img:2")], [], [])] = t.o.register_pod_spec([("late", "img:2")], [], [])  # (the engines: as it appears)
    t.batch([("ADDED", t.doc("l%d" % k, names[k % 6], spec=k % 2)) for k in range(40)], "list page", as_list=True, want_runs=1)
    t.tick("listed")
    h, s, _r = t.batch([("ADDED", t.doc("l3", names[3], spec=1)), ("ADDED", t.doc("host-0", names[0], spec=late)),
                        ("ADDED", t.doc("l39", names[3], spec=1)), ("ADDED", t.doc("host-0", names[0], spec=late))],
                       "page with known pods and a new spec", as_list=True, want_runs=2)
    assert not s.any() and h[1] == h[3]
    t.tick("after")
    t.close()


def test_enable_cni():
    t = Lock(once=True, enable_cni=True)
    names = fleet(t, 6)
    h, s, _r = t.batch([("ADDED", t.doc("c%d" % k, names[k % 6])) for k in range(30)] +
                       [("MODIFIED", t.doc("c7", names[1], status_nonempty=True))], "cni creates", want_runs=2)
    assert not s.any()
    pend = [np.sort(x.cni_pending()) for x in t.all]
    assert list(pend[0]) == list(pend[1]) == list(pend[2]) and len(pend[0]) == 30
    ips = [abi.ip4("10.0.%d.%d" % (1 + i // 200, 2 + i % 200)) for i in range(30)]
    for x in t.all:
        x.cni_assign(pend[0], ips)
    t.tick("cni assigned")
    _h, s, rel = t.batch([("DELETED", t.doc("c%d" % k, names[k % 6])) for k in range(0, 30, 2)] +
                         [("DELETED", t.doc("nobody", names[0]))], "cni deletes", want_runs=1)
    assert list(s) == [0] * 15 + [NOT_SENT] and not rel.any()  # (EnableCNI: nothing goes back to the pool)
    t.tick("cni after")
    t.close()


def test_block_and_wave_edges():
    """1, 255, 256, 257 and 1025 records (one thread per record, 256 per block): all creates, then the same
    pods deleted with one of them named twice (both resolve at the start of the run: the second finds the slot freed)"""
    t = Lock(once=True)
    names = fleet(t, 24)
    first = 0
    for n in (1, 255, 256, 257, 1025):
        keys = ["e%d" % k for k in range(first, first + n)]
        first += n
        h, s, _r = t.batch([("ADDED", t.doc(k, names[i % 24])) for i, k in enumerate(keys)], "%d creates" % n, want_runs=1)
        assert not s.any() and len(set(h)) == n
        h2, s2, _r = t.batch([("DELETED", t.doc(k, names[i % 24])) for i, k in enumerate(keys + keys[-1:])], "%d deletes" % n,
                             want_runs=1)
        assert list(h2[:n]) == list(h) and list(s2) == [0] * n + [abi.ENOTFOUND]
    t.tick("edges")
    t.close()


@pytest.mark.parametrize("once", [True, False], ids=["heartbeat-once", "full-body"])
def test_fuzz(once):
    """~2000 events over 300 uids, all three types, in 8 batches with a tick between them.  Any type meets
    any state (Added of a known pod, Modified and Deleted of unknown ones); a uid comes back in later
    batches.  Within one batch nothing follows a uid's DELETED line, as on a real watch: an event after it
    in the same run would carry the handle resolved at the run's start, and where another create took the
    freed slot meanwhile the host map ends with two uids on one handle - a state of the yardstick itself
    that no directory keyed by the slot can hold."""
    t = Lock(once=once, seed=11)
    names = fleet(t, 16)
    rng = t.rng
    total = 0
    for r in range(8):
        n = int(rng.integers(240, 340))
        lines, gone = [], set()
        for _ in range(n):
            k = int(rng.integers(0, 300))
            typ = ("ADDED", "MODIFIED", "MODIFIED", "DELETED")[int(rng.integers(0, 4))]
            kw = dict(status_nonempty=True) if rng.integers(0, 2) else {}
            if k in gone:
                continue
            if typ == "DELETED":
                gone.add(k)
            lines.append((typ, t.doc("f%d" % k, names[k % 16], spec=k % 2, **kw)))
        t.batch(lines, "fuzz batch %d" % r)
        total += len(lines)
        t.tick("fuzz tick %d" % r)
    s = t.a.uid_stats()
    assert total > 1600 and s["cuts"] > 10 and s["lookups"] >= total
    t.close()


def test_call_level_errors():
    e = Engine(make_config(**KW))
    codec = Codec(manage_all_nodes=True)
    stream = wf.wrap(json.dumps(pod_doc(dict(key="k", node="n", disregard=False, deleting=False, finalizers=0, creation=T0,
                                             phase="Pending", status_nonempty=False, conforms=False, hostIP="", podIP="",
                                             spec=spec_of(0)))).encode(), "ADDED")
    _f, _u, _n, sid = e.frame_watch(stream)
    with pytest.raises(KwokError) as ei:  # the directory is not enabled
        e.ingest_pods_framed_uid(codec, sid, [0])
    assert ei.value.code == abi.EINVAL
    e.uid_dir_enable()
    for bad in (0, sid + 1):
        with pytest.raises(KwokError) as ei:
            e.ingest_pods_framed_uid(codec, bad, [0])
        assert ei.value.code == abi.EINVAL
    h, s, _r, _nh, runs = e.ingest_pods_framed_uid(codec, sid, [0, 0, 5, 4000000000])
    assert list(s) == [0, 0, abi.EINVAL, abi.EINVAL] and h[0] == h[1] >= 0 and runs == 2
    assert e.ingest_pods_framed_uid(codec, sid, [])[4] == 0
    e.close()
