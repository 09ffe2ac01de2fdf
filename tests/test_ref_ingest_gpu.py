"""GPU: the reference directory behind the by-uid and echo ingests (include/kwok_watch.h,
DESIGN.md §25; refs.hip: k_refs_note, k_refs_size, k_refs_gather; kwok_read_refs).

Engine `a` runs with the directory, engine `b` without it (its uid directory, and for
the echo entry its ledger, enabled); both are fed the same calls.  The test keeps
handle -> (namespace, name, uid) from the frames and a's own results: an OK create adds
an entry, an OK delete, a tick delete or a sweep removes one.  After every batch:
kwok_refs_lookup of every live handle.  After every tick: kwok_read_refs of all four
lists, whole and in ranges of 1 and of 256, against the dict - the delete list before
its entries leave it.  And a's results, outputs, counters and pod state equal b's: the
directory changes nothing else.  Every comparison is byte for byte."""
import json
import zlib

import numpy as np
import pytest

import watch_frames as wf
from harness import pod_doc
from kwok_amd import abi
from kwok_amd.codec import Codec
from kwok_amd.controller import NOT_SENT
from kwok_amd.engine import Engine, KwokError, make_config
from test_ref_dir_gpu import check_layout

pytestmark = pytest.mark.gpu

T0 = 1704067230
KW = dict(cidr="10.0.0.1/16", node_ip="196.168.0.1", buckets=64, node_slots_per_bucket=32, pod_slots_per_bucket=512)
SPEC = {"containers": [["fake-pod", "fake"]], "init": [], "gates": []}
NONE = (abi.REF_NONE, b"", b"")
LISTS = (abi.REFS_HEARTBEAT, abi.REFS_NODE_INIT, abi.REFS_POD_PATCH, abi.REFS_DELETE)


class RefLock:
    def __init__(self, once=False, entry="uid", enable_cni=False, seed=5, **geom):
        self.kw = dict(KW, **geom)
        self.once, self.entry = once, entry
        self.a = Engine(make_config(heartbeat_once=once, enable_cni=enable_cni, **self.kw))
        self.b = Engine(make_config(heartbeat_once=once, enable_cni=enable_cni, **self.kw))
        self.both = (self.a, self.b)
        self.spec = [x.register_pod_spec([("fake-pod", "fake")], [], []) for x in self.both][0]
        self.codec = Codec(manage_all_nodes=True)
        self.a.refs_enable()
        self.b.uid_dir_enable()
        if entry == "echo":
            for x in self.both:
                x.echo_enable()
        self.stride = self.kw.get("pod_handle_stride") or self.kw["pod_slots_per_bucket"]
        self.n_slots = self.kw["buckets"] * self.stride
        self.by_uid = {}     # uid -> handle of the live pods that have one
        self.live = {}       # handle -> (namespace, name, uid): the yardstick (name b"": none stored)
        self.last = {}       # handle -> what its slot last stored, live or not
        self.node_name = {}  # node handle -> name
        self.now = T0
        self.rng = np.random.default_rng(seed)

    def close(self):
        for x in self.both:
            x.close()
        self.codec.close()

    def nodes(self, names, managed=1):
        ar = abi.Arena()
        ev = np.zeros(len(names), abi.NODE_EVENT_DTYPE)
        ev["op"], ev["managed"], ev["lockable"] = abi.OP_UPSERT, managed, 1
        for i, n in enumerate(names):
            ev[i]["name"] = ar.ref(n)
        (ha, sa), (hb, sb) = (x.ingest_nodes_raw(ev, bytes(ar.buf)) for x in self.both)
        assert list(ha) == list(hb) and not sa.any() and not sb.any()
        self.node_name.update(zip((int(h) for h in ha), (n.encode() for n in names)))
        return ha

    @staticmethod
    def uid_of(ns, name):
        return "u-%08x-%d" % (zlib.crc32(("%s/%s" % (ns, name)).encode()), len(name))

    @staticmethod
    def doc(name, node="node-000", ns="default", uid=None, **kw):
        ev = dict(key=name, node=node, disregard=False, deleting=False, finalizers=0, creation=T0 - 90, phase="Pending",
                  status_nonempty=False, conforms=False, hostIP="", podIP="", spec=SPEC)
        ev.update(kw)
        d = pod_doc(ev)
        d["metadata"]["namespace"] = ns
        d["metadata"]["uid"] = RefLock.uid_of(ns, name) if uid is None else uid
        return json.dumps(d, separators=(",", ":")).encode()

    def set_pod(self, h, ref):
        self.live[h] = ref
        self.last[h] = ref

    def drop(self, handles):
        for h in handles:
            ref = self.live.pop(int(h))
            self.by_uid.pop(ref[2], None)

    # ---- one batch of frames through the entry under test: lines = [(type, document bytes)] ----
    def batch(self, lines, where, as_list=False):
        docs = [d for _t, d in lines]
        if as_list:
            stream = b'{"kind":"PodList","apiVersion":"v1","metadata":{"resourceVersion":"7"},"items":[' + b",".join(docs) + b"]}"
            (fa, _i, _n, sa), (fb, _i2, _n2, sb) = (x.frame_list(stream) for x in self.both)
        else:
            stream = b"".join(d if t == "RAW" else wf.wrap(d, t) for t, d in lines)
            (fa, _u, _n, sa), (fb, _u2, _n2, sb) = (x.frame_watch(stream) for x in self.both)
        assert fa.tobytes() == fb.tobytes() and len(fa) == len(lines)
        idx = np.arange(len(fa))
        if self.entry == "echo":
            ra, rb = (x.ingest_pods_framed_echo(self.codec, s, idx) for x, s in ((self.a, sa), (self.b, sb)))
        else:
            ra, rb = (x.ingest_pods_framed_uid(self.codec, s, idx) for x, s in ((self.a, sa), (self.b, sb)))
        for p, q in zip(ra, rb):  # handles, statuses, released, documents the host decided, runs (, echoes)
            assert np.array_equal(p, q), "%s: the directory changed a result" % where
        ha, sta = ra[0], ra[1]
        span = lambda f, k: bytes(stream[int(f[k]["off"]):int(f[k]["off"]) + int(f[k]["len"])])  # noqa: E731
        created = []
        for i, f in enumerate(fa):
            if sta[i] != abi.OK or f["type"] not in (abi.WATCH_ADDED, abi.WATCH_MODIFIED, abi.WATCH_DELETED):
                continue
            uid, h = span(f, "uid"), int(ha[i])
            if f["type"] == abi.WATCH_DELETED:
                assert self.by_uid.get(uid) == h, where
                self.drop([h])
            elif uid not in self.by_uid:  # an OK create
                assert h not in self.live, where
                named = (not (f["flags"] & (abi.FRAME_ESC_NAME | abi.FRAME_ESC_NS)) and 0 < int(f["name"]["len"]) <= abi.REF_NAME_MAX
                         and int(f["namespace_"]["len"]) <= abi.REF_NS_MAX)
                self.by_uid[uid] = h
                self.set_pod(h, (span(f, "namespace_"), span(f, "name"), uid) if named else (b"", b"", uid))
                created.append(i)
            else:
                assert self.by_uid[uid] == h, where
        self.lookups(where)
        return ha, sta, created

    def expect(self, h, any_slot=True):
        ref = self.live.get(int(h)) or (self.last.get(int(h)) if any_slot else None)
        if ref is None:
            return (abi.ENOTFOUND, b"", b"", b"")
        return (abi.OK,) + ref if ref[1] else (abi.REF_NONE, b"", b"", ref[2])

    def lookups(self, where):
        """every live handle, and the freed ones without and with KWOK_REFS_ANY_SLOT"""
        hs = list(self.live)
        refs, blob = self.a.refs_lookup(abi.KIND_PODS, hs)
        check_layout(refs, blob, where)
        assert Engine.ref_items(refs, blob) == [self.expect(h) for h in hs], where + " lookups"
        freed = [h for h in self.last if h not in self.live]
        if freed:
            refs, blob = self.a.refs_lookup(abi.KIND_PODS, freed)
            assert Engine.ref_items(refs, blob) == [(abi.ENOTFOUND, b"", b"", b"")] * len(freed), where + " freed"
            refs, blob = self.a.refs_lookup(abi.KIND_PODS, freed, abi.REFS_ANY_SLOT)
            assert Engine.ref_items(refs, blob) == [self.expect(h) for h in freed], where + " freed, any slot"

    def state(self, where):
        da, db = (x.dump_pods(0, self.n_slots) for x in self.both)
        for k, what in enumerate(("used", "phase", "hostIP", "podIP")):
            assert (da[k] == db[k]).all(), "%s: pod %s differs from the engine without the directory" % (where, what)
        ua, ub = self.a.uid_stats(), self.b.uid_stats()
        assert ua == ub, "%s uid stats %r vs %r" % (where, ua, ub)
        assert self.a.watch_stats() == self.b.watch_stats(), where
        if self.entry == "echo":
            assert self.a.echo_stats() == self.b.echo_stats(), where

    def read_list(self, which, want, where):
        """the whole list, then ranges of 256 and of 1"""
        n = len(want)
        refs, blob = self.a.read_refs(which, 0, n)
        check_layout(refs, blob, where)
        assert Engine.ref_items(refs, blob) == want, "%s: list %d" % (where, which)
        for step in (256, 1):
            if n <= step and step != 1:
                continue
            got = []
            for lo in range(0, n, step) if step != 1 else sorted(set([0, n // 2, n - 1]) if n else []):
                cnt = min(step, n - lo)
                refs, blob = self.a.read_refs(which, lo, cnt)
                check_layout(refs, blob, where)
                part = Engine.ref_items(refs, blob)
                assert part == want[lo:lo + cnt], "%s: list %d range [%d, +%d)" % (where, which, lo, cnt)
                got += part
            assert step == 1 or got == want
        for first, count in ((n + 1, 0), (n, 1), (0, n + 1)):  # a range outside the list
            with pytest.raises(KwokError) as ei:
                self.a.read_refs(which, first, count)
            assert ei.value.code == abi.EINVAL, where
        refs, blob = self.a.read_refs(which, n, 0)  # the empty range at its end
        assert len(refs) == 0 and len(blob) == 0

    def tick(self, where, read=True):
        for x in self.both:
            x.tick(self.now, read=False)
        self.now += 30
        ao, bo = (x.read_outputs(heartbeat_once=self.once) for x in self.both)
        assert list(ao.heartbeat_nodes) == list(bo.heartbeat_nodes), where
        assert ao.node_inits == bo.node_inits and ao.pod_patches == bo.pod_patches and ao.deletes == bo.deletes, where
        assert ao.counters == bo.counters and ao.arena == bo.arena, where
        assert self.a.stats() == self.b.stats(), "%s: tick kernels %r vs %r" % (where, self.a.stats(), self.b.stats())
        if read:
            node = lambda h: (abi.OK, b"", self.node_name[int(h)], b"")  # noqa: E731
            self.read_list(abi.REFS_HEARTBEAT, [node(h) for h in ao.heartbeat_nodes], where)
            self.read_list(abi.REFS_NODE_INIT, [node(h) for h, _b in ao.node_inits], where)
            self.read_list(abi.REFS_POD_PATCH, [self.expect(h) for h, _b in ao.pod_patches], where)
            # the delete list, before its entries leave the dict: the tick freed these pods, their bytes stay
            self.read_list(abi.REFS_DELETE, [self.expect(h) for h, _f in ao.deletes], where)
            assert all(self.expect(h)[0] != abi.ENOTFOUND for h, _f in ao.deletes), where
        self.drop(h for h, _f in ao.deletes)
        if read:  # ... and after: still answered (the slots were not created into)
            self.read_list(abi.REFS_DELETE, [self.expect(h) for h, _f in ao.deletes], where + " (popped)")
        self.state(where)
        self.lookups(where)
        return ao


def fleet(t, n=12):
    names = ["node-%03d" % i for i in range(n)]
    t.nodes(names)
    return names


NAMES = [("n", "a"), ("default", "x" * 15), ("default", "x" * 16), ("default", "x" * 17), ("d" * 63, "p" * 253),
         ("kube-system", "same-in-all-but-the-last-byte-A"), ("kube-system", "same-in-all-but-the-last-byte-B"),
         ("default", "q" * 20), ("default", "q" * 21), ("default", "q" * 22)]


@pytest.mark.parametrize("entry", ["uid", "echo"])
@pytest.mark.parametrize("once", [True, False], ids=["heartbeat-once", "full-body"])
def test_named_batches(once, entry):
    t = RefLock(once=once, entry=entry)
    names = fleet(t)
    node = lambda k: names[k % len(names)]  # noqa: E731
    # watch lines: names and namespaces of every length the record's units distinguish
    t.batch([("ADDED", t.doc(nm, node(k), ns=ns)) for k, (ns, nm) in enumerate(NAMES)], "watch creates")
    assert len(t.live) == len(NAMES) and all(r[1] for r in t.live.values())
    t.tick("watch creates")
    # List items; known pods' upserts store nothing (a relist restates them under names that would differ if stored)
    t.batch([("ADDED", t.doc("list-%d" % k, node(k), ns="ns-%d" % (k % 3))) for k in range(30)], "list creates", as_list=True)
    t.batch([("MODIFIED", t.doc(nm, node(k), ns=ns, status_nonempty=True)) for k, (ns, nm) in enumerate(NAMES)], "upserts")
    t.tick("list creates")
    n0 = t.a.refs_stats()
    assert n0["notes"] == len(NAMES) + 30 and n0["unnamed"] == 0 and n0["binds"] == 0
    # a Deleted line, then a create that reuses the slot: the new pod's name, not the old one's
    h0, s0, _c = t.batch([("DELETED", t.doc("list-3", node(3), ns="ns-0"))], "deleted")
    h1, s1, _c = t.batch([("ADDED", t.doc("successor", node(3), ns="other"))], "slot reused")
    assert not s0.any() and not s1.any() and h0[0] == h1[0] and t.live[int(h1[0])][:2] == (b"other", b"successor")
    # X added, X deleted, Y added in one call: two runs, Y holds X's slot under its own name
    h, s, _c = t.batch([("ADDED", t.doc("x", node(4))), ("DELETED", t.doc("x", node(4))), ("ADDED", t.doc("y", node(4)))], "x, -x, y")
    assert not s.any() and h[0] == h[1] == h[2] and t.live[int(h[2])][1] == b"y"
    t.tick("slot order")
    # frames whose name or namespace holds an escape: the codec keeps them out (not a safe string), nothing is created;
    # names over the limits: created without a name, never truncated
    esc = [("escXname", "default"), ("plain", "escXns"), ("L" * 254, "default"), ("ok-name", "N" * 64)]
    h, s, created = t.batch([("ADDED", t.doc(nm, node(k), ns=ns, uid="u-esc-%d" % k).replace(b"escX", b"esc\\u002d"))
                             for k, (nm, ns) in enumerate(esc)], "escaped")
    assert list(s) == [abi.EDOMAIN, abi.EDOMAIN, 0, 0] and created == [2, 3]
    assert all(t.live[int(x)][:2] == (b"", b"") for x in h[2:])
    refs, blob = t.a.refs_lookup(abi.KIND_PODS, h[2:])
    assert [it[:3] for it in Engine.ref_items(refs, blob)] == [NONE] * 2
    assert (refs["uid_len"] == 7).all()  # (the uid is still given)
    assert t.a.refs_stats()["unnamed"] == 2
    # ... the caller ingests the escaped ones as typed events and binds the decoded text and the uid
    nh = [k for k, v in t.node_name.items() if v == node(5).encode()][0]
    ev = np.zeros(2, abi.POD_EVENT_DTYPE)
    ev["op"], ev["handle"], ev["node_handle"], ev["spec_id"] = abi.OP_UPSERT, -1, nh, t.spec
    ev["creation_unix"], ev["phase"] = T0 - 90, abi.PHASE_PENDING
    (he, se, _r), (he2, se2, _r2) = (x.ingest_pods_raw(ev, b"") for x in t.both)
    assert list(he) == list(he2) and not se.any() and not se2.any()
    for x in t.both:
        assert x.uid_bind(he, [b"u-esc-0", b"u-esc-1"]) == 0
    assert t.a.refs_bind(he, [b"default", b"esc-ns"], [b"esc-name", b"plain"]) == 0
    for x, ns, nm, uid in ((he[0], b"default", b"esc-name", b"u-esc-0"), (he[1], b"esc-ns", b"plain", b"u-esc-1")):
        t.set_pod(int(x), (ns, nm, uid))
        t.by_uid[uid] = int(x)
    t.lookups("escaped names bound")
    assert t.a.refs_stats()["unnamed"] == 4 and t.a.refs_stats()["binds"] == 2
    # a create through the packed record wire in between: no name, no uid; then named
    (hw, sw, _r), (hw2, sw2, _r2) = (x.ingest_pods_packed(abi.pack_pod_events(ev)) for x in t.both)
    assert list(hw) == list(hw2) and not sw.any() and not sw2.any()
    for x in hw:
        t.set_pod(int(x), (b"", b"", b""))
    t.lookups("wire creates")
    assert t.a.refs_bind(hw, [b"wire", b""], [b"w0", b"w1"]) == 0
    t.set_pod(int(hw[0]), (b"wire", b"w0", b""))
    t.set_pod(int(hw[1]), (b"", b"w1", b""))
    t.lookups("wire creates bound")
    t.tick("wire creates")
    # deletion-marked pods, with and without finalizers: the tick's delete list and its finalizer patches
    t.batch([("MODIFIED", t.doc(nm, node(k), ns=ns, deleting=True, finalizers=k % 2)) for k, (ns, nm) in enumerate(NAMES[:6])],
            "deletion-marked")
    out = t.tick("tick deletes")
    assert len(out.deletes) == 6
    # the freed pods' Deleted lines come back: not sent, nothing changes
    h, s, _c = t.batch([("DELETED", t.doc(nm, node(k), ns=ns)) for k, (ns, nm) in enumerate(NAMES[:6])], "late deletes")
    assert list(s) == [NOT_SENT] * 6
    # a sweep: the pods a relist no longer holds
    for x in t.both:
        x.resync_begin(abi.KIND_PODS)
    keep = [k for k in range(30) if k % 4 and k != 3]
    t.batch([("ADDED", t.doc("list-%d" % k, node(k), ns="ns-%d" % (k % 3))) for k in keep], "relist", as_list=True)
    others = [h for h, r in t.live.items() if not r[1].startswith(b"list-")]
    for x in t.both:
        assert x.resync_mark(abi.KIND_PODS, others) == 0
    (swa, _ra, _na), (swb, _rb, _nb) = (x.resync_sweep(abi.KIND_PODS) for x in t.both)
    assert list(swa) == list(swb) and len(swa) == 30 - 1 - len(keep)
    refs, blob = t.a.refs_lookup(abi.KIND_PODS, swa, abi.REFS_ANY_SLOT)  # (asked before the next pod ingest)
    assert Engine.ref_items(refs, blob) == [t.expect(h) for h in swa] and (refs["status"] == abi.OK).all()
    t.drop(swa)
    t.tick("after the sweep")
    t.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_block_edges(n):
    """n creates in one batch (k_refs_note: 32 records per block), the tick that patches them all
    (k_refs_size: 256 items per block, k_refs_gather: 64), then n deletion marks and the tick's delete list"""
    t = RefLock(once=True)
    names = fleet(t, 24)
    keys = [("ns-%d" % (k % 7), "edge-%d-%s" % (k, "z" * (k % 40))) for k in range(n)]
    _h, s, created = t.batch([("ADDED", t.doc(nm, names[k % 24], ns=ns)) for k, (ns, nm) in enumerate(keys)], "%d creates" % n)
    assert not s.any() and len(created) == n
    out = t.tick("%d creates" % n)
    assert len(out.pod_patches) == n
    t.batch([("MODIFIED", t.doc(nm, names[k % 24], ns=ns, deleting=True)) for k, (ns, nm) in enumerate(keys)], "%d marks" % n)
    out = t.tick("%d deletes" % n)
    assert len(out.deletes) == n
    t.close()


def test_enable_cni():
    t = RefLock(once=True, enable_cni=True)
    names = fleet(t, 6)
    t.batch([("ADDED", t.doc("cni-%d" % k, names[k % 6], ns="cni")) for k in range(20)], "cni creates")
    pend = [x.cni_pending() for x in t.both]
    assert list(pend[0]) == list(pend[1]) and len(pend[0]) == 20
    # the pods that wait for an address, by name: what cni.Setup is called with
    refs, blob = t.a.refs_lookup(abi.KIND_PODS, pend[0])
    assert Engine.ref_items(refs, blob) == [t.expect(h, False) for h in pend[0]] and (refs["status"] == abi.OK).all()
    ips = np.arange(20, dtype=np.uint32) + abi.ip4("10.0.3.1")
    for x in t.both:
        assert not x.cni_assign(pend[0], ips).any()
    out = t.tick("cni patches")
    assert len(out.pod_patches) == 20
    t.batch([("MODIFIED", t.doc("cni-%d" % k, names[k % 6], ns="cni", deleting=True)) for k in range(0, 20, 2)], "cni marks")
    out = t.tick("cni deletes")
    assert len(out.deletes) == 10
    t.close()


def test_the_stale_guard():
    t = RefLock(once=True)
    names = fleet(t, 6)
    t.batch([("ADDED", t.doc("g-%d" % k, names[k % 6])) for k in range(12)], "creates")
    t.tick("creates")
    t.batch([("MODIFIED", t.doc("g-%d" % k, names[k % 6], deleting=True)) for k in range(4)], "marks")
    out = t.tick("deletes", read=False)
    assert len(out.deletes) == 4
    gone = [h for h, _f in out.deletes]
    refs, blob = t.a.read_refs(abi.REFS_DELETE, 0, 4)
    assert Engine.ref_items(refs, blob) == [t.expect(h) for h in gone]
    # one create after the tick: it takes a slot the tick freed, so the delete list is refused from here on
    h, s, _c = t.batch([("ADDED", t.doc("late", names[0]))], "a create after the tick")
    assert not s.any() and int(h[0]) in gone
    for which in (abi.REFS_DELETE, abi.REFS_POD_PATCH):
        with pytest.raises(KwokError) as ei:
            t.a.read_refs(which, 0, 0)
        assert ei.value.code == abi.EINVAL and "stale" in str(ei.value)
    # the node lists still answer: no node was ingested
    n_hb = len(out.heartbeat_nodes)
    refs, blob = t.a.read_refs(abi.REFS_HEARTBEAT, 0, n_hb)
    assert n_hb and [it[2] for it in Engine.ref_items(refs, blob)] == [t.node_name[int(h)] for h in out.heartbeat_nodes]
    # the next tick's lists answer again; a bind moves the counter as an ingest does
    n_hb = len(t.tick("next tick").heartbeat_nodes)
    assert t.a.refs_bind([int(h[0])], [b"re"], [b"bound"]) == 0
    t.set_pod(int(h[0]), (b"re", b"bound", t.live[int(h[0])][2]))
    with pytest.raises(KwokError) as ei:
        t.a.read_refs(abi.REFS_POD_PATCH, 0, 0)
    assert ei.value.code == abi.EINVAL
    # ... and a node ingest moves the nodes' counter only after it happens
    t.a.read_refs(abi.REFS_HEARTBEAT, 0, n_hb)
    t.nodes(["one-more"])
    with pytest.raises(KwokError) as ei:
        t.a.read_refs(abi.REFS_HEARTBEAT, 0, n_hb)
    assert ei.value.code == abi.EINVAL and "stale" in str(ei.value)
    t.tick("after the node")
    # a tick submitted before the ingest and collected after it: the value is taken at submit
    t.batch([("MODIFIED", t.doc("g-%d" % k, names[k % 6], deleting=True)) for k in range(4, 6)], "more marks")
    marked = [t.by_uid[RefLock.uid_of("default", "g-%d" % k).encode()] for k in range(4, 6)]
    for x in t.both:
        x.tick_submit(t.now)
    t.drop(marked)  # (the ingest finishes the submitted tick first, which frees them)
    t.batch([("ADDED", t.doc("between", names[1]))], "a create between submit and collect")
    for x in t.both:
        assert sorted(h for h, _f in x.tick_collect().deletes) == sorted(marked)
    with pytest.raises(KwokError) as ei:
        t.a.read_refs(abi.REFS_DELETE, 0, 0)
    assert ei.value.code == abi.EINVAL and "stale" in str(ei.value)
    t.close()


@pytest.mark.parametrize("entry", ["uid", "echo"])
def test_fuzz(entry):
    """~1200 pod events over 160 pods in 5 batches with a tick between them: creates, upserts, deletion marks
    and Deleted lines (nothing follows a uid's Deleted line in a batch, as on a real watch), names of 1..60 bytes in 5 namespaces"""
    t = RefLock(once=entry == "uid", entry=entry, seed=11)
    names = fleet(t, 16)
    rng = t.rng
    ident = [("fz-%d" % (k % 5), "f%d-%s" % (k, "n" * int(rng.integers(0, 56)))) for k in range(160)]
    total = 0
    for r in range(5):
        lines, gone = [], set()
        for _ in range(int(rng.integers(200, 280))):
            k = int(rng.integers(0, 160))
            if k in gone:
                continue
            typ = ("ADDED", "MODIFIED", "MODIFIED", "DELETED")[int(rng.integers(0, 4))]
            if typ == "DELETED":
                gone.add(k)
            kw = dict(deleting=True, finalizers=int(rng.integers(0, 2))) if rng.integers(0, 6) == 0 else {}
            lines.append((typ, t.doc(ident[k][1], names[k % 16], ns=ident[k][0], **kw)))
        t.batch(lines, "fuzz batch %d" % r)
        total += len(lines)
        t.tick("fuzz tick %d" % r)
    s = t.a.refs_stats()
    assert total > 800 and s["notes"] > 160 and s["unnamed"] == 0
    t.close()
