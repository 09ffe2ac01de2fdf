"""GPU: every scratch group of the framed ingests and the directories at first use, grown
once, grown again and used small afterwards (engine_impl.h DevGroup, engine.cpp).

One engine `a` with the uid directory, the echo ledger and the reference directory takes
every path with batches of 8, 4097, 5122 and 8 records: first use at the 4096 floor, the
first growth (capacity 5121), a growth past it, and a small call on grown buffers.  Every
call's per-record outputs equal the comparison the path's own test uses: the host framers
(kwok_frame_watch / kwok_frame_list), the host-map runs of controller.ingest_pod_runs and
the typed echo front end on a second engine `b` fed the same sequence, Python maps for the
directories' bind / lookup pairs.  At the end both engines hold the same pods."""
import numpy as np
import pytest

import watch_frames as wf
from kwok_amd import abi
from kwok_amd.codec import Codec, frame_list, frame_watch
from kwok_amd.controller import NOT_SENT, Echoes, ingest_pod_runs
from kwok_amd.engine import Engine, make_config

pytestmark = pytest.mark.gpu

SIZES = (8, 4097, 5122, 8)
N = max(SIZES)
T0 = 1704067230
# one pod per node: 5122 of each spread over 64 buckets (about 80 per bucket)
KW = dict(cidr="10.0.0.1/16", node_ip="196.168.0.1", buckets=64, node_slots_per_bucket=256, pod_slots_per_bucket=512,
          heartbeat_once=True)
N_SLOTS = KW["buckets"] * KW["pod_slots_per_bucket"]
SPEC = ([("fake-pod", "fake")], [], [])
POD = ('{"apiVersion":"v1","kind":"Pod","metadata":{"name":"p%d","namespace":"ns%d","creationTimestamp":'
       '"2024-01-01T00:00:00Z","uid":"u-%d","resourceVersion":"%s","labels":{"app":"fake"}},"spec":{"nodeName":"n%d",'
       '"containers":[{"name":"fake-pod","image":"fake"}]},"status":{"phase":"Pending"}}')
NODE = ('{"apiVersion":"v1","kind":"Node","metadata":{"name":"n%d","uid":"nu-%d","resourceVersion":"%s","annotations":'
        '{"kwok.x-k8s.io/node":"fake"}},"spec":{},"status":{"daemonEndpoints":{"kubeletEndpoint":{"Port":0}},"nodeInfo":{}}}')


def pod(i, rv="1"):
    return (POD % (i, i % 7, i, rv, i)).encode()


def node(i, rv="1"):
    return (NODE % (i, i, rv)).encode()


def stream_of(docs, typ):
    return b"".join(wf.wrap(d, typ) for d in docs)


def span(stream, f, key):
    return bytes(stream[int(f[key]["off"]):int(f[key]["off"]) + int(f[key]["len"])])


class Pair:
    def __init__(self):
        self.a, self.b = Engine(make_config(**KW)), Engine(make_config(**KW))
        assert self.a.register_pod_spec(*SPEC) == self.b.register_pod_spec(*SPEC)
        self.codec = Codec(manage_all_nodes=True)
        self.a.refs_enable()  # (the uid directory with it)
        self.a.echo_enable()
        self.b.echo_enable()
        self.echo = Echoes()
        self.by_uid = {}       # b's host map: uid -> handle
        self.node_handle = {}
        self.round = 0

    def close(self):
        self.a.close()
        self.b.close()
        self.codec.close()

    def frame(self, stream, n, where):
        """both engines frame the stream; a's frames equal the host framer's"""
        want, consumed = frame_watch(stream)
        fa, used, _nh, sa = self.a.frame_watch(stream)
        _fb, _ub, _nhb, sb = self.b.frame_watch(stream)
        assert used == consumed == len(stream) and len(fa) == n, where
        wf.assert_frames_equal(fa, want, where)
        return fa, sa, sb

    def note(self, pairs, where):
        """the engine's own patches: a note in a's ledger, in b's and in the host rule's"""
        if not pairs:
            return
        for x in (self.a, self.b):
            assert not x.echo_update([abi.ECHO_NOTE] * len(pairs), [u for u, _r in pairs], [r for _u, r in pairs]).any(), where
        for u, r in pairs:
            self.echo.note(u, r)

    def same_pods(self, where):
        da, db = self.a.dump_pods(0, N_SLOTS), self.b.dump_pods(0, N_SLOTS)
        for k, what in enumerate(("used", "phase", "hostIP", "podIP")):
            assert (da[k] == db[k]).all(), "%s: pod %s" % (where, what)
        return da

    # ---- kwok_frame_watch_gpu + kwok_ingest_nodes_framed_echo ----
    def nodes_echo(self, n, known):
        where = "nodes, %d" % n
        self.round += 1
        rv = lambda i: "n%d-%d" % (self.round, i)  # noqa: E731
        self.note([(b"nu-%d" % i, rv(i).encode()) for i in range(0, min(n, known), 5)], where)
        stream = stream_of([node(i, rv(i)) for i in range(n)], "MODIFIED")
        fa, sa, sb = self.frame(stream, n, where)
        ha, sta, _nh, ne = self.a.ingest_nodes_framed_echo(self.codec, sa, np.arange(n))
        uids, rvs = [span(stream, f, "uid") for f in fa], [span(stream, f, "resource_version") for f in fa]
        drop = self.b.echo_match(uids, rvs, np.zeros(n, np.uint8)).astype(bool)
        assert list(drop) == [self.echo.is_echo(u, r) for u, r in zip(uids, rvs)], where + " (typed front end / host rule)"
        hb, stb = np.full(n, -1, np.int32), np.full(n, abi.ECHO, np.int32)
        keep = np.nonzero(~drop)[0]
        hb[keep], stb[keep], _nhb = self.b.ingest_nodes_framed(self.codec, sb, keep.astype(np.uint32))
        for i in np.nonzero(drop)[0]:
            hb[i] = self.node_handle.get(int(i), -1)
        assert list(sta) == list(stb) and list(ha) == list(hb) and ne == int(drop.sum()), where
        assert not stb[keep].any(), where
        self.node_handle.update((int(i), int(hb[i])) for i in keep)

    def host_runs(self, sb, frames, uids, deleted):
        """b: the frames through controller.ingest_pod_runs over kwok_ingest_pods_framed and the host's uid map"""
        relb = np.zeros(len(frames), np.uint32)

        def send(idx, ops, hv):
            h1, s1, r1, _nhb = self.b.ingest_pods_framed(self.codec, sb, frames[idx].astype(np.uint32), hv.astype(np.int32))
            relb[idx] = r1
            return h1, s1

        hb, stb, runs = ingest_pod_runs(self.b, self.by_uid, np.empty(len(frames)), uids, [deleted] * len(frames), None, sender=send)
        return hb, stb, relb, runs

    # ---- kwok_ingest_pods_framed_uid against the host-map runs over kwok_ingest_pods_framed ----
    def pods_uid(self, ids, typ, where):
        n = len(ids)
        stream = stream_of([pod(i) for i in ids], typ)
        fa, sa, sb = self.frame(stream, n, where)
        ha, sta, rela, _nh, runs_a = self.a.ingest_pods_framed_uid(self.codec, sa, np.arange(n))
        uids = [span(stream, f, "uid") for f in fa]
        hb, stb, relb, runs_b = self.host_runs(sb, np.arange(n), uids, typ == "DELETED")
        assert list(sta) == list(stb) and list(ha) == list(hb) and list(rela) == list(relb) and runs_a == runs_b, where
        return ha, sta

    # ---- kwok_ingest_pods_framed (by handle) against kwok_ingest_pods_json ----
    def pods_framed(self, n):
        where = "framed, %d" % n
        docs = [pod(i, "m%d" % n) for i in range(n)]
        stream = stream_of(docs, "MODIFIED")
        _fa, sa, _sb = self.frame(stream, n, where)
        hv = np.array([self.by_uid[b"u-%d" % i] for i in range(n)], np.int32)
        ha, sta, rela, _nh = self.a.ingest_pods_framed(self.codec, sa, np.arange(n), hv)
        arena, offs, lens = Engine._docs(docs)
        hb, stb, relb, _nhb = self.b.ingest_pods_json(self.codec, arena, offs, lens, np.full(n, abi.OP_UPSERT, np.uint8), hv)
        assert not sta.any() and list(ha) == list(hv), where
        assert list(sta) == list(stb) and list(ha) == list(hb) and list(rela) == list(relb), where

    # ---- kwok_echo_update / kwok_echo_match against the host rule ----
    def echo_typed(self, n):
        where = "echo update / match, %d" % n
        self.round += 1
        uids = [b"u-%d" % i for i in range(n)]
        rvs = [b"t%d-%d" % (self.round, i) for i in range(n)]
        self.note(list(zip(uids, rvs)), where)
        # every other event names the noted version; every seventh is a Deleted event (never an echo: it forgets)
        ask = [r if i % 2 == 0 else r + b"x" for i, r in enumerate(rvs)]
        dl = np.array([i % 7 == 3 for i in range(n)], np.uint8)
        want = []
        for u, r, d in zip(uids, ask, dl):
            want.append((not d) and self.echo.is_echo(u, r))
            if d:
                self.echo.forget(u)
        for x in (self.a, self.b):
            assert list(x.echo_match(uids, ask, dl).astype(bool)) == want, where
        assert self.a.echo_stats()["live_uids"] == len(self.echo.rv), where

    # ---- kwok_ingest_pods_framed_echo against the typed front end + the host-map runs over what it keeps ----
    def pods_echo(self, n):
        where = "framed echo, %d" % n
        self.round += 1
        rv = lambda i: "e%d-%d" % (self.round, i)  # noqa: E731
        self.note([(b"u-%d" % i, rv(i).encode()) for i in range(0, n, 3)], where)
        stream = stream_of([pod(i, rv(i)) for i in range(n)], "MODIFIED")
        fa, sa, sb = self.frame(stream, n, where)
        ha, sta, rela, _nh, runs_a, ne = self.a.ingest_pods_framed_echo(self.codec, sa, np.arange(n))
        uids, rvs = [span(stream, f, "uid") for f in fa], [span(stream, f, "resource_version") for f in fa]
        drop = self.b.echo_match(uids, rvs, np.zeros(n, np.uint8)).astype(bool)
        assert list(drop) == [self.echo.is_echo(u, r) for u, r in zip(uids, rvs)] and drop.sum() == len(range(0, n, 3)), where
        keep = np.nonzero(~drop)[0]
        hb, stb, relb = np.full(n, -1, np.int32), np.full(n, abi.ECHO, np.int32), np.zeros(n, np.uint32)
        hb[keep], stb[keep], relb[keep], runs_b = self.host_runs(sb, keep, [uids[i] for i in keep], False)
        hb[drop] = [self.by_uid[u] for u, d in zip(uids, drop) if d]  # (the echoes' live handles)
        assert list(sta) == list(stb) and list(ha) == list(hb) and list(rela) == list(relb), where
        assert runs_a == runs_b and ne == int(drop.sum()) and not stb[keep].any(), where

    # ---- kwok_uid_bind / _lookup and kwok_refs_bind / _lookup against the maps ----
    def dirs(self, n):
        where = "bind / lookup, %d" % n
        uids = [b"u-%d" % i for i in range(n)]
        hv = np.array([self.by_uid[u] for u in uids], np.int32)
        assert list(self.a.uid_lookup(uids)) == list(hv), where + " (the ingests' uids)"
        items = Engine.ref_items(*self.a.refs_lookup(abi.KIND_PODS, hv))
        assert items == [(abi.OK, b"ns%d" % (i % 7), b"p%d" % i, uids[i]) for i in range(n)], where + " (the ingests' names)"
        # rebound under other names and uids, looked up, and put back
        alt = [b"alt-%d" % i for i in range(n)]
        assert self.a.uid_bind(hv, alt) == 0 and self.a.refs_bind(hv, [b"other"] * n, alt) == 0, where
        assert list(self.a.uid_lookup(alt)) == list(hv), where
        assert Engine.ref_items(*self.a.refs_lookup(abi.KIND_PODS, hv)) == [(abi.OK, b"other", u, u) for u in alt], where
        assert self.a.uid_bind(hv, uids) == 0, where
        assert self.a.refs_bind(hv, [b"ns%d" % (i % 7) for i in range(n)], [b"p%d" % i for i in range(n)]) == 0, where
        assert list(self.a.uid_lookup(uids + alt)) == list(hv) + [-1] * n, where

    # ---- kwok_frame_list_gpu against the host framer, its items through the by-uid entry ----
    def listed(self, n):
        where = "list, %d" % n
        body = (b'{"kind":"PodList","apiVersion":"v1","metadata":{"resourceVersion":"7"},"items":[' +
                b",".join(pod(i, "l%d" % n) for i in range(n)) + b"]}")
        want, _info = frame_list(body)
        fa, _ia, _nh, sa = self.a.frame_list(body)
        assert len(fa) == n, where
        wf.assert_frames_equal(fa, want, where)
        ha, sta, _rel, _nh, runs = self.a.ingest_pods_framed_uid(self.codec, sa, np.arange(n))
        arena, offs, lens = Engine._docs([pod(i, "l%d" % n) for i in range(n)])
        hv = np.array([self.by_uid[b"u-%d" % i] for i in range(n)], np.int32)
        hb, stb, _relb, _nhb = self.b.ingest_pods_json(self.codec, arena, offs, lens, np.full(n, abi.OP_UPSERT, np.uint8), hv)
        assert list(ha) == list(hb) == list(hv) and list(sta) == list(stb) and not sta.any() and runs == 1, where

    # ---- kwok_resync_mark / _sweep: n marks in a session of their own; then the first n pods swept and created again ----
    def sweep(self, n):
        where = "sweep, %d" % n
        live = np.array([self.by_uid[b"u-%d" % i] for i in range(N)], np.int32)
        self.a.resync_begin(abi.KIND_PODS)
        assert self.a.resync_mark(abi.KIND_PODS, live[:n]) == 0, where
        assert self.a.resync_mark(abi.KIND_PODS, np.concatenate([live[:n], np.array([-1], np.int32)])) == 1, where
        self.a.resync_end(abi.KIND_PODS)
        self.a.resync_begin(abi.KIND_PODS)  # (the marks are cleared)
        if n < N:
            assert self.a.resync_mark(abi.KIND_PODS, live[n:]) == 0, where
        absent = np.sort(live[:n])
        pip = self.same_pods(where)[3]
        swept, rel, _nd = self.a.resync_sweep(abi.KIND_PODS)
        assert list(swept) == list(absent), where
        recs = np.zeros(n, abi.POD_REC_DTYPE)
        recs["op"], recs["target"], recs["pod_ip"] = abi.OP_DELETE, absent, pip[absent]
        hb, sb, rb = self.b.ingest_pods_packed(recs)
        assert not sb.any() and list(hb) == list(absent) and list(rel) == list(rb), where
        uids = [b"u-%d" % i for i in range(n)]
        for u in uids:  # the swept pods leave b's map, their notes the ledgers (Controller._end_resync)
            del self.by_uid[u]
            self.echo.forget(u)
        for x in (self.a, self.b):
            x.echo_update([abi.ECHO_FORGET] * n, uids, [b""] * n)
        self.same_pods(where + " swept")
        _h, st = self.pods_uid(range(n), "ADDED", where + " created again")
        assert not st.any(), where


def test_every_scratch_group_at_its_floor_grown_and_grown_again():
    t = Pair()
    known = 0
    for n in SIZES:
        t.nodes_echo(n, known)
        known = max(known, n)
    assert len(t.node_handle) == N and len(set(t.node_handle.values())) == N
    for n in SIZES:  # creates, then the same pods again
        h, st = t.pods_uid(range(n), "ADDED", "by uid, %d" % n)
        assert not st.any() and len(set(h)) == n
    h, st = t.pods_uid([N, N + 1], "DELETED", "unknown pods")
    assert list(st) == [NOT_SENT] * 2
    assert len(t.by_uid) == N
    for step in (t.pods_framed, t.echo_typed, t.pods_echo, t.dirs, t.listed, t.sweep):
        for n in SIZES:
            step(n)
    assert len(t.by_uid) == N
    for x in (t.a, t.b):
        x.tick(T0, read=False)
    t.same_pods("after the tick")
    t.close()
