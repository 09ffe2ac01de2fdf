"""GPU: the pod uid directory itself (include/kwok_watch.h; uid.hip:
k_uid_bind, k_uid_lookup, k_uid_note, k_uid_rebuild), through kwok_uid_bind and
kwok_uid_lookup.  The table is forced to 64 entries (KWOK_UID_TAB_LOG2=6) under 24
pods and more, so that probes chain, wrap the table's end and meet stale entries; the
yardstick is a Python dict kept beside it.

Not tested: the refusal of kwok_uid_dir_enable on a multi-rank engine (no forced-multi
fixture is at hand in one process; the check is the sweep's, `e->multi`)."""
import numpy as np
import pytest

from kwok_amd import abi
from kwok_amd.engine import Engine, KwokError, make_config

pytestmark = pytest.mark.gpu

T0 = 1704067230
KW = dict(cidr="10.0.0.1/16", node_ip="196.168.0.1", buckets=64, node_slots_per_bucket=32, pod_slots_per_bucket=512)
SPEC = ([("fake-pod", "fake")], [], [])


class Rig:
    def __init__(self, monkeypatch, log2=6, enable=True, **geom):
        if log2:
            monkeypatch.setenv("KWOK_UID_TAB_LOG2", str(log2))
        else:
            monkeypatch.delenv("KWOK_UID_TAB_LOG2", raising=False)
        self.kw = dict(KW, **geom)
        self.e = Engine(make_config(**self.kw))
        self.spec = self.e.register_pod_spec(*SPEC)
        self.stride = self.kw.get("pod_handle_stride") or self.kw["pod_slots_per_bucket"]
        self.n_slots = self.kw["buckets"] * self.stride
        self.want = {}  # uid (bytes) -> handle: the host's map
        if enable:
            self.e.uid_dir_enable()

    def nodes(self, names):
        ar = abi.Arena()
        ev = np.zeros(len(names), abi.NODE_EVENT_DTYPE)
        ev["op"], ev["managed"], ev["lockable"] = abi.OP_UPSERT, 1, 1
        for i, n in enumerate(names):
            ev[i]["name"] = ar.ref(n)
        h, s = self.e.ingest_nodes_raw(ev, bytes(ar.buf))
        assert not s.any()
        return h

    def create(self, node_handles, flags=abi.POD_STATUS_NONEMPTY):
        n = len(node_handles)
        ev = np.zeros(n, abi.POD_EVENT_DTYPE)
        ev["op"], ev["handle"], ev["node_handle"], ev["spec_id"] = abi.OP_UPSERT, -1, node_handles, self.spec
        ev["creation_unix"], ev["phase"], ev["flags"] = T0 - 90, abi.PHASE_PENDING, flags
        h, s, _ = self.e.ingest_pods_raw(ev, b"")
        assert not s.any()
        return h

    def delete(self, handles):
        rec = np.zeros(len(handles), abi.POD_REC_DTYPE)
        rec["op"], rec["target"] = abi.OP_DELETE, handles
        h, s, _ = self.e.ingest_pods_packed(rec)
        assert not s.any()
        for u in [u for u, x in self.want.items() if x in set(int(v) for v in handles)]:
            del self.want[u]

    def bind(self, handles, uids, bad=0):
        assert self.e.uid_bind(handles, uids) == bad
        for h, u in zip(handles, uids):
            for old in [k for k, x in self.want.items() if x == int(h)]:
                del self.want[old]  # rebinding a handle replaces its uid
            self.want[bytes(u)] = int(h)

    def check(self, where, extra=()):
        uids = list(self.want) + list(extra)
        got = self.e.uid_lookup(uids)
        assert list(got) == [self.want.get(u, -1) for u in uids], where

    def used(self):
        return np.nonzero(self.e.dump_pods(0, self.n_slots)[0])[0].astype(np.int32)


def uids_of(n, seed=0):
    """uids of length 1, 36 and 40, two equal in their first 39 bytes, the rest UUID-shaped"""
    rng = np.random.default_rng(seed)
    out = [b"a", b"b", b"x" * 39 + b"1", b"x" * 39 + b"2", b"y" * 40, b"y" * 39]
    while len(out) < n:
        h = rng.bytes(16).hex()
        out.append(("%s-%s-%s-%s-%s" % (h[:8], h[8:12], h[12:16], h[16:20], h[20:])).encode())
    assert len(set(out)) == len(out) and any(len(u) == 36 for u in out)
    return out[:n]


def test_bind_lookup_in_a_chained_table(monkeypatch):
    r = Rig(monkeypatch)
    nh = r.nodes(["node-%d" % i for i in range(6)])
    pods = r.create(np.repeat(nh, 4))
    assert len(pods) == 24
    assert list(r.e.uid_lookup([b"a", b"nobody"])) == [-1, -1]  # pods that exist have no uid until bound
    uids = uids_of(24)
    r.bind(pods, uids)
    s = r.e.uid_stats()
    assert s["binds"] == 24 and s["table_entries"] == 24 and s["rebuilds"] == 0
    # 24 of 64 entries from 24 hashes: some probe chains past its home entry (the dict says what is right)
    r.check("bound", extra=[b"", b"c", b"x" * 39, b"x" * 40, b"y" * 38, b"z" * 41, uids[7][:-1], uids[7] + b"0"])
    s = r.e.uid_stats()
    assert s["hits"] == 24 and s["lookups"] == 24 + 2 + 6  # (the empty and the 41-byte key are never probed)
    # lengths 0 and 41, and handles that name no live pod, bind nothing
    free = int(np.setdiff1d(np.arange(r.stride * 3, r.stride * 3 + 64), pods)[0])
    assert r.e.uid_bind([pods[0], pods[1]], [b"", b"q" * 41]) == 2
    assert r.e.uid_bind([-1, r.n_slots + 5, 2 ** 31 - 1, free], [b"h1", b"h2", b"h3", b"h4"]) == 4
    r.check("after rejected binds", extra=[b"h1", b"h2", b"h3", b"h4", b"q" * 40])
    # rebinding replaces the handle's uid
    r.bind(pods[:3], [b"new-0", b"new-1", uids[2]])
    r.check("rebound", extra=[uids[0], uids[1]])
    assert list(r.e.uid_lookup([uids[0], b"new-0"])) == [-1, int(pods[0])]
    r.e.close()


def test_a_freed_slot_unbinds(monkeypatch):
    r = Rig(monkeypatch)
    nh = r.nodes(["node-%d" % i for i in range(6)])
    pods = r.create(np.repeat(nh, 4))
    uids = uids_of(24, seed=1)
    r.bind(pods, uids)
    r.e.tick(T0)
    # by a DELETE record
    r.delete(pods[:5])
    r.check("deleted by record", extra=uids[:5])
    # by the engine's tick: a deletion-marked pod on a managed node
    ev = np.zeros(3, abi.POD_EVENT_DTYPE)
    ev["op"], ev["handle"], ev["node_handle"], ev["spec_id"] = abi.OP_UPSERT, pods[5:8], -1, r.spec
    ev["creation_unix"], ev["phase"] = T0 - 90, abi.PHASE_RUNNING
    ev["flags"] = abi.POD_STATUS_NONEMPTY | abi.POD_DELETING
    assert not r.e.ingest_pods_raw(ev, b"")[1].any()
    out = r.e.tick(T0 + 30)
    assert sorted(h for h, _f in out.deletes) == sorted(int(h) for h in pods[5:8])
    for u in uids[5:8]:
        del r.want[u]
    r.check("deleted by the tick", extra=uids[:8])
    # by a sweep
    r.e.resync_begin(abi.KIND_PODS)
    assert r.e.resync_mark(abi.KIND_PODS, pods[12:]) == 0
    swept, _rel, _nd = r.e.resync_sweep(abi.KIND_PODS)
    assert sorted(swept) == sorted(int(h) for h in pods[8:12])
    for u in uids[8:12]:
        del r.want[u]
    r.check("swept", extra=uids[:12])
    # the freed slots taken by creates that carry no uid do not answer to the old uids
    unbound0 = r.e.uid_stats()["unbound"]
    again = r.create(np.repeat(nh[:3], 4))
    assert set(int(h) for h in again) == set(int(h) for h in pods[:12])  # the lowest free slots of their buckets
    assert r.e.uid_stats()["unbound"] - unbound0 == 12
    r.check("slots reused without a uid", extra=uids[:12])
    # ... until bound again, under other uids
    r.bind(again, [b"second-%d" % i for i in range(12)])
    r.check("slots reused and bound", extra=uids[:12])
    r.e.close()


def test_rebuilds_keep_every_lookup_right(monkeypatch):
    r = Rig(monkeypatch)
    nh = r.nodes(["node-%d" % i for i in range(6)])
    keep = r.create(np.repeat(nh, 3))  # 18 pods that stay
    r.bind(keep, uids_of(18, seed=2))
    gone = []
    for c in range(8):  # 8 x 6 creates and deletes: 48 stale entries could not stay in 64
        pods = r.create(nh)
        uids = [b"cycle-%d-%d" % (c, i) for i in range(6)]
        r.bind(pods, uids)
        r.check("cycle %d bound" % c, extra=gone)
        r.delete(pods)
        gone += uids
        r.check("cycle %d deleted" % c, extra=gone)
    s = r.e.uid_stats()
    assert s["rebuilds"] >= 1 and s["table_entries"] < 64
    assert sorted(r.used()) == sorted(int(h) for h in keep)
    # the forced table cannot take more live uids than it has entries: refused, nothing breaks
    more = r.create(np.repeat(nh, 8))
    with pytest.raises(KwokError) as ei:
        r.e.uid_bind(more, [b"m-%d" % i for i in range(48)])
    assert ei.value.code == abi.EFULL
    r.check("after the refusal", extra=[b"m-0", b"m-47"])
    r.e.close()


def test_growth_between_binds_and_lookups(monkeypatch):
    r = Rig(monkeypatch, log2=0, buckets=64, node_slots_per_bucket=8, pod_slots_per_bucket=16, pod_handle_stride=8192)
    nh = r.nodes(["node-%07d" % i for i in range(40)])
    old = r.create(np.concatenate([np.full(14, nh[0], np.int32), nh[1:]]))
    uids = uids_of(len(old), seed=3)
    r.bind(old, uids)
    e0 = r.e.uid_stats()
    new = r.create(np.full(300, nh[0], np.int32))  # grows every bucket: the per-slot uids are re-laid out
    assert int(new.max()) % r.stride >= 16
    r.check("grown", extra=[b"nobody"])
    assert r.e.uid_stats()["rebuilds"] > e0["rebuilds"]  # (the table follows the pod slots)
    r.bind(new, [b"grown-%d" % i for i in range(300)])
    r.delete(old[:7])
    r.check("grown and bound", extra=uids[:7])
    r.e.close()


def test_calls_without_the_directory(monkeypatch):
    r = Rig(monkeypatch, enable=False)
    for call in (lambda: r.e.uid_bind([0], [b"u"]), lambda: r.e.uid_lookup([b"u"])):
        with pytest.raises(KwokError) as ei:
            call()
        assert ei.value.code == abi.EINVAL
    assert r.e.uid_stats() == dict.fromkeys(abi.UID_STATS, 0)
    r.e.uid_dir_enable()
    r.e.uid_dir_enable()  # idempotent
    assert list(r.e.uid_lookup([b"u"])) == [-1]
    r.e.close()
