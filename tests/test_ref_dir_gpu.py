"""GPU: the reference directory itself (include/kwok_watch.h; refs.hip:
k_refs_bind, k_refs_size, k_refs_gather, k_refs_note's no-name store), through
kwok_refs_bind and kwok_refs_lookup on the small geometry with a few dozen pods.  The
yardstick is a Python dict kept beside it: handle -> (namespace, name, uid); every
comparison is byte for byte, the layout of the blob included.

Not tested: the refusal of kwok_refs_enable on a multi-rank engine (no forced-multi
fixture is at hand in one process; the check is kwok_uid_dir_enable's, `e->multi`)."""
import ctypes as C

import numpy as np
import pytest

from kwok_amd import abi
from kwok_amd.engine import Engine, KwokError, make_config

pytestmark = pytest.mark.gpu

T0 = 1704067230
KW = dict(cidr="10.0.0.1/16", node_ip="196.168.0.1", buckets=64, node_slots_per_bucket=32, pod_slots_per_bucket=512)
SPEC = ([("fake-pod", "fake")], [], [])
UID36 = b"0f0e0d0c-0b0a-4908-8706-05040302%04d"


def check_layout(refs, blob, where=""):
    """offsets are multiples of 16, items lie in list order without gaps, every tail is zero, the blob ends
    with the last item"""
    raw = blob.tobytes()
    at = 0
    for r in refs:
        n = int(r["ns_len"]) + int(r["name_len"]) + int(r["uid_len"])
        assert int(r["off"]) == at and at % 16 == 0 and int(r["reserved0"]) == 0, where
        pad = -n % 16
        assert raw[at + n:at + n + pad] == b"\0" * pad, where
        at += n + pad
    assert at == len(raw), where


class Rig:
    def __init__(self, enable=True, **geom):
        self.kw = dict(KW, **geom)
        self.e = Engine(make_config(**self.kw))
        self.spec = self.e.register_pod_spec(*SPEC)
        self.stride = self.kw.get("pod_handle_stride") or self.kw["pod_slots_per_bucket"]
        self.n_slots = self.kw["buckets"] * self.stride
        self.want = {}  # handle -> [namespace, name, uid] (name b"": none stored): the host's map of the live pods
        self.last = {}  # handle -> what its slot last stored (live or not)
        if enable:
            self.e.refs_enable()

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
        for x in h:  # a create through an entry that carries neither a name nor a uid
            self.want[int(x)] = [b"", b"", b""]
            self.last[int(x)] = self.want[int(x)]
        return h

    def gone(self, handles):
        for h in handles:
            del self.want[int(h)]

    def delete(self, handles):
        rec = np.zeros(len(handles), abi.POD_REC_DTYPE)
        rec["op"], rec["target"] = abi.OP_DELETE, handles
        assert not self.e.ingest_pods_packed(rec)[1].any()
        self.gone(handles)

    def bind(self, handles, nss, names, bad=0):
        assert self.e.refs_bind(handles, nss, names) == bad
        if not bad:
            for h, ns, nm in zip(handles, nss, names):
                self.want[int(h)][0:2] = [bytes(ns), bytes(nm)]

    def bind_uid(self, handles, uids):
        assert self.e.uid_bind(handles, uids) == 0
        for h, u in zip(handles, uids):
            self.want[int(h)][2] = bytes(u)

    def expect(self, h, any_slot=False):
        w = self.want.get(int(h))
        if w is None and any_slot and int(h) in self.last:
            w = self.last[int(h)]
        if w is None:
            return (abi.ENOTFOUND, b"", b"", b"")
        return (abi.OK, w[0], w[1], w[2]) if w[1] else (abi.REF_NONE, b"", b"", w[2])

    def check(self, where, handles=None, flags=0):
        hs = list(self.want) if handles is None else [int(h) for h in handles]
        refs, blob = self.e.refs_lookup(abi.KIND_PODS, hs, flags)
        check_layout(refs, blob, where)
        got = Engine.ref_items(refs, blob)
        want = [self.expect(h, flags & abi.REFS_ANY_SLOT) for h in hs]
        assert got == want, where
        return refs, blob


CASES = [  # (namespace, name, uid)
    (b"n", b"a", UID36 % 0),                                 # 1 + 1
    (b"default", b"x" * 15, UID36 % 1),
    (b"default", b"x" * 16, UID36 % 2),
    (b"default", b"x" * 17, UID36 % 3),
    (b"d" * 63, b"p" * 253, b"u" * 40),                      # every length at its limit: 356 bytes, 23 units
    (b"", b"no-namespace", UID36 % 4),
    (b"default", b"q" * 21, UID36 % 5),                      # 7 + 21 + 36 = 64: ends on a unit
    (b"default", b"q" * 20, UID36 % 6),                      # 63: one short of it
    (b"default", b"q" * 22, UID36 % 7),                      # 65: one past it
    (b"kube-system", b"same-in-all-but-the-last-byte-A", UID36 % 8),
    (b"kube-system", b"same-in-all-but-the-last-byte-B", UID36 % 9),
    (b"s" * 63, b"y", b"v"),                                 # a 1-byte uid
    (b"ns", b"z" * 16, b""),                                 # no uid bound: a record that ends on a unit, nothing after it
    (b"n" * 9, b"m" * 7, b"w" * 16),                         # the uid starts on a unit boundary
    (b"n" * 9, b"m" * 8, b"w" * 39),                         # ... and one byte past it
    (b"n" * 8, b"m" * 7, b"w" * 33),                         # ... and one byte before it
]


def rig_with_cases():
    r = Rig()
    nh = r.nodes(["node-%d" % i for i in range(6)])
    pods = r.create(np.repeat(nh, 4))
    assert len(pods) == 24 and len(CASES) <= 24
    r.check("created without names")  # every one KWOK_REF_NONE
    hs = pods[:len(CASES)]
    r.bind(hs, [c[0] for c in CASES], [c[1] for c in CASES])
    with_uid = [(h, c[2]) for h, c in zip(hs, CASES) if c[2]]
    r.bind_uid([h for h, _u in with_uid], [u for _h, u in with_uid])
    return r, nh, pods


def test_bind_and_lookup_every_length():
    r, nh, pods = rig_with_cases()
    refs, blob = r.check("bound")
    assert (refs["status"][:len(CASES)] == abi.OK).all() and (refs["status"][len(CASES):] == abi.REF_NONE).all()
    assert int(refs[4]["ns_len"]) == 63 and int(refs[4]["name_len"]) == 253 and int(refs[4]["uid_len"]) == 40
    s = r.e.refs_stats()
    assert s["binds"] == len(CASES) and s["unnamed"] == 24 and s["notes"] == 0 and s["not_found"] == 0
    assert s["bytes"] >= r.n_slots * (abi.REF_STRIDE + 2)
    # each alone, and in reverse: the caller's order
    for h in pods:
        r.check("alone", [h])
    r.check("reversed", list(pods[::-1]))
    # refused, storing nothing: a 254-byte name, a 64-byte namespace, an empty name
    assert r.e.refs_bind(pods[:3], [b"a", b"b" * 64, b"c"], [b"n" * 254, b"ok", b""]) == 3
    r.check("after refused binds")
    # bad handles: negative, past the slots, on an unused slot
    free = int(np.setdiff1d(np.arange(r.stride * 3, r.stride * 3 + 64), pods)[0])
    bad = [-1, r.n_slots + 5, 2 ** 31 - 1, free]
    assert r.e.refs_bind(bad, [b"x"] * 4, [b"h1", b"h2", b"h3", b"h4"]) == 4
    r.check("bad handles", bad + [int(pods[0])])
    assert r.e.refs_stats()["not_found"] == 4
    # rebinding replaces: shorter, longer, and a name that differs in its last byte only
    r.bind(pods[:3], [b"", b"other-namespace", CASES[2][0]], [b"r", b"r" * 200, CASES[2][1][:-1] + b"y"])
    r.check("rebound")
    # an unknown kind and unknown flags are refused
    for call in (lambda: r.e.refs_lookup(2, [0]), lambda: r.e.refs_lookup(abi.KIND_PODS, [0], 2)):
        with pytest.raises(KwokError) as ei:
            call()
        assert ei.value.code == abi.EINVAL
    r.e.close()


def test_freed_slots_keep_their_bytes_and_reused_slots_lose_them():
    r, nh, pods = rig_with_cases()
    r.e.tick(T0)
    # by a DELETE record
    r.delete(pods[:5])
    r.check("deleted by record", pods)
    r.check("deleted by record, any slot", pods, abi.REFS_ANY_SLOT)
    # by the engine's tick: a deletion-marked pod on a managed node
    ev = np.zeros(3, abi.POD_EVENT_DTYPE)
    ev["op"], ev["handle"], ev["node_handle"], ev["spec_id"] = abi.OP_UPSERT, pods[5:8], -1, r.spec
    ev["creation_unix"], ev["phase"] = T0 - 90, abi.PHASE_RUNNING
    ev["flags"] = abi.POD_STATUS_NONEMPTY | abi.POD_DELETING
    assert not r.e.ingest_pods_raw(ev, b"")[1].any()
    out = r.e.tick(T0 + 30)
    assert sorted(h for h, _f in out.deletes) == sorted(int(h) for h in pods[5:8])
    r.gone(pods[5:8])
    r.check("deleted by the tick", pods)
    r.check("deleted by the tick, any slot", pods, abi.REFS_ANY_SLOT)
    # the tick's own delete list answers in list order
    refs, blob = r.e.read_refs(abi.REFS_DELETE, 0, 3)
    check_layout(refs, blob)
    assert Engine.ref_items(refs, blob) == [r.expect(h, True) for h, _f in out.deletes]
    # by a sweep
    r.e.resync_begin(abi.KIND_PODS)
    assert r.e.resync_mark(abi.KIND_PODS, pods[12:]) == 0
    swept, _rel, _nd = r.e.resync_sweep(abi.KIND_PODS)
    assert sorted(swept) == sorted(int(h) for h in pods[8:12])
    r.gone(pods[8:12])
    r.check("swept", pods)
    refs, _b = r.check("swept, any slot", swept, abi.REFS_ANY_SLOT)
    assert (refs["status"] == abi.OK).all()
    assert r.e.refs_stats()["not_found"] == 5 + 8 + 12
    # the freed slots taken by creates that carry no name: KWOK_REF_NONE, not the previous pod's name
    again = r.create(np.repeat(nh[:3], 4))
    assert set(int(h) for h in again) == set(int(h) for h in pods[:12])  # the lowest free slots of their buckets
    refs, _b = r.check("slots reused without a name", pods)
    assert (refs["status"][:12] == abi.REF_NONE).all() and (refs["name_len"][:12] == 0).all()
    assert (refs["uid_len"][:12] == 0).all()  # (the uid directory dropped the previous pod's uid as well)
    r.check("slots reused without a name, any slot", pods, abi.REFS_ANY_SLOT)
    # ... until bound again, under other names
    r.bind(again, [b"second"] * 12, [b"second-%d" % i for i in range(12)])
    r.check("slots reused and bound", pods)
    r.e.close()


def test_growth_between_binds_and_lookups():
    r = Rig(buckets=64, node_slots_per_bucket=8, pod_slots_per_bucket=16, pod_handle_stride=8192)
    nh = r.nodes(["node-%07d" % i for i in range(40)])
    old = r.create(np.concatenate([np.full(14, nh[0], np.int32), nh[1:]]))
    r.bind(old, [b"ns-%d" % (i % 5) for i in range(len(old))], [b"pod-" + b"g" * (i * 4) + b"%d" % i for i in range(len(old))])
    r.bind_uid(old, [UID36 % i for i in range(len(old))])
    r.check("before the growth")
    new = r.create(np.full(300, nh[0], np.int32))  # grows every bucket: the per-slot records are re-laid out
    assert int(new.max()) % r.stride >= 16
    r.check("grown")
    r.bind(new, [b"grown"] * 300, [b"grown-%d" % i for i in range(300)])
    r.delete(old[:7])
    r.check("grown and bound", list(old) + list(new))
    r.check("grown and bound, any slot", list(old) + list(new), abi.REFS_ANY_SLOT)
    r.e.close()


def test_a_blob_one_byte_short_writes_nothing():
    r, nh, pods = rig_with_cases()
    hs = np.ascontiguousarray(pods, np.int32)
    _refs, blob = r.e.refs_lookup(abi.KIND_PODS, hs)
    need = len(blob)
    assert need % 16 == 0 and need > 356
    refs = np.full(len(hs), 0xAB, np.uint8).repeat(16)
    buf = np.full(need, 0xAB, np.uint8)
    used = C.c_size_t(1)
    rc = r.e._lib.kwok_refs_lookup(r.e._h, abi.KIND_PODS, hs.ctypes.data, len(hs), 0, refs.ctypes.data, buf.ctypes.data,
                                   need - 1, C.byref(used))
    assert rc == abi.EINVAL and used.value == need
    assert (refs == 0xAB).all() and (buf == 0xAB).all()
    with pytest.raises(KwokError) as ei:
        r.e.refs_lookup(abi.KIND_PODS, hs, blob_cap=need - 1)
    assert ei.value.code == abi.EINVAL and "blob_cap" in str(ei.value)
    # exactly the need: answered
    refs2, blob2 = r.e.refs_lookup(abi.KIND_PODS, hs, blob_cap=need)
    assert len(blob2) == need and Engine.ref_items(refs2, blob2) == [r.expect(h) for h in hs]
    # no handles: nothing to write, KWOK_OK
    refs0, blob0 = r.e.refs_lookup(abi.KIND_PODS, [])
    assert len(refs0) == 0 and len(blob0) == 0
    r.e.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_lookups_of_many_handles_with_repeats(n):
    r, nh, pods = rig_with_cases()
    rng = np.random.default_rng(n)
    pool = np.concatenate([pods, [-1, r.n_slots + 1]]).astype(np.int32)
    hs = pool[rng.integers(0, len(pool), n)]
    r.check("%d handles" % n, hs)
    r.e.close()


def test_node_lookups_answer_the_ingested_names():
    r = Rig()
    names = [b"n", b"node-%d" % 7, b"x" * 15, b"x" * 16, b"x" * 17, b"w" * 253, b"worker-a", b"worker-b"]
    nh = r.nodes([n.decode() for n in names])
    hs = [int(h) for h in nh] + [-1, 64 * 32 + 3, int(nh[0])]
    refs, blob = r.e.refs_lookup(abi.KIND_NODES, hs)
    check_layout(refs, blob)
    want = [(abi.OK, b"", n, b"") for n in names] + [(abi.ENOTFOUND, b"", b"", b"")] * 2 + [(abi.OK, b"", names[0], b"")]
    assert Engine.ref_items(refs, blob) == want
    # a slot of the directory that holds no node
    used = set(int(h) for h in nh)
    free = next(h for h in range(64 * 32) if h not in used)
    refs, blob = r.e.refs_lookup(abi.KIND_NODES, [free], abi.REFS_ANY_SLOT)
    assert Engine.ref_items(refs, blob) == [(abi.ENOTFOUND, b"", b"", b"")]
    # the tick's heartbeat and node-init lists, in list order
    out = r.e.tick(T0)
    name_of = dict(zip((int(h) for h in nh), names))
    for which, handles in ((abi.REFS_HEARTBEAT, list(out.heartbeat_nodes)), (abi.REFS_NODE_INIT, [h for h, _b in out.node_inits])):
        assert len(handles) == len(names)
        refs, blob = r.e.read_refs(which, 0, len(handles))
        check_layout(refs, blob)
        assert Engine.ref_items(refs, blob) == [(abi.OK, b"", name_of[int(h)], b"") for h in handles]
    with pytest.raises(KwokError) as ei:
        r.e.read_refs(abi.REFS_HEARTBEAT, len(names), 1)
    assert ei.value.code == abi.EINVAL
    r.e.close()


def test_calls_without_the_directory():
    r = Rig(enable=False)
    for call in (lambda: r.e.refs_bind([0], [b"ns"], [b"n"]), lambda: r.e.refs_lookup(abi.KIND_PODS, [0]),
                 lambda: r.e.read_refs(abi.REFS_DELETE, 0, 0)):
        with pytest.raises(KwokError) as ei:
            call()
        assert ei.value.code == abi.EINVAL
    assert r.e.refs_stats() == dict.fromkeys(abi.REFS_STATS, 0)
    assert r.e.uid_stats() == dict.fromkeys(abi.UID_STATS, 0)
    r.e.refs_enable()
    r.e.refs_enable()  # idempotent, and it enabled the uid directory
    assert list(r.e.uid_lookup([b"u"])) == [-1]
    refs, blob = r.e.refs_lookup(abi.KIND_PODS, [0])
    assert Engine.ref_items(refs, blob) == [(abi.ENOTFOUND, b"", b"", b"")]
    r.e.close()
