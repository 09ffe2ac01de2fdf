"""GPU: the node uid directory itself (include/kwok_watch.h; nodes.hip:
k_nd_lookup, k_nd_uid_bind, k_nd_uid_note; refs.hip: k_refs_size_nd, k_refs_gather_nd)
through kwok_node_lookup, kwok_node_bind and the node answers of kwok_refs_lookup /
kwok_read_refs, on the small geometry (64 buckets x 32 node slots).  The yardstick is a
set of Python dicts kept beside the engine: name -> handle of the existing nodes, handle
-> the directory entry (an existing node, a zombie, a placeholder), handle -> (uid, stale)
by the rule of controller.py's _node_put / _node_pop.  Every comparison is byte for byte,
the layout of the blob included.

(tests/test_node_dir_gpu.py is the older parity test of the device node directory; this
file is the one the issue calls test_node_dir_gpu.py.)

Not tested: the refusal of kwok_node_dir_enable on a multi-rank engine (no forced-multi
fixture is at hand in one process; the check is kwok_uid_dir_enable's, `e->multi`)."""
import json

import numpy as np
import pytest

import watch_frames as wf
from harness import node_doc
from kwok_amd import abi
from kwok_amd.codec import Codec
from kwok_amd.engine import Engine, KwokError, load_engine_lib, make_config
from test_ref_dir_gpu import check_layout

pytestmark = pytest.mark.gpu

T0 = 1704067230
B, CN = 64, 32
KW = dict(cidr="10.0.0.1/16", node_ip="196.168.0.1", buckets=B, node_slots_per_bucket=CN, pod_slots_per_bucket=512)
UID36 = b"0f0e0d0c-0b0a-4908-8706-05040302%04d"
NOT_FOUND = (abi.ENOTFOUND, b"", b"", b"")


def bucket(name):
    return load_engine_lib().kwok_bucket_of(name, len(name), B)


def names_in_bucket(b, k, stem=b"bk"):
    out, i = [], 0
    while len(out) < k:
        nm = b"%s-%d" % (stem, i)
        if bucket(nm) == b:
            out.append(nm)
        i += 1
    return out


class Rig:
    def __init__(self, enable=True):
        self.e = Engine(make_config(**KW))
        self.spec = self.e.register_pod_spec([("fake-pod", "fake")], [], [])
        self.codec = Codec(manage_all_nodes=True)
        self.e.refs_enable()
        self.on = enable
        if enable:
            self.e.node_dir_enable()
            self.e.node_dir_enable()  # idempotent
        self.handle = {}  # name -> handle of the existing nodes
        self.entry = {}   # handle -> name of every directory entry (existing, zombie or placeholder)
        self.uid = {}     # handle -> [uid, stale, the name it was stored for]

    def close(self):
        self.e.close()
        self.codec.close()

    # ---- the rule, record by record in event order ----
    def apply(self, name, h, st, deleted, uid, zombie=False):
        if st != abi.OK:
            return
        h = int(h)
        if deleted:
            self.handle.pop(name, None)
            if not zombie:
                self.entry.pop(h, None)
            self.uid.setdefault(h, [b"", False, name])[1] = True
        else:
            self.handle[name] = h
            self.entry[h] = name
            u = self.uid.get(h)
            if u is None or not u[0] or u[1]:
                self.uid[h] = [uid if 0 < len(uid) <= abi.UID_MAX else b"", False, name]

    def typed(self, names, op=abi.OP_UPSERT, zombie=False):
        ar = abi.Arena()
        ev = np.zeros(len(names), abi.NODE_EVENT_DTYPE)
        ev["op"], ev["managed"], ev["lockable"] = op, 1, 1
        for i, n in enumerate(names):
            ev[i]["name"] = ar.ref(n.decode())
        h, s = self.e.ingest_nodes_raw(ev, bytes(ar.buf))
        for n, hh, st in zip(names, h, s):
            self.apply(n, hh, st, op == abi.OP_DELETE, b"", zombie)
        return h, s

    def framed(self, lines, zombie=False):
        """lines: (type, name, uid or None: no uid member; a str uid is written raw between the quotes)"""
        docs = []
        for typ, name, uid in lines:
            d = node_doc(dict(name=name.decode(), managed=True, lockable=True, nodeInfo={}, addresses=[], allocatable={},
                              capacity={}, phase=""))
            d["metadata"]["resourceVersion"] = "5"
            if uid is not None:
                d["metadata"]["uid"] = "@UID@"
            raw = json.dumps(d, separators=(",", ":")).encode()
            if uid is not None:
                raw = raw.replace(b"@UID@", uid if isinstance(uid, bytes) else uid.encode())
            docs.append(wf.wrap(raw, typ))
        stream = b"".join(docs)
        frames, _u, _nh, sid = self.e.frame_watch(stream)
        assert len(frames) == len(lines)
        h, s, _n = self.e.ingest_nodes_framed(self.codec, sid, np.arange(len(lines)))
        for (typ, name, uid), f, hh, st in zip(lines, frames, h, s):
            esc = bool(f["flags"] & abi.FRAME_ESC_UID)
            u = b"" if uid is None or esc else (uid if isinstance(uid, bytes) else uid.encode())
            self.apply(name, hh, st, typ == "DELETED", u, zombie)
        return h, s

    def bind(self, handles, uids, bad=0):
        assert self.e.node_bind(handles, uids) == bad
        if not bad:
            for h, u in zip(handles, uids):
                self.uid[int(h)] = [bytes(u), False, self.entry[int(h)]]

    def pods(self, node_handles=None, node_names=None):
        n = len(node_handles if node_handles is not None else node_names)
        ar = abi.Arena()
        ev = np.zeros(n, abi.POD_EVENT_DTYPE)
        ev["op"], ev["handle"], ev["spec_id"] = abi.OP_UPSERT, -1, self.spec
        ev["creation_unix"], ev["phase"], ev["flags"] = T0 - 90, abi.PHASE_PENDING, abi.POD_STATUS_NONEMPTY
        ev["node_handle"] = node_handles if node_handles is not None else -1
        if node_names is not None:
            for i, nm in enumerate(node_names):
                ev[i]["node_name"] = ar.ref(nm.decode())
        h, s, _ = self.e.ingest_pods_raw(ev, bytes(ar.buf))
        assert not s.any()
        return h

    # ---- the checks ----
    def lookups(self, names, where=""):
        got = self.e.node_lookup(names)
        assert list(got) == [self.handle.get(bytes(n), -1) for n in names], where
        return got

    def expect(self, h, any_slot=False):
        u, stale, whose = self.uid.get(int(h), [b"", False, None])
        stored = u if self.on and (any_slot or not stale) else b""
        if int(h) in self.entry and whose != self.entry[int(h)]:
            stored = b""  # (another node's: a placeholder made in a slot a deleted node left)
        if int(h) in self.entry:
            return (abi.OK, b"", self.entry[int(h)], stored)
        if any_slot and stored:
            return (abi.REF_NONE, b"", b"", stored)
        return NOT_FOUND

    def refs(self, handles, flags=0, where=""):
        refs, blob = self.e.refs_lookup(abi.KIND_NODES, [int(h) for h in handles], flags)
        check_layout(refs, blob, where)
        assert Engine.ref_items(refs, blob) == [self.expect(h, flags & abi.REFS_ANY_SLOT) for h in handles], where
        return refs

    def everything(self, where):
        self.lookups(sorted(self.handle) + [b"no-such-node"], where)
        hs = sorted(set(self.entry) | set(self.uid))
        self.refs(hs, 0, where)
        self.refs(hs, abi.REFS_ANY_SLOT, where + ", any slot")


NAMES = [b"n", b"x" * 15, b"x" * 16, b"x" * 17, b"w" * 253, b"same-in-all-but-the-last-byte-A", b"same-in-all-but-the-last-byte-B",
         b"node-7", b"worker-a"]


def test_lookup_every_name_length_and_the_names_no_node_has():
    r = Rig()
    h, s = r.typed(NAMES)
    assert not s.any() and len(set(h)) == len(NAMES)
    got = r.lookups(NAMES + [b"", b"w" * 254, b"w" * 252, b"x" * 14, b"x" * 18, b"same-in-all-but-the-last-byte-C", b"N", b"n" * 2])
    assert list(got[:len(NAMES)]) == list(h) and (got[len(NAMES):] == -1).all()
    st = r.e.node_dir_stats()
    # an empty name and one of 254 bytes are not probed
    assert st["lookups"] == len(NAMES) + 6 and st["hits"] == len(NAMES) and st["unbound"] == len(NAMES) and st["notes"] == 0
    assert st["bytes"] >= B * CN * (abi.UID_MAX + 1)
    assert len(r.e.node_lookup([])) == 0
    # kwok_node_has agrees
    for nm in NAMES:
        assert r.e.node_has(nm.decode())
    r.everything("typed creates carry no uid")
    r.close()


def test_a_shared_and_a_full_bucket():
    r = Rig()
    full = names_in_bucket(5, CN + 1)
    assert len(set(bucket(n) for n in full)) == 1
    h, s = r.framed([("ADDED", n, UID36 % i) for i, n in enumerate(full)])
    assert list(s) == [abi.OK] * CN + [abi.EFULL] and h[CN] == -1
    assert sorted(h[:CN]) == list(range(5 * CN, 6 * CN))
    r.lookups(full, "a full bucket")  # the 33rd: -1
    assert r.e.node_lookup([full[CN]])[0] == -1
    assert r.e.node_dir_stats()["notes"] == CN  # the refused create stored no uid
    r.everything("a full bucket")
    # its neighbours are untouched
    other = names_in_bucket(6, 3, b"nb") + names_in_bucket(4, 2, b"nb")
    r.typed(other)
    r.everything("neighbours")
    # delete from the middle of the full bucket: the 33rd fits, in the freed slot, under its own uid
    gone = full[13]
    hd, sd = r.typed([gone], abi.OP_DELETE)
    assert not sd.any()
    h2, s2 = r.framed([("ADDED", full[CN], UID36 % 77)])
    assert not s2.any() and h2[0] == hd[0]
    assert r.expect(h2[0]) == (abi.OK, b"", full[CN], UID36 % 77)
    r.everything("the freed slot taken")
    r.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_lookups_of_many_names_with_repeats(n):
    r = Rig()
    names = [b"fleet-%04d" % i for i in range(300)]
    r.typed(names)
    r.typed(names[:40], abi.OP_DELETE)
    rng = np.random.default_rng(n)
    pool = names + [b"ghost-%d" % i for i in range(20)] + [b"", b"q" * 254]
    ask = [pool[i] for i in rng.integers(0, len(pool), n)]
    got = r.lookups(ask, "%d names" % n)
    if n >= 255:
        assert (got >= 0).any() and (got < 0).any()
    r.close()


def test_deleted_zombie_and_placeholder_entries():
    r = Rig()
    h, _s = r.framed([("ADDED", b"plain", UID36 % 1), ("ADDED", b"held", UID36 % 2)])
    r.pods(node_handles=[int(h[1])] * 3)
    # a deleted node: -1, its entry gone, its uid what the slot last stored
    r.framed([("DELETED", b"plain", UID36 % 1)])
    assert r.e.node_lookup([b"plain"])[0] == -1
    assert r.expect(h[0], True) == (abi.REF_NONE, b"", b"", UID36 % 1) and r.expect(h[0]) == NOT_FOUND
    # a zombie (pods reference it): -1, the entry stays, the uid is stale
    r.framed([("DELETED", b"held", UID36 % 2)], zombie=True)
    assert r.e.node_lookup([b"held"])[0] == -1 and not r.e.node_has("held")
    assert r.expect(h[1]) == (abi.OK, b"", b"held", b"") and r.expect(h[1], True) == (abi.OK, b"", b"held", UID36 % 2)
    r.everything("deleted and zombie")
    assert r.e.node_bind([int(h[0]), int(h[1])], [b"u1", b"u2"]) == 2  # neither exists
    # the zombie exists again under a new uid: the same handle, the new uid
    h2, s2 = r.framed([("ADDED", b"held", UID36 % 3)])
    assert not s2.any() and h2[0] == h[1]
    assert r.expect(h[1]) == (abi.OK, b"", b"held", UID36 % 3)
    r.everything("the zombie re-added")
    # a placeholder made by a pod that names an unknown node: -1, no uid, no bind
    r.pods(node_names=[b"not-yet"])
    assert r.e.node_lookup([b"not-yet"])[0] == -1
    ph = next(hh for hh in range(bucket(b"not-yet") * CN, (bucket(b"not-yet") + 1) * CN) if hh not in r.entry)
    r.entry[ph] = b"not-yet"
    r.refs([ph], 0, "placeholder")
    r.refs([ph], abi.REFS_ANY_SLOT, "placeholder, any slot")
    assert r.e.node_bind([ph], [b"u"]) == 1
    # ... until the node arrives
    h3, _s = r.framed([("ADDED", b"not-yet", UID36 % 4)])
    assert h3[0] == ph
    r.everything("the placeholder became a node")
    # a MODIFIED of a known node under another uid: the old one stays; a typed upsert stores nothing either
    r.framed([("MODIFIED", b"not-yet", UID36 % 5)])
    r.typed([b"not-yet"])
    assert r.expect(ph) == (abi.OK, b"", b"not-yet", UID36 % 4)
    # DELETED then ADDED of one name with different uids in one batch
    r.framed([("DELETED", b"not-yet", UID36 % 4), ("ADDED", b"not-yet", UID36 % 6)])
    assert r.expect(r.handle[b"not-yet"]) == (abi.OK, b"", b"not-yet", UID36 % 6)
    # (the placeholder's pod still references the node: its entry stays)
    r.framed([("DELETED", b"not-yet", UID36 % 6)], zombie=True)
    assert r.expect(ph) == (abi.OK, b"", b"not-yet", b"")
    # frames whose uid the device does not store: escaped, empty, absent, 41 bytes
    hh, _s = r.framed([("ADDED", b"esc", "a\\u0062c"), ("ADDED", b"empty", b""), ("ADDED", b"absent", None), ("ADDED", b"long", b"L" * 41),
                       ("ADDED", b"edge", b"E" * 40), ("ADDED", b"one", b"1")])
    for k in range(4):
        assert r.expect(hh[k])[3] == b""
    assert r.expect(hh[4])[3] == b"E" * 40 and r.expect(hh[5])[3] == b"1"
    r.everything("uids the device does not store")
    r.close()


def test_a_placeholder_in_a_freed_slot_does_not_answer_the_previous_uid():
    r = Rig()
    first, second = names_in_bucket(9, 2, b"ph")
    h, _s = r.framed([("ADDED", first, UID36 % 1)])
    assert h[0] == 9 * CN  # the empty bucket's first slot
    r.framed([("DELETED", first, UID36 % 1)])
    assert r.expect(h[0], True) == (abi.REF_NONE, b"", b"", UID36 % 1)
    r.everything("freed")
    # a pod names a node the engine does not hold: its placeholder takes the freed slot, whose bytes are another node's
    r.pods(node_names=[second])
    r.entry[int(h[0])] = second
    assert r.expect(h[0]) == r.expect(h[0], True) == (abi.OK, b"", second, b"")
    r.everything("a placeholder in the freed slot")
    assert r.e.node_lookup([first, second]).tolist() == [-1, -1]
    # the node arrives: its own uid
    h2, _s = r.framed([("ADDED", second, UID36 % 2)])
    assert h2[0] == h[0] and r.expect(h[0], True) == (abi.OK, b"", second, UID36 % 2)
    r.everything("the placeholder became a node")
    # an upsert of a node recorded without a uid is no create: UNBOUND counts creates
    hh, _s = r.typed([b"plain-a", b"plain-b"])
    before = r.e.node_dir_stats()["unbound"]
    r.typed([b"plain-a", b"plain-b", b"plain-a"])
    assert r.e.node_dir_stats()["unbound"] == before == 2
    # ... and its first frame with a uid brings it
    r.framed([("MODIFIED", b"plain-a", UID36 % 3)])
    assert r.expect(hh[0]) == (abi.OK, b"", b"plain-a", UID36 % 3) and r.e.node_dir_stats()["unbound"] == before
    r.everything("a typed node's first uid")
    r.close()


def test_bind_and_refs_layout():
    r = Rig()
    # the uid starts on (16), before (15) and past (17) a 16-byte unit; the longest name; no uid at all
    names = [b"x" * 16, b"x" * 15, b"x" * 17, b"w" * 253, b"bare", b"n"]
    h, _s = r.typed(names)
    r.refs(h, 0, "no uid yet")
    r.bind(h[:4], [UID36 % 0, b"u" * 40, b"v", UID36 % 3])
    r.bind([int(h[5])], [b"w" * 39])
    refs = r.refs(h, 0, "bound")
    assert [int(x) for x in refs["uid_len"]] == [36, 40, 1, 36, 0, 39] and (refs["status"] == abi.OK).all()
    assert int(refs[3]["name_len"]) == 253
    for hh in h:
        r.refs([hh], 0, "alone")
    r.refs(list(h[::-1]) + [-1, B * CN + 3, 2 ** 31 - 1, int(h[0])], 0, "reversed, with bad handles")
    # refused, storing nothing: 41 bytes, empty; bad handles: negative, past the slots, a free slot
    assert r.e.node_bind(h[:2], [b"z" * 41, b""]) == 2
    free = next(x for x in range(B * CN) if x not in r.entry)
    assert r.e.node_bind([-1, B * CN, 2 ** 31 - 1, free], [b"a", b"b", b"c", b"d"]) == 4
    r.everything("after refused binds")
    # rebinding replaces: shorter, longer
    r.bind(h[:2], [b"s", b"t" * 40])
    r.everything("rebound")
    st = r.e.node_dir_stats()
    assert st["binds"] == 7 and st["unbound"] == len(names)
    # the tick's lists answer in list order, with the uids
    out = r.e.tick(T0)
    for which, handles in ((abi.REFS_HEARTBEAT, list(out.heartbeat_nodes)), (abi.REFS_NODE_INIT, [x for x, _b in out.node_inits])):
        assert len(handles) == len(names)
        refs, blob = r.e.read_refs(which, 0, len(handles))
        check_layout(refs, blob)
        assert Engine.ref_items(refs, blob) == [r.expect(x, True) for x in handles]
    # a bind moves the nodes' stale guard
    r.bind([int(h[4])], [b"late"])
    with pytest.raises(KwokError) as ei:
        r.e.read_refs(abi.REFS_HEARTBEAT, 0, 1)
    assert ei.value.code == abi.EINVAL
    r.close()


def test_a_swept_node_answers_its_uid_under_any_slot():
    r = Rig()
    names = [b"sweep-%d" % i for i in range(8)]
    h, _s = r.framed([("ADDED", n, UID36 % i) for i, n in enumerate(names)])
    r.pods(node_handles=[int(h[7])])
    r.e.resync_begin(abi.KIND_NODES)
    assert r.e.resync_mark(abi.KIND_NODES, h[:4]) == 0
    swept, _rel, _nd = r.e.resync_sweep(abi.KIND_NODES)
    assert sorted(swept) == sorted(int(x) for x in h[4:])
    for k in range(4, 8):
        r.apply(names[k], h[k], abi.OK, True, b"", zombie=k == 7)
    refs = r.refs(swept, abi.REFS_ANY_SLOT, "swept, any slot")
    want = {int(h[k]): abi.OK if k == 7 else abi.REF_NONE for k in range(4, 8)}
    assert [int(x) for x in refs["status"]] == [want[int(x)] for x in swept] and (refs["uid_len"] == 36).all()
    r.refs(swept, 0, "swept")
    r.everything("swept")
    # a swept slot taken by a typed create: not the previous node's uid, under any flag
    h2, _s = r.typed([b"sweep-4"])
    assert h2[0] == h[4] and r.expect(h2[0], True) == (abi.OK, b"", b"sweep-4", b"")
    r.everything("a swept slot reused")
    r.close()


def test_the_same_calls_with_the_directory_off():
    r = Rig(enable=False)
    h, _s = r.typed(NAMES)
    r.framed([("ADDED", b"framed", UID36 % 9)])
    r.lookups(NAMES + [b"framed", b"ghost", b""], "lookup works without the directory")
    assert r.e.node_dir_stats() == dict.fromkeys(abi.NODE_DIR_STATS, 0)
    with pytest.raises(KwokError) as ei:
        r.e.node_bind([int(h[0])], [b"u"])
    assert ei.value.code == abi.EINVAL
    r.everything("node refs have no uid")
    r.typed(NAMES[:2], abi.OP_DELETE)
    assert r.expect(h[0], True) == NOT_FOUND
    r.everything("a cleared entry is not found")
    # enabled late: the nodes that exist have no uid until bound
    r.e.node_dir_enable()
    r.on = True
    r.uid.clear()
    r.everything("enabled late")
    r.bind([r.handle[b"framed"]], [UID36 % 9])
    r.everything("bound late")
    r.close()
