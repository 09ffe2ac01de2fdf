"""GPU: the node uid directory behind the framed node ingests (include/kwok_watch.h,
DESIGN.md §26; nodes.hip: k_nd_frame_recs, k_nd_echo_fix, k_nd_stat_scatter, k_nd_lookup_frames
in place of k_echo_node_handles, k_nd_uid_note behind every node apply pass), record for record against the path without it.

The backends of test_echo_ingest_gpu.py in lockstep: engine `a` has the uid directory, the
echo ledger, the reference directory and the node directory on and takes ALL frames of a
batch through kwok_ingest_nodes_framed_echo - the device-input node ingest: the kept records
from the resident frames by the device-resident index list, every answer merged on the
device; engine `b` has the node directory off and gets the host rule (Python, EchoLock) and
kwok_ingest_nodes_framed on the kept records - not kwok_ingest_nodes_framed_echo with three
directories: k_nd_lookup_frames is checked against the host's name -> handle dict, not against
k_echo_node_handles directly (tests/test_echo_ingest_gpu.py checks that kernel against the same
dict); the oracle is fed b's records.  After every batch, beside what EchoLock.node_batch compares (handles,
statuses, documents the host decided, echoes, watch and echo stats): every kwok_node_lookup
against the host's name -> handle dict, and every node's stored uid (kwok_refs_lookup of
nodes, live and KWOK_REFS_ANY_SLOT) against a dict run by controller.py's _node_put /
_node_pop rule.  After every tick, beside the outputs, counters and kwok_engine_stats: the
node references of the heartbeat and node-init lists, a's with the uids."""
import numpy as np
import pytest

from kwok_amd import abi, codec as host_codec
from kwok_amd.engine import Engine
from test_echo_ingest_gpu import E, EchoLock
from test_ref_dir_gpu import check_layout
from test_uid_ingest_gpu import BOOKMARK, fleet
import watch_frames as wf

pytestmark = pytest.mark.gpu

NOT_FOUND = (abi.ENOTFOUND, b"", b"", b"")
STATUS = dict(addresses=[{"type": "InternalIP", "address": "10.1.2.3"}], allocatable={"cpu": "4"}, capacity={"cpu": "4"})


class NodeLock(EchoLock):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.a.refs_enable()
        self.b.refs_enable()
        self.a.node_dir_enable()
        self.by_name = {}  # decoded name -> handle of the existing nodes
        self.entry = {}    # handle -> name
        self.uid = {}      # handle -> [uid, stale]

    def rule(self, name, h, deleted, uid):
        if deleted:
            self.by_name.pop(name, None)
            self.entry.pop(h, None)
            self.uid.setdefault(h, [b"", False])[1] = True
            return
        self.by_name[name] = h
        self.entry[h] = name
        u = self.uid.get(h)
        if u is None or not u[0] or u[1]:
            self.uid[h] = [uid if 0 < len(uid) <= abi.UID_MAX else b"", False]

    def nodes(self, names, managed=1):
        hs = super().nodes(names, managed)
        for n, h in zip(names, hs):
            self.rule(n.encode(), int(h), False, b"")  # a typed event carries no uid
        self.check("typed nodes")
        return hs

    def node_batch(self, lines, where, as_list=False, want_status=None):
        ha, sta = super().node_batch(lines, where, as_list, want_status)
        if as_list:
            stream = b'{"kind":"NodeList","apiVersion":"v1","metadata":{"resourceVersion":"7"},"items":[' + \
                     b",".join(d for _t, d in lines) + b"]}"
            frames = host_codec.frame_list(stream)[0]
        else:
            stream = b"".join(d if t == "RAW" else wf.wrap(d, t) for t, d in lines)
            frames = host_codec.frame_watch(stream)[0]
        assert len(frames) == len(ha)
        span = lambda f, k: bytes(stream[int(f[k]["off"]):int(f[k]["off"]) + int(f[k]["len"])])  # noqa: E731
        for f, h, s in zip(frames, ha, sta):
            if s != abi.OK:
                continue
            name = span(f, "name")  # (a kept record's name holds no escape: the decode refuses one)
            uid = b"" if f["flags"] & abi.FRAME_ESC_UID else span(f, "uid")
            self.rule(name, int(h), f["type"] == abi.WATCH_DELETED, uid)
        self.check(where)
        return ha, sta

    def expect(self, h, any_slot):
        u, stale = self.uid.get(h, [b"", False])
        stored = u if any_slot or not stale else b""
        if h in self.entry:
            return (abi.OK, b"", self.entry[h], stored)
        return (abi.REF_NONE, b"", b"", stored) if any_slot and stored else NOT_FOUND

    def check(self, where):
        names = sorted(self.by_name) + [b"ghost", b"no-such-node"]
        assert list(self.a.node_lookup(names)) == [self.by_name.get(n, -1) for n in names], where + " lookups"
        assert list(self.b.node_lookup(names)) == [self.by_name.get(n, -1) for n in names], where + " lookups (directory off)"
        hs = sorted(set(self.entry) | set(self.uid))
        for flags in (0, abi.REFS_ANY_SLOT):
            refs, blob = self.a.refs_lookup(abi.KIND_NODES, hs, flags)
            check_layout(refs, blob, where)
            assert Engine.ref_items(refs, blob) == [self.expect(h, flags) for h in hs], "%s uids (flags %d)" % (where, flags)
        assert self.b.node_dir_stats() == dict.fromkeys(abi.NODE_DIR_STATS, 0), where

    def tick(self, where):
        ao = super().tick(where)
        for which, handles in ((abi.REFS_HEARTBEAT, [int(h) for h in ao.heartbeat_nodes]),
                               (abi.REFS_NODE_INIT, [int(h) for h, _b in ao.node_inits])):
            if not handles:
                continue
            ra, ba = self.a.read_refs(which, 0, len(handles))
            rb, bb = self.b.read_refs(which, 0, len(handles))
            check_layout(ra, ba, where)
            want = [self.expect(h, True) for h in handles]
            assert Engine.ref_items(ra, ba) == want, where + " list refs"
            assert Engine.ref_items(rb, bb) == [(s, ns, nm, b"") for s, ns, nm, _u in want], where + " list refs (directory off)"
        return ao


def u(name):
    return b"nu-" + name.encode()


@pytest.mark.parametrize("once", [True, False], ids=["heartbeat-once", "full-body"])
def test_named_node_batches(once):
    t = NodeLock(once=once)
    names = fleet(t, 4)
    new = ["nd-node-%d" % k for k in range(6)]
    # nothing dropped: creates with their uids
    t.node_batch([("ADDED", t.ndoc(nm, "10")) for nm in new], "creates", want_status=[0] * 6)
    assert t.a.node_dir_stats()["notes"] == 6
    t.tick("creates")
    # an all-echo batch: nothing kept, every handle by the grouped lookup
    t.note([(u(nm), b"20") for nm in new + names])
    h, s = t.node_batch([("MODIFIED", t.ndoc(nm, "20")) for nm in new + names], "all echoes", want_status=[E] * 10)
    assert sorted(h) == sorted(t.by_name[nm.encode()] for nm in new + names)
    # MODIFIED of a known node under another uid: the old one stays
    t.node_batch([("MODIFIED", t.ndoc(new[0], "30", uid="another-uid"))], "another uid", want_status=[0])
    assert t.expect(t.by_name[new[0].encode()], False)[3] == u(new[0])
    # the typed fleet's nodes had none: their first framed record brings it
    t.node_batch([("MODIFIED", t.ndoc(names[0], "31"))], "first uid of a typed node", want_status=[0])
    assert t.expect(t.by_name[names[0].encode()], False)[3] == u(names[0])
    # DELETED then ADDED of one name with different uids in one batch; bookmarks and bad lines between records
    h, s = t.node_batch([("DELETED", t.ndoc(new[1], "40")), ("RAW", BOOKMARK), ("ADDED", t.ndoc(new[1], "41", uid="second-life")),
                         ("RAW", b"{not json}\n"), ("RAW", b"\n"), ("DELETED", t.ndoc(new[2], "42"))], "delete and add",
                        want_status=[0, abi.EINVAL, 0, abi.EINVAL, abi.EINVAL, 0])
    assert t.expect(int(h[2]), False)[3] == b"second-life"
    assert t.expect(int(h[5]), True) == (abi.REF_NONE, b"", b"", u(new[2]))
    # escaped uid / resourceVersion: the device does not decide them; an escaped name: its echo has no handle (the
    # name is compared as written; kept, such a document is the decode's KWOK_EDOMAIN: test_json_nodes_gpu.py)
    t.note([(u(new[3]), b"51"), (b"nu-escn", b"53")])
    esc_name = t.ndoc("@N@", "53", uid="nu-escn").replace(b"@N@", new[4][:-1].encode() + b"\\u003%s" % new[4][-1:].encode())
    h, s = t.node_batch([("ADDED", t.ndoc("esc-uid", "50", uid="a\\u0062c")), ("MODIFIED", t.ndoc(new[3], "5\\u0031")),
                         ("MODIFIED", esc_name)], "escapes", want_status=[abi.EDOMAIN, abi.EDOMAIN, E])
    assert list(h) == [-1] * 3 and new[4].encode() in t.by_name
    t.tick("after the named batches")
    # non-empty statuses (the documents the host completes: the second apply pass), alone and mixed with empty ones
    t.node_batch([("ADDED", t.ndoc("st-%d" % k, "60", **STATUS)) for k in range(3)], "statuses alone", want_status=[0] * 3)
    t.node_batch([("ADDED", t.ndoc("mx-%d" % k, "61", **(STATUS if k % 2 else {}))) for k in range(7)] +
                 [("DELETED", t.ndoc("st-1", "62"))], "statuses mixed", want_status=[0] * 8)
    t.tick("after the statuses")
    t.close()


def test_block_edges():
    """1 / 255 / 256 / 257 / 1025 records: creates, then every second record an echo (the lookup groups and the note's
    ranges across block and wave edges)"""
    t = NodeLock(once=True)
    first = 0
    for n in (1, 255, 256, 257, 1025):
        # (64 buckets x 32 slots hold them: 1794 names, 28 per bucket on average, no bucket full with this stem)
        names = ["e%05d" % k for k in range(first, first + n)]
        first += n
        h, s = t.node_batch([("ADDED", t.ndoc(nm, "70")) for nm in names], "%d creates" % n)
        full = int((s == abi.EFULL).sum())
        assert set(s.tolist()) <= {abi.OK, abi.EFULL} and full < n // 4 + 1
        t.note([(u(nm), b"77") for nm in names[::2]])
        h2, s2 = t.node_batch([("MODIFIED", t.ndoc(nm, "77" if i % 2 == 0 else "78")) for i, nm in enumerate(names)],
                              "%d half echoes" % n)
        assert list(s2[::2]) == [E] * len(names[::2])
        assert list(h2[::2]) == [t.by_name.get(nm.encode(), -1) for nm in names[::2]]
    t.tick("edges")
    t.close()


def test_relist_with_replace_sweeps_nodes():
    t = NodeLock(once=True)
    fleet(t, 3)
    names = ["rl-%d" % k for k in range(10)]
    t.node_batch([("ADDED", t.ndoc(nm, "80")) for nm in names], "before the relist")
    t.tick("before the relist")
    for x in (t.a, t.b):
        x.resync_begin(abi.KIND_NODES)
    listed = ["node-000", "node-001", "node-002"] + names[:6]
    t.node_batch([("ADDED", t.ndoc(nm, "81")) for nm in listed], "the list", as_list=True, want_status=[0] * 9)
    sa, sb = (x.resync_sweep(abi.KIND_NODES)[0] for x in (t.a, t.b))
    assert list(sa) == list(sb) == sorted(t.by_name[nm.encode()] for nm in names[6:])
    # the controller's _end_resync: the swept nodes' uids from the device, their notes forgotten
    refs, blob = t.a.refs_lookup(abi.KIND_NODES, sa, abi.REFS_ANY_SLOT)
    got = Engine.ref_items(refs, blob)
    assert [g[3] for g in got] == [t.uid[int(h)][0] for h in sa] == [u(t.entry[int(h)].decode()) for h in sa]
    assert all(g[0] == abi.REF_NONE for g in got)
    # (the oracle has no sweep: the same DELETE records)
    ar = abi.Arena()
    ev = np.zeros(len(sa), abi.NODE_EVENT_DTYPE)
    ev["op"] = abi.OP_DELETE
    for i, h in enumerate(sa):
        ev[i]["name"] = ar.ref(t.entry[int(h)].decode())
    assert not t.o.ingest_nodes_raw(ev, bytes(ar.buf))[1].any()
    for h in sa:
        nm = t.entry[int(h)]
        t.node_handle.pop(nm.decode(), None)
        t.rule(nm, int(h), True, b"")
    t.check("swept")
    t.tick("after the sweep")
    # a swept slot created into again through a typed event: not the swept node's uid
    t.nodes([names[9]])
    assert t.expect(t.by_name[names[9].encode()], True)[3] == b""
    t.close()


@pytest.mark.parametrize("once", [True, False], ids=["heartbeat-once", "full-body"])
def test_fuzz(once):
    """~900 node lines over 120 names in 6 batches with a tick between them: adds, modifies under the same and under
    other uids, deletes followed by adds, noted versions coming back as echoes, bookmarks, non-empty statuses"""
    t = NodeLock(once=once, seed=29)
    rng = t.rng
    life = {}  # name -> the uid of its current life
    total = 0
    for r in range(6):
        notes = {}
        for k in rng.choice(120, 40, replace=False).tolist():
            nm = "fz-%d" % k
            if nm in life:
                notes[nm] = b"%d" % (1000 * (r + 1) + k)
        if notes:
            t.note([(life[nm].encode(), v) for nm, v in notes.items()])
        lines = []
        for _ in range(int(rng.integers(120, 180))):
            nm = "fz-%d" % int(rng.integers(0, 120))
            roll = int(rng.integers(0, 10))
            if roll == 0:
                lines.append(("RAW", BOOKMARK))
            elif nm not in life or roll == 1:
                if nm in life:
                    lines.append(("DELETED", t.ndoc(nm, "9", uid=life[nm])))
                life[nm] = "nu-%s-%d-%d" % (nm, r, len(lines))
                lines.append(("ADDED", t.ndoc(nm, "10", uid=life[nm], **(STATUS if roll == 2 else {}))))
            elif roll == 3:
                lines.append(("DELETED", t.ndoc(nm, "11", uid=life.pop(nm))))
                notes.pop(nm, None)
            elif nm in notes and roll < 8:
                lines.append(("MODIFIED", t.ndoc(nm, notes.pop(nm).decode(), uid=life[nm])))
            else:
                lines.append(("MODIFIED", t.ndoc(nm, "12", uid=life[nm] if roll < 9 else "stranger", **(STATUS if roll == 4 else {}))))
        t.node_batch(lines, "fuzz batch %d" % r)
        total += len(lines)
        t.tick("fuzz tick %d" % r)
    s = t.a.node_dir_stats()
    assert total > 700 and s["notes"] > 100 and s["hits"] > 5 and t.a.echo_stats()["dropped"] > 5
    t.close()
