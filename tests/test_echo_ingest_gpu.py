"""GPU: kwok_ingest_pods_framed_echo / kwok_ingest_nodes_framed_echo against the host
path, record for record (include/kwok_watch.h; echo.hip).

Three backends in lockstep, as in test_uid_ingest_gpu.py: engine `a` takes ALL frames of
every batch with one call and drops the echoes on the device; engine `b` gets the host
rule (Controller._ingest_frames' loop over controller.Echoes, restated below) and then
kwok_ingest_pods_framed_uid / kwok_ingest_nodes_framed on `keep`; the oracle `o` is fed
b's kept records through the host codec.  After every batch: status, handle and released
address of every record, the runs, the documents the host decided, the echo / uid / watch
stats; after every tick: every output list, the counters and the pod state."""
import json

import numpy as np
import pytest

import watch_frames as wf
from harness import node_doc
from kwok_amd import abi
from kwok_amd.controller import NOT_SENT, Echoes, ingest_pod_runs
from kwok_amd.engine import Engine, KwokError, make_config
from kwok_amd.codec import Codec
from test_uid_ingest_gpu import BOOKMARK, KW, Lock, fleet, spec_of

pytestmark = pytest.mark.gpu

INGESTIBLE = (abi.WATCH_ADDED, abi.WATCH_MODIFIED, abi.WATCH_DELETED)


class EchoLock(Lock):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.b.uid_dir_enable()
        self.a.echo_enable()
        self.echo = Echoes()   # b's ledger (keys and versions as bytes)
        self.want = dict(matched=0, dropped=0, kept_matched=0)
        self.rv = 1000

    # ---- the engine's own patches: a note on both sides ----
    def note(self, pairs):
        """pairs: (uid, rv) as a patch's response names them"""
        st = self.a.echo_update([abi.ECHO_NOTE] * len(pairs), [u for u, _r in pairs], [r for _u, r in pairs])
        assert not st.any()
        for u, r in pairs:
            self.echo.note(u, r)

    def forget(self, handles):
        """the tick's delete list / a sweep: the pods leave b's map, their notes both ledgers"""
        gone = set(int(h) for h in handles)
        us = [u for u, h in self.by_uid.items() if h in gone]
        if us:
            self.a.echo_update([abi.ECHO_FORGET] * len(us), us, [b""] * len(us))
        for u in us:
            self.echo.forget(u)
        super().forget(gone)

    def doc(self, key, node="node-000", spec=0, uid=None, rv=None, **kw):
        d = json.loads(super().doc(key, node, spec, uid, **kw))
        if rv is None:
            self.rv += 1
            rv = str(self.rv)
        d["metadata"]["resourceVersion"] = rv
        return json.dumps(d, separators=(",", ":")).encode()

    # ---- the host rule: _ingest_frames' loop ----
    def host_rule(self, stream, frames):
        """-> (keep, uids, deleted, echoed, status): status[i] is what kwok_watch.h answers for a record the
        controller never sends (EINVAL: not ingestible; EDOMAIN: an escaped uid / resourceVersion, which the
        device does not decide; ECHO: dropped)"""
        n = len(frames)
        status = np.full(n, abi.EINVAL, np.int32)
        keep, uids, deleted, echoed, seen = [], [], [], [], set()
        for i, f in enumerate(frames):
            if f["status"] != abi.OK or f["type"] not in INGESTIBLE:
                continue
            if f["flags"] & (abi.FRAME_ESC_UID | abi.FRAME_ESC_RV):
                status[i] = abi.EDOMAIN
                continue
            span = lambda k: bytes(stream[int(f[k]["off"]):int(f[k]["off"]) + int(f[k]["len"])])  # noqa: E731
            uid, rv = span("uid"), span("resource_version")
            dl = f["type"] == abi.WATCH_DELETED
            m = (not dl) and self.echo.is_echo(uid, rv)
            self.want["matched"] += m
            if m and uid not in seen:
                self.want["dropped"] += 1
                status[i] = abi.ECHO
                echoed.append(i)
                continue
            self.want["kept_matched"] += m
            seen.add(uid)
            if dl:
                self.echo.forget(uid)
            keep.append(i)
            uids.append(uid)
            deleted.append(dl)
        return keep, uids, deleted, echoed, status

    def compare_echo(self, where):
        s = self.a.echo_stats()
        assert {k: s[k] for k in self.want} == self.want, "%s: %r" % (where, s)
        assert s["live_uids"] == len(self.echo.rv), where

    # ---- one pod batch: lines = [(type, document bytes)] ----
    def batch(self, lines, where, as_list=False, want_status=None, want_runs=None):
        docs = [d for _t, d in lines]
        if as_list:
            stream = b'{"kind":"PodList","apiVersion":"v1","metadata":{"resourceVersion":"7"},"items":[' + b",".join(docs) + b"]}"
            fa, _ia, _nha, sa = self.a.frame_list(stream)
            fb, _ib, _nhb, sb = self.b.frame_list(stream)
        else:
            stream = b"".join(d if t == "RAW" else wf.wrap(d, t) for t, d in lines)
            fa, _ua, _nha, sa = self.a.frame_watch(stream)
            fb, _ub, _nhb, sb = self.b.frame_watch(stream)
        assert fa.tobytes() == fb.tobytes() and len(fa) == len(lines)
        n = len(fa)
        # a: one call over all frames
        ha, sta, rela, nha, runs_a, ne = self.a.ingest_pods_framed_echo(self.codec, sa, np.arange(n))
        # b: the host rule, then the by-uid entry on keep
        keep, uids, deleted, echoed, stb = self.host_rule(stream, fb)
        hb = np.full(n, -1, np.int32)
        relb = np.zeros(n, np.uint32)
        if echoed:  # (the echoes' handles: what the caller marks in a resync session)
            hb[echoed] = self.b.uid_lookup([bytes(stream[int(fb[i]["uid"]["off"]):int(fb[i]["uid"]["off"]) + int(fb[i]["uid"]["len"])])
                                            for i in echoed])
        runs_b = nhb = 0
        if keep:
            hk, sk, rk, nhb, runs_b = self.b.ingest_pods_framed_uid(self.codec, sb, np.array(keep, np.uint32))
            hb[keep], stb[keep], relb[keep] = hk, sk, rk
            # the oracle: the records b sent, cut into runs by the host map
            sent = [q for q in range(len(keep)) if sk[q] != abi.EDOMAIN or 0 < len(uids[q]) <= abi.UID_MAX]
            if sent:
                dec = self.codec.decode_pods([docs[keep[q]] for q in sent], strict=False)
                ro = np.zeros(len(sent), np.uint32)

                def send(idx, ops, hv):
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
                    ro[idx] = r2
                    return h2, s2

                ho, so, runs_o = ingest_pod_runs(None, self.by_uid, np.empty(len(sent)), [uids[q] for q in sent],
                                                 [deleted[q] for q in sent], None, sender=send)
                assert list(ho) == [int(hk[q]) for q in sent] and list(so) == [int(sk[q]) for q in sent], where + " (b / oracle)"
                assert list(ro) == [int(rk[q]) for q in sent] and runs_o == runs_b, where + " (b / oracle)"
        assert list(sta) == list(stb), "%s statuses\n%r\n%r" % (where, list(sta), list(stb))
        assert list(ha) == list(hb), "%s handles\n%r\n%r" % (where, list(ha), list(hb))
        assert list(rela) == list(relb), where + " released"
        assert runs_a == runs_b and nha == nhb and ne == len(echoed), "%s runs %d / %d, host %d / %d, echoes %d / %d" % (
            where, runs_a, runs_b, nha, nhb, ne, len(echoed))
        assert self.a.watch_stats() == self.b.watch_stats(), where + " watch stats"
        ua, ub = self.a.uid_stats(), self.b.uid_stats()
        assert ua == ub, "%s uid stats %r vs %r" % (where, ua, ub)
        self.compare_echo(where)
        if want_status is not None:
            assert list(sta) == list(want_status), "%s: %r" % (where, list(sta))
        if want_runs is not None:
            assert runs_a == want_runs, "%s: %d runs" % (where, runs_a)
        self.state(where)
        return ha, sta, rela

    # ---- one node batch: lines = [(type, node event dict, rv)] or ("RAW", bytes, None) ----
    def ndoc(self, name, rv, uid=None, **kw):
        ev = dict(name=name, managed=True, lockable=True, nodeInfo={}, addresses=[], allocatable={}, capacity={}, phase="")
        ev.update(kw)
        d = node_doc(ev)
        d["metadata"]["uid"] = "nu-" + name if uid is None else uid
        d["metadata"]["resourceVersion"] = rv
        return json.dumps(d, separators=(",", ":")).encode()

    def node_batch(self, lines, where, as_list=False, want_status=None):
        docs = [d for _t, d in lines]
        if as_list:
            stream = b'{"kind":"NodeList","apiVersion":"v1","metadata":{"resourceVersion":"7"},"items":[' + b",".join(docs) + b"]}"
            fa, _ia, _nha, sa = self.a.frame_list(stream)
            fb, _ib, _nhb, sb = self.b.frame_list(stream)
        else:
            stream = b"".join(d if t == "RAW" else wf.wrap(d, t) for t, d in lines)
            fa, _ua, _nha, sa = self.a.frame_watch(stream)
            fb, _ub, _nhb, sb = self.b.frame_watch(stream)
        assert fa.tobytes() == fb.tobytes() and len(fa) == len(lines)
        n = len(fa)
        ha, sta, nha, ne = self.a.ingest_nodes_framed_echo(self.codec, sa, np.arange(n))
        keep, _uids, deleted, echoed, stb = self.host_rule(stream, fb)
        hb = np.full(n, -1, np.int32)
        name = lambda i: bytes(stream[int(fb[i]["name"]["off"]):int(fb[i]["name"]["off"]) + int(fb[i]["name"]["len"])]).decode()  # noqa: E731
        for i in echoed:  # (the controller's node_handle map)
            hb[i] = self.node_handle.get(name(i), -1)
        nhb = 0
        if keep:
            hk, sk, nhb = self.b.ingest_nodes_framed(self.codec, sb, np.array(keep, np.uint32))
            hb[keep], stb[keep] = hk, sk
            dec = self.codec.decode_nodes([docs[i] for i in keep], strict=False)
            ar = abi.Arena()
            ar.buf = bytearray(dec.buf)
            recs = np.zeros(len(keep), abi.NODE_EVENT_DTYPE)
            for q in range(len(keep)):
                assert dec.status[q] == abi.OK
                recs[q] = np.frombuffer(bytes(dec.nodes[q]), abi.NODE_EVENT_DTYPE)[0]
                recs[q]["op"] = abi.OP_DELETE if deleted[q] else abi.OP_UPSERT
            ho, so = self.o.ingest_nodes_raw(recs, bytes(ar.buf))
            assert list(ho) == list(hk) and list(so) == list(sk), where + " (b / oracle)"
            for q, i in enumerate(keep):
                if sk[q] == abi.OK:
                    if deleted[q]:
                        self.node_handle.pop(name(i), None)
                    else:
                        self.node_handle[name(i)] = int(hk[q])
        assert list(sta) == list(stb), "%s statuses\n%r\n%r" % (where, list(sta), list(stb))
        assert list(ha) == list(hb), "%s handles\n%r\n%r" % (where, list(ha), list(hb))
        assert nha == nhb and ne == len(echoed), where
        assert self.a.watch_stats() == self.b.watch_stats(), where + " watch stats"
        self.compare_echo(where)
        if want_status is not None:
            assert list(sta) == list(want_status), "%s: %r" % (where, list(sta))
        return ha, sta


E = abi.ECHO


@pytest.mark.parametrize("once", [True, False], ids=["heartbeat-once", "full-body"])
def test_named_pod_batches(once):
    t = EchoLock(once=once)
    names = fleet(t)
    node = lambda k: names[k % len(names)]  # noqa: E731
    u = lambda k: b"u-" + k.encode()  # noqa: E731
    t.batch([("ADDED", t.doc("p%d" % k, node(k), spec=k % 2)) for k in range(40)], "creates", want_status=[0] * 40, want_runs=1)
    t.tick("creates")
    # the pod patches' echoes: every one of them dropped, with its live handle; nothing reaches the ingest
    t.note([(u("p%d" % k), b"%d" % (2000 + k)) for k in range(40)])
    h, s, _r = t.batch([("MODIFIED", t.doc("p%d" % k, node(k), spec=k % 2, rv=str(2000 + k))) for k in range(40)],
                       "all echoes", want_status=[E] * 40, want_runs=0)
    assert sorted(h) == sorted(t.by_uid[u("p%d" % k)] for k in range(40))
    t.tick("steady")
    # an echo before and after a real change of the same object; an echo of another object between them
    t.note([(u("p1"), b"3001"), (u("p1"), b"3002"), (u("p2"), b"3003"), (u("p3"), b"3004")])
    t.batch([("MODIFIED", t.doc("p1", node(1), spec=1, rv="3001")),
             ("MODIFIED", t.doc("p1", node(1), spec=1, status_nonempty=True)),
             ("MODIFIED", t.doc("p2", node(2), rv="3003")),
             ("MODIFIED", t.doc("p1", node(1), spec=1, rv="3002")),
             ("MODIFIED", t.doc("p5", node(5), spec=1)),
             ("MODIFIED", t.doc("p3", node(3), spec=1, rv="3004"))], "echo, change, echo",
            want_status=[E, 0, E, 0, 0, E], want_runs=1)
    # ... the consumed one matches no more; a note that never came back stays
    t.batch([("MODIFIED", t.doc("p1", node(1), spec=1, rv="3002"))], "consumed", want_status=[0])
    # an echo behind a Deleted line: never an echo (the Deleted forgot the notes), a Deleted is never one either
    t.note([(u("p6"), b"3100"), (u("p6"), b"3101"), (u("p7"), b"3102")])
    t.batch([("DELETED", t.doc("p6", node(6), rv="3100")), ("MODIFIED", t.doc("p6", node(6), rv="3101")),
             ("MODIFIED", t.doc("p7", node(7), spec=1, rv="3102")), ("DELETED", t.doc("p7", node(7), spec=1, rv="3102"))],
            "echoes around Deleted lines", want_status=[0, abi.ENOTFOUND, E, 0])
    t.tick("after deletes")
    # the finalizer patch's echo of a pod the tick already freed: its earlier notes go with the delete list, the
    # patch's note comes after it; the echo is dropped with no handle, the Deleted line is not sent
    t.note([(u("p10"), b"3199")])
    t.batch([("MODIFIED", t.doc("p%d" % k, node(k), spec=k % 2, deleting=True)) for k in (10, 11)], "deletion-marked")
    out = t.tick("tick deletes")  # (forget(): the delete list)
    assert len(out.deletes) == 2
    assert list(t.a.echo_match([u("p10")], [b"3199"], [0])) == [0] and not t.echo.is_echo(u("p10"), b"3199")
    t.note([(u("p10"), b"3200"), (u("p11"), b"3201")])
    h, s, _r = t.batch([("MODIFIED", t.doc("p10", node(10), rv="3200")), ("MODIFIED", t.doc("p11", node(11), spec=1, rv="3201")),
                        ("DELETED", t.doc("p10", node(10))), ("DELETED", t.doc("p11", node(11), spec=1))],
                       "finalizer echoes", want_status=[E, E, NOT_SENT, NOT_SENT], want_runs=0)
    assert list(h) == [-1] * 4
    t.tick("after the finalizer echoes")
    # escaped uid / resourceVersion: not decided on the device, nothing changes; other frames that are no pod events
    t.note([(u("p12"), b"3300"), (b"u-esc", b"3301")])
    t.batch([("MODIFIED", t.doc("p12", node(12), rv="33\\u00300")), ("MODIFIED", t.doc("esc", node(1), uid="u\\u002desc", rv="3301")),
             ("RAW", BOOKMARK), ("MODIFIED", t.doc("p12", node(12), rv="3300")), ("RAW", b'{"type":"ADDED","object":[]}\n'),
             ("RAW", b"\r\n"), ("ADDED", t.doc("empty", node(2), uid="", rv="3300")), ("ADDED", t.doc("long", node(2), uid="L" * 41)),
             ("MODIFIED", t.doc("p13", node(13), spec=1, rv="9" * 25))], "frames outside the domain",
            want_status=[abi.EDOMAIN, abi.EDOMAIN, abi.EINVAL, E, abi.EINVAL, abi.EINVAL, abi.EDOMAIN, abi.EDOMAIN, 0])
    # List items: a relist whose items are echoes beside real ones; the echoes' handles are what the caller marks
    t.note([(u("p%d" % k), b"%d" % (3400 + k)) for k in range(20, 30)])
    for x in (t.a, t.b):
        x.resync_begin(abi.KIND_PODS)
    live = sorted(t.by_uid.items(), key=lambda kv: kv[1])
    items = []
    for uid, _h in live:
        key, nd, sp, uu = t.meta[uid]
        k = int(key[1:]) if key[1:].isdigit() else -1
        items.append(("ADDED", t.doc(key, nd, spec=sp, uid=uu, rv=str(3400 + k) if 20 <= k < 30 else None)))
    h, s, _r = t.batch(items, "relist with echoes", as_list=True)
    assert int((s == E).sum()) == 10 and (h[s == E] >= 0).all()
    for x in (t.a, t.b):
        assert x.resync_mark(abi.KIND_PODS, h[s == E]) == 0
    sa, _ra, _na = t.a.resync_sweep(abi.KIND_PODS)
    sb, _rb, _nb = t.b.resync_sweep(abi.KIND_PODS)
    assert list(sa) == list(sb) == []
    t.tick("after the relist")
    s = t.a.echo_stats()
    assert s["dropped"] >= 56 and s["kept_matched"] >= 1
    t.close()


def test_block_edges_and_one_uid():
    """255 / 256 / 257 / 1025 records (one thread per record, 256 per block): creates, then every second record an echo;
    then 300 lines of ONE pod in one batch"""
    t = EchoLock(once=True)
    names = fleet(t, 24)
    first = 0
    for n in (255, 256, 257, 1025):
        keys = ["e%d" % k for k in range(first, first + n)]
        first += n
        h, s, _r = t.batch([("ADDED", t.doc(k, names[i % 24])) for i, k in enumerate(keys)], "%d creates" % n, want_runs=1)
        assert not s.any()
        t.note([(b"u-" + k.encode(), b"77") for k in keys[::2]])
        h2, s2, _r = t.batch([("MODIFIED", t.doc(k, names[i % 24], rv="77" if i % 2 == 0 else None)) for i, k in enumerate(keys)],
                             "%d half echoes" % n, want_runs=1)
        assert list(s2) == [E if i % 2 == 0 else 0 for i in range(n)] and list(h2) == list(h)
    t.tick("edges")
    t.note([(b"u-e0", b"%d" % (500 + k)) for k in range(8)])
    lines = [("MODIFIED", t.doc("e0", names[0], rv=str(500 + k if k < 4 else 208 + k) if k < 4 or k >= 296 else None)) for k in range(300)]
    _h, s, _r = t.batch(lines, "300 lines of one pod", want_runs=1)
    assert list(s) == [E] * 4 + [0] * 296  # (the last four match behind kept records: consumed and kept)
    t.compare_echo("one pod")
    assert t.a.echo_stats()["live_uids"] == 0
    t.tick("one pod")
    t.close()


def test_named_node_batches():
    t = EchoLock(once=True)
    names = fleet(t, 4)  # (typed events: the ledger knows nothing of them)
    new = ["echo-node-%d" % k for k in range(6)]
    t.node_batch([("ADDED", t.ndoc(nm, "10")) for nm in new], "node creates", want_status=[0] * 6)
    t.tick("nodes")
    # the heartbeat patches' echoes: all dropped, with the handle the name resolves to
    t.note([(b"nu-" + nm.encode(), b"20") for nm in new + names])
    h, s = t.node_batch([("MODIFIED", t.ndoc(nm, "20")) for nm in new + names], "all echoes", want_status=[E] * 10)
    assert (h >= 0).all() and len(set(h)) == 10
    # echo, change, echo of one node; a bookmark; an escaped version; a node without a uid (ingested by name);
    # a Deleted node forgets; an echo of a node the engine does not hold has no handle
    t.note([(b"nu-" + new[0].encode(), b"31"), (b"nu-" + new[0].encode(), b"32"), (b"nu-" + new[1].encode(), b"33"),
            (b"nu-" + new[2].encode(), b"34"), (b"nu-ghost", b"35"), (b"nu-" + new[3].encode(), b"36")])
    t.node_batch([("MODIFIED", t.ndoc(new[0], "31")), ("MODIFIED", t.ndoc(new[0], "40", lockable=False)),
                  ("MODIFIED", t.ndoc(new[0], "32")), ("RAW", BOOKMARK), ("MODIFIED", t.ndoc(new[1], "3\\u0033")),
                  ("MODIFIED", t.ndoc(new[4], "41", uid="")), ("DELETED", t.ndoc(new[2], "34")),
                  ("MODIFIED", t.ndoc(new[2], "34")), ("MODIFIED", t.ndoc("ghost", "35")), ("MODIFIED", t.ndoc(new[3], "36"))],
                 "mixed node lines", want_status=[E, 0, 0, abi.EINVAL, abi.EDOMAIN, 0, 0, 0, E, E])
    t.tick("after the node lines")
    # a NodeList whose items are echoes
    t.note([(b"nu-" + nm.encode(), b"50") for nm in new[3:]])
    h, s = t.node_batch([("ADDED", t.ndoc(nm, "50" if k >= 3 else "51")) for k, nm in enumerate(new)], "node list", as_list=True)
    assert list(s[3:]) == [E] * 3 and (h[3:] >= 0).all()
    t.tick("after the node list")
    t.close()


@pytest.mark.parametrize("once", [True, False], ids=["heartbeat-once", "full-body"])
def test_fuzz(once):
    """~1500 pod events over 200 uids in 6 batches with a tick between them; before every batch a third of the
    pods get one or two notes, and every noted version comes back in the batch with probability 3/4 - before,
    between and behind real changes of the same pod (a third of them right behind one), Deleted lines included (nothing follows a uid's Deleted
    line, as on a real watch: test_uid_ingest_gpu.py test_fuzz)"""
    t = EchoLock(once=once, seed=13)
    names = fleet(t, 16)
    rng = t.rng
    total = 0
    for r in range(6):
        notes = {}
        for k in rng.choice(200, 70, replace=False).tolist():
            notes[k] = [b"%d" % (10000 * (r + 1) + 10 * k + j) for j in range(int(rng.integers(1, 3)))]
        t.note([(b"u-f%d" % k, v) for k, vs in notes.items() for v in vs])
        lines, gone = [], set()
        for _ in range(int(rng.integers(220, 300))):
            k = int(rng.integers(0, 200))
            if k in gone:
                continue
            typ = ("ADDED", "MODIFIED", "MODIFIED", "DELETED")[int(rng.integers(0, 4))]
            rv = None
            if notes.get(k) and rng.integers(0, 4):
                rv = notes[k].pop(0).decode()
                typ = "MODIFIED" if typ == "ADDED" else typ
                if rng.integers(0, 3) == 0:  # a real change right before the echo: the match is consumed, the line kept
                    lines.append(("MODIFIED", t.doc("f%d" % k, names[k % 16], spec=k % 2)))
            if typ == "DELETED":
                gone.add(k)
            kw = dict(status_nonempty=True) if rng.integers(0, 2) else {}
            lines.append((typ, t.doc("f%d" % k, names[k % 16], spec=k % 2, rv=rv, **kw)))
        t.batch(lines, "fuzz batch %d" % r)
        total += len(lines)
        t.tick("fuzz tick %d" % r)
    s = t.a.echo_stats()
    assert total > 1200 and s["dropped"] > 100 and s["kept_matched"] > 20 and s["forgets"] > 10
    t.close()


def test_call_level_errors():
    e = Engine(make_config(**KW))
    codec = Codec(manage_all_nodes=True)
    t = EchoLock.__new__(EchoLock)
    stream = wf.wrap(EchoLock.ndoc(t, "n0", "5"), "ADDED")
    _f, _u, _n, sid = e.frame_watch(stream)
    for call in (lambda: e.ingest_nodes_framed_echo(codec, sid, [0]), lambda: e.ingest_pods_framed_echo(codec, sid, [0])):
        with pytest.raises(KwokError) as ei:  # the ledger is not enabled
            call()
        assert ei.value.code == abi.EINVAL
    e.echo_enable()
    with pytest.raises(KwokError) as ei:  # the pod entry needs the uid directory
        e.ingest_pods_framed_echo(codec, sid, [0])
    assert ei.value.code == abi.EINVAL
    e.uid_dir_enable()
    for bad in (0, sid + 1):
        for call in (lambda: e.ingest_nodes_framed_echo(codec, bad, [0]), lambda: e.ingest_pods_framed_echo(codec, bad, [0])):
            with pytest.raises(KwokError) as ei:
                call()
            assert ei.value.code == abi.EINVAL
    h, s, _nh, ne = e.ingest_nodes_framed_echo(codec, sid, [0, 5, 4000000000])
    assert list(s) == [0, abi.EINVAL, abi.EINVAL] and h[0] >= 0 and ne == 0
    assert e.ingest_nodes_framed_echo(codec, sid, [])[3] == 0 and e.ingest_pods_framed_echo(codec, sid, [])[5] == 0
    e.close()
