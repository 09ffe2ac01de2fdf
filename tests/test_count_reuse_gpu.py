"""GPU: count reuse.  A quiet tick of a single-rank engine that writes every body
runs k_once_stream: the heartbeat streamers beside the counting blocks.  The count
(handle list, totals) reads state words, never the clock, so a quiet tick that
follows a cleanly counted one with no state change in between launches the
streamers alone (k_hb_stream) and takes its header from the engine's clean-count
record and its handle list from the slot (engine_state.h: kwok_engine::CleanCount,
TickSlot::ListValid, state_gen).  A reused tick has no net that finds unexpected
work, so everything here is about WHEN the path is taken.

The engine rule, as the tests state it: tick k is reused iff it would be a
k_once_stream tick, is not a requeue, the clean-count record is of the engine's
current state generation, and its slot's list record is of that generation too.
Both records are written when a clean k_once_stream tick (counted or reused)
retires; every ingest, CNI assignment, pool Put, sweep and k_tick launch starts
a new generation.  So with blocking ticks (one slot) a tick is reused exactly
when it is a k_once_stream tick, the tick before it was a k_once_stream tick that
was not redone, and nothing changed state between the two: tick 0 is k_tick,
tick 1 counts (it builds the summaries), ticks 2.. are reused.  Queued two deep,
tick 1 and tick 2 are both enqueued before tick 1 retires, so each of the two
slots counts once and ticks 3.. are reused.

The pattern is test_once_stream_gpu.py's Trio: e (default), f (KWOK_COUNT_REUSE=0,
the parent's behaviour) and the oracle in lockstep.  After EVERY tick: the whole
heartbeat region, padding included, against f byte for byte and the bodies against
the oracle; the handle list; counters and local counters; the result's sizes; and
the ticks_count_reused delta against the rule above.  Reused ticks still count as
ticks_once_stream / ticks_full / ticks_hb_delta / once_summary, so e's and f's
other path counters must agree tick by tick."""
import ctypes as C
import ipaddress
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from gpu_common import compare_tick, mark_deleting, new_pods
from kwok_amd import abi
from kwok_amd.engine import Engine, make_config
from oracle.oracle import Oracle
from test_hb_delta_gpu import blocking_clocks
from test_once_stream_gpu import DAY, KW, KW_PODS, T0, Trio, cni_assign_half, pod_fleet

ROOT = Path(__file__).resolve().parent.parent
SAME = ("ticks_full", "ticks_once", "once_redo", "once_summary", "ticks_hb_delta", "ticks_once_stream")
SIZES = ("n_heartbeat", "heartbeat_len", "heartbeat_stride", "n_node_init", "n_pod_patch", "n_delete", "arena_bytes")
gpu = pytest.mark.gpu
NODES = [1, 3, 4, 5, 1027]  # around the stream's 4-slot group; 1027: more than one streamer share


def test_stat_list_matches_header():
    """abi.ENGINE_STATS is the header's KWOK_STAT_* list, in order, and the new stat is last"""
    text = (ROOT / "include" / "kwok_engine.h").read_text()
    body = text[text.index("enum { KWOK_STAT_TICKS_FULL"):]
    body = re.sub(r"/\*.*?\*/", "", body[:body.index("KWOK_STAT_COUNT")], flags=re.S)
    names = re.findall(r"KWOK_STAT_(\w+)", body)
    assert [n.lower() for n in names] == list(abi.ENGINE_STATS)
    assert abi.ENGINE_STATS[-1] == "ticks_count_reused" and Engine.STATS == abi.ENGINE_STATS


class Reuse(Trio):
    """e (under test), f (KWOK_COUNT_REUSE=0) and the oracle; env: for both engines"""

    def __init__(self, monkeypatch, env=None, oracle=True, **cfg):
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, str(v))
        kw = dict(KW, **cfg)
        monkeypatch.setenv("KWOK_COUNT_REUSE", "0")
        self.f = Engine(make_config(**kw))
        monkeypatch.delenv("KWOK_COUNT_REUSE")
        self.e = Engine(make_config(**kw))
        self.o = Oracle(make_config(**kw)) if oracle else None
        self.all = [x for x in (self.e, self.f, self.o) if x is not None]
        self.rng = np.random.default_rng(11)
        self.body = None
        self.prev_clean = False  # blocking ticks: the previous tick was a clean k_once_stream tick, no change since
        self.seq = []            # per blocking tick: "tick" (k_tick) / "count" / "reuse" / "redo"

    def changed(self):
        """the test changed state on every engine: the next tick cannot be reused"""
        self.prev_clean = False

    def check(self, now, where):
        fs = self.f.stats()
        assert fs["ticks_count_reused"] == 0, "KWOK_COUNT_REUSE=0 reused a count"
        E, F = self.e.read_arrays(), self.f.read_arrays()
        n, st, ln = len(E["heartbeat_nodes"]), E["heartbeat_stride"], E["heartbeat_len"]
        assert n == len(F["heartbeat_nodes"]) and E["heartbeat_off"] == 0
        if self.o is not None:
            compare_tick(self.e, self.o, where)
            compare_tick(self.f, self.o, where + " (KWOK_COUNT_REUSE=0)")
            assert list(self.e.last.local_counters) == list(self.o.last.local_counters), where + " local counters"
        else:
            rows = E["arena"][:n * st].reshape(n, st)[:, :ln]
            assert (rows == np.frombuffer(self.body(now), np.uint8)[None, :]).all(), where + " heartbeat bodies"
        assert (E["heartbeat_nodes"] == F["heartbeat_nodes"]).all(), where + " heartbeat handles"
        assert E["counters"] == F["counters"], where + " counters"
        assert list(self.e.last.local_counters) == list(self.f.last.local_counters), where + " local counters"
        for k in SIZES:
            assert getattr(self.e.last, k) == getattr(self.f.last, k), "%s: %s" % (where, k)
        same = E["arena"][:n * st] == F["arena"][:n * st]
        assert same.all(), "%s: byte %d of the heartbeat region differs from the KWOK_COUNT_REUSE=0 engine's" % (
            where, int(np.argmin(same)))
        return E, n

    def tick(self, now, where, want=None):
        """one blocking tick everywhere; the reused delta against the one-slot rule, e's other
        path counters against f's; want: what the tick must have been (see seq), if the case says"""
        e0, f0 = self.e.stats(), self.f.stats()
        for x in self.all:
            x.tick(now, read=False)
        e1, f1 = self.e.stats(), self.f.stats()
        d = {k: e1[k] - e0[k] for k in e1}
        assert {k: d[k] for k in SAME} == {k: f1[k] - f0[k] for k in SAME}, where + ": paths differ from KWOK_COUNT_REUSE=0"
        once = d["ticks_once_stream"] == 1 and d["once_redo"] == 0
        expect = int(once and self.prev_clean)
        assert d["ticks_count_reused"] == expect, "%s: reused %d, the rule says %d (after %r)" % (
            where, d["ticks_count_reused"], expect, self.seq[-3:])
        self.prev_clean = once
        self.seq.append("redo" if d["once_redo"] else "reuse" if expect else "count" if once else "tick")
        if want is not None:
            assert self.seq[-1] == want, "%s: a %s tick, expected %s" % (where, self.seq[-1], want)
        return self.check(now, where)

    def settle(self, now, where):
        """ticks until reuse resumes: it must, within 4 ticks, right after one clean count (one slot),
        and the first tick after the change is never reused; two more reused ticks follow"""
        n0 = len(self.seq)
        for k in range(4):
            self.tick(now + 30 * k, "%s, tick %d after" % (where, k))
            if self.seq[-1] == "reuse":
                break
        got = self.seq[n0:]
        assert got[0] != "reuse" and got[-1] == "reuse" and got[-2] == "count" and got.count("reuse") == 1, (where, got)
        for k in range(2):
            self.tick(now + 30 * (len(got) + k), "%s, steady %d" % (where, k), want="reuse")
        return got


def steady(t, now, where, n=2):
    for k in range(n):
        t.tick(now + 30 * k, "%s, reused %d" % (where, k), want="reuse")


@gpu
@pytest.mark.parametrize("n", NODES)
def test_blocking_sequence(n, monkeypatch):
    """one slot: k_tick, one counting tick (BUILD), then every tick reused - 8 of them, over
    clock steps +30, +1, +0 (the same clock twice: nothing written), -30 (backwards), +3600,
    +86400 (a day), a jump to the year's end and +30 across it"""
    t = Reuse(monkeypatch)
    h = t.nodes(["node-%07d" % i for i in range(n)])
    spec = t.specs()
    ev, ar = new_pods(t.rng, h, 10 * n, spec)
    ev["phase"] = abi.PHASE_PENDING
    ev["flags"] |= abi.POD_STATUS_NONEMPTY
    t.pods(ev, ar)
    clocks = blocking_clocks()
    for k, now in enumerate(clocks):
        _, got = t.tick(now, "blocking tick %d (n=%d)" % (k, n))
        assert got == n
    assert t.seq == ["tick", "count"] + ["reuse"] * (len(clocks) - 2), t.seq
    s = t.e.stats()
    assert s["ticks_count_reused"] == len(clocks) - 2 >= 3 and s["ticks_hb_delta"] == len(clocks) - 1
    assert s["ticks_once_stream"] == len(clocks) - 1 and s["once_summary"] == len(clocks) - 2 and s["once_redo"] == 0
    t.close()


@gpu
@pytest.mark.parametrize("n", NODES)
def test_queued_two_deep(n, monkeypatch):
    """tick k+1 is submitted before tick k is collected: tick 0 is k_tick, ticks 1 and 2 count
    (one per slot: tick 2 is enqueued before tick 1 retires), ticks 3..9 are reused; the handle
    list of both slots is read (every tick's, alternating slots)"""
    t = Reuse(monkeypatch)
    h = t.nodes(["node-%07d" % i for i in range(n)])
    ev, ar = new_pods(t.rng, h, 10 * n, t.specs())
    ev["phase"] = abi.PHASE_PENDING
    ev["flags"] |= abi.POD_STATUS_NONEMPTY
    t.pods(ev, ar)
    clocks = [T0 + 30 * k for k in range(10)]
    for x in (t.e, t.f):
        x.tick_submit(clocks[0])
    for k, now in enumerate(clocks):
        for x in (t.e, t.f):
            if k + 1 < len(clocks):
                x.tick_submit(clocks[k + 1])
            x.tick_collect(read=False)
        t.o.tick(now, read=False)
        s = t.e.stats()
        assert (s["ticks_count_reused"], s["ticks_once_stream"], s["once_redo"]) == (max(0, k - 2), k, 0), "queued tick %d" % k
        _, got = t.check(now, "queued tick %d (n=%d)" % (k, n))
        assert got == n
    s, fs = t.e.stats(), t.f.stats()
    assert s["ticks_count_reused"] == 7 and {k: s[k] for k in SAME} == {k: fs[k] for k in SAME}
    t.close()


@gpu
def test_custom_template(monkeypatch):
    """heartbeat_a.tpl (79 units per slot) at n = 5: the custom-unit-count walk in k_hb_stream"""
    from kwok_amd import engine
    from test_template_cpu import tpl
    htext = tpl("heartbeat_a.tpl")
    t = Reuse(monkeypatch, oracle=False, node_heartbeat_template=htext)
    t.body = lambda now: engine.heartbeat_template_patch(htext, 1704067200, "196.168.0.1", now)
    t.nodes(["node-%07d" % i for i in range(5)])
    for k, now in enumerate((T0, T0 + 30, T0 + 60, T0 + 60, T0 + 3600, T0 + DAY, T0)):
        E, got = t.tick(now, "custom heartbeat tick %d" % k)
        assert got == 5 and E["heartbeat_len"] == len(t.body(now)) and E["heartbeat_stride"] // 16 == 79
    assert t.seq == ["tick", "count"] + ["reuse"] * 5, t.seq
    t.close()


def settled_fleet(monkeypatch, **cfg):
    """300 nodes, 2000 settled pods, ticked until two reused ticks have run; returns the trio,
    what pod_fleet returns, the creating events' bookkeeping (for mark_deleting) and the next clock"""
    t = Reuse(monkeypatch, **dict(KW_PODS, **cfg))
    nh, spec, _ = pod_fleet(t)
    for k in range(4):
        t.tick(T0 + 30 * k, "fleet tick %d" % k)
    assert t.seq == ["tick", "count", "reuse", "reuse"], t.seq
    return t, nh, spec, T0 + 120


def node_events(t, names, op):
    ar = abi.Arena()
    ev = np.zeros(len(names), abi.NODE_EVENT_DTYPE)
    ev["op"], ev["managed"], ev["lockable"] = op, 1, 1
    for i, n in enumerate(names):
        ev[i]["name"] = ar.ref(n)
    got = [x.ingest_nodes_raw(ev, bytes(ar.buf)) for x in t.all]
    for h, s in got[1:]:
        assert (h == got[0][0]).all() and (s == got[0][1]).all()
    assert (got[0][1] == 0).all()
    t.changed()
    return got[0][0]


@gpu
def test_pod_create_between_reused_ticks(monkeypatch):
    t, nh, spec, now = settled_fleet(monkeypatch)
    ev, ar = new_pods(t.rng, nh, 1, spec)
    ev["phase"] = abi.PHASE_PENDING
    ev["flags"] |= abi.POD_STATUS_NONEMPTY
    t.pods(ev, ar)
    t.changed()
    got = t.settle(now, "one pod create")
    assert got[0] == "tick", got  # (events since the last tick: k_tick)
    t.close()


@gpu
def test_pod_delete_mark_between_reused_ticks(monkeypatch):
    t, nh, spec, now = settled_fleet(monkeypatch)
    n_slots = KW_PODS["buckets"] * KW_PODS["pod_slots_per_bucket"]
    used, phase, hip, pip = t.o.dump_pods(0, n_slots)
    idx = np.nonzero(used)[0]
    d = SimpleNamespace(live=lambda: (idx, phase[idx], hip[idx], pip[idx]),
                        spec_of=np.full(n_slots, spec[0], np.int32), ctime_of=np.full(n_slots, 1704067000, np.int64))
    ev, ar = mark_deleting(t.rng, d, idx[:1].astype(np.int32))
    t.pods(ev, ar)
    t.changed()
    E, _ = t.tick(now, "the delete", want="tick")
    assert len(E["delete_pods"]) == 1
    t.changed()  # (the tick changed state itself: a delete, the zombie sweep)
    t.settle(now + 30, "one pod delete mark")
    t.close()


@gpu
def test_node_add_between_reused_ticks(monkeypatch):
    """n_hb changes: the whole stream and a count"""
    t, nh, spec, now = settled_fleet(monkeypatch)
    node_events(t, ["extra-node-0"], abi.OP_UPSERT)
    d0 = t.e.stats()["ticks_hb_delta"]
    E, n = t.tick(now, "after the node add")
    assert n == 301 and t.seq[-1] != "reuse" and t.e.stats()["ticks_hb_delta"] == d0
    t.settle(now + 30, "one node add")
    t.close()


@gpu
def test_node_delete_between_reused_ticks(monkeypatch):
    t, nh, spec, now = settled_fleet(monkeypatch)
    node_events(t, ["extra-node-0"], abi.OP_UPSERT)  # (a node without pods)
    got = t.settle(now, "node add")
    now += 30 * (len(got) + 2)
    node_events(t, ["extra-node-0"], abi.OP_DELETE)
    E, n = t.tick(now, "after the node delete")
    assert n == 300 and t.seq[-1] != "reuse"
    t.settle(now + 30, "one node delete")
    t.close()


@gpu
def test_pool_put_between_reused_ticks(monkeypatch):
    t, nh, spec, now = settled_fleet(monkeypatch)
    for x in t.all:
        x.pool_put([int(ipaddress.IPv4Address("10.0.200.200"))])
    t.changed()
    t.settle(now, "kwok_pool_put")
    t.close()


@gpu
def test_cni_assign_between_reused_ticks(monkeypatch):
    """a CNI engine with pods waiting for their IPs: the assignment starts a new generation, the
    counting tick after it finds the pods' patches and is redone with k_tick"""
    t = Reuse(monkeypatch, **dict(KW_PODS, enable_cni=True))
    pod_fleet(t, settled=False)
    for k in range(4):
        t.tick(T0 + 30 * k, "cni fleet tick %d" % k)
    assert t.seq[-2:] == ["reuse", "reuse"], t.seq
    took = cni_assign_half(t)
    t.changed()
    E, _ = t.tick(T0 + DAY, "after the assignment", want="redo")
    assert took and len(E["pod_patch_pods"]) > 0
    t.changed()  # (k_tick ran: pod states changed)
    t.settle(T0 + 2 * DAY, "a CNI assign")
    t.close()


@gpu
def test_resync_sweep_between_reused_ticks(monkeypatch):
    """a relist that holds every pod but one: the sweep removes it through the ingest path"""
    t, nh, spec, now = settled_fleet(monkeypatch)
    n_slots = KW_PODS["buckets"] * KW_PODS["pod_slots_per_bucket"]
    live = np.nonzero(t.o.dump_pods(0, n_slots)[0])[0].astype(np.int32)
    swept = []
    for x in (t.e, t.f):
        x.resync_begin(abi.KIND_PODS)
        assert x.resync_mark(abi.KIND_PODS, live[1:]) == 0
        hs, rel, _nd = x.resync_sweep(abi.KIND_PODS)
        swept.append((list(hs), list(rel)))
    assert swept[0] == swept[1] and swept[0][0] == [int(live[0])]
    ar = abi.Arena()
    ev = np.zeros(1, abi.POD_EVENT_DTYPE)
    ev["op"], ev["handle"] = abi.OP_DELETE, live[0]
    if swept[0][1][0]:
        ev[0]["pod_ip"] = ar.ref(abi.ip4s(int(swept[0][1][0])))
    assert not t.o.ingest_pods_raw(ev, bytes(ar.buf))[1].any()
    t.changed()
    t.settle(now, "a resync sweep")
    t.close()


@gpu
def test_followup_tick_is_not_reused(monkeypatch):
    """test_once_stream_gpu's follow-up case: pods created with an empty status are patched
    without IPs and take their Gets in the next tick, which follows no event - that tick runs
    k_tick and is never reused, nor is the one after it (a count)"""
    t = Reuse(monkeypatch, **KW_PODS)
    nh, _, _ = pod_fleet(t, settled=False)
    E, _ = t.tick(T0, "initial", want="tick")
    assert len(E["pod_patch_pods"]) > 0
    E, _ = t.tick(T0 + 30, "their Gets", want="tick")
    assert len(E["pod_patch_pods"]) > 0
    t.tick(T0 + 60, "quiet", want="count")
    steady(t, T0 + 90, "after the follow-up", 3)
    # the same between two reused ticks
    ev, ar = new_pods(t.rng, nh[:4], 8, [0])
    ev["phase"], ev["flags"] = abi.PHASE_NONE, 0
    t.pods(ev, ar)
    t.changed()
    E, _ = t.tick(T0 + 300, "empty-status creates", want="tick")
    assert len(E["pod_patch_pods"]) == 8
    t.changed()
    E, _ = t.tick(T0 + 330, "the tick after their patches", want="tick")
    assert len(E["pod_patch_pods"]) == 8
    t.changed()
    t.tick(T0 + 360, "quiet again", want="count")
    steady(t, T0 + 390, "steady again")
    t.close()


@gpu
@pytest.mark.parametrize("env,reuse", [({"KWOK_ONCE_STREAM": 0}, False), ({"KWOK_ONCE": 0}, False),
                                       ({"KWOK_HB_DELTA": 0}, True)], ids=lambda v: "-".join(v) if isinstance(v, dict) else "")
def test_switches(env, reuse, monkeypatch):
    """KWOK_ONCE_STREAM=0 and KWOK_ONCE=0: the parent's behaviour, nothing reused.  KWOK_HB_DELTA=0:
    reused ticks, each writing the whole stream"""
    t = Reuse(monkeypatch, env=env)
    t.nodes(["node-%07d" % i for i in range(1027)])
    for k, now in enumerate((T0, T0 + 30, T0 + DAY, T0 + DAY, T0 + 60)):
        t.tick(now, "%r tick %d" % (env, k))
    s = t.e.stats()
    assert s["ticks_count_reused"] == (3 if reuse else 0) and s["ticks_hb_delta"] == (0 if reuse else 4), s
    t.close()


@gpu
def test_no_stream_diagnostic(monkeypatch):
    """KWOK_TICK_NO_STREAM=1 (bodies not written): k_tick as before, nothing reused"""
    monkeypatch.setenv("KWOK_TICK_NO_STREAM", "1")
    e = Engine(make_config(**KW))
    monkeypatch.delenv("KWOK_TICK_NO_STREAM")
    o = Oracle(make_config(**KW))
    ar = abi.Arena()
    ev = np.zeros(1027, abi.NODE_EVENT_DTYPE)
    ev["op"], ev["managed"], ev["lockable"] = abi.OP_UPSERT, 1, 1
    for i in range(len(ev)):
        ev[i]["name"] = ar.ref("node-%07d" % i)
    assert (e.ingest_nodes_raw(ev, bytes(ar.buf))[0] == o.ingest_nodes_raw(ev, bytes(ar.buf))[0]).all()
    for k in range(5):
        e.tick(T0 + 30 * k, read=False)
        o.tick(T0 + 30 * k, read=False)
        E, O = e.read_arrays(), o.read_arrays()
        assert E["counters"] == O["counters"] and (E["heartbeat_nodes"] == O["heartbeat_nodes"]).all()
    s = e.stats()
    assert s["ticks_count_reused"] == 0 and s["ticks_once_stream"] == 0 and s["ticks_full"] == 5, s
    e.close()
    o.close()


def _host_gather(user, send, nbytes, recv):  # one rank: the gathered array is its own message
    C.memmove(recv, send, nbytes)
    return 0


@gpu
@pytest.mark.parametrize("kind", ["heartbeat-once", "KWOK_FORCE_MULTI"])
def test_other_engines_never_reuse(kind, monkeypatch):
    """a heartbeat-once engine (k_once, untouched) and a multi-rank engine: quiet ticks, none reused"""
    once = kind == "heartbeat-once"
    if not once:
        monkeypatch.setenv("KWOK_FORCE_MULTI", "1")
    e = Engine(make_config(heartbeat_once=once, allgather=None if once else _host_gather, **KW))
    o = Oracle(make_config(**KW))
    ar = abi.Arena()
    ev = np.zeros(1027, abi.NODE_EVENT_DTYPE)
    ev["op"], ev["managed"], ev["lockable"] = abi.OP_UPSERT, 1, 1
    for i in range(len(ev)):
        ev[i]["name"] = ar.ref("node-%07d" % i)
    assert (e.ingest_nodes_raw(ev, bytes(ar.buf))[0] == o.ingest_nodes_raw(ev, bytes(ar.buf))[0]).all()
    for k in range(6):
        e.tick(T0 + 30 * k, read=False)
        o.tick(T0 + 30 * k, read=False)
        if once:
            compare_tick(e, o, "%s tick %d" % (kind, k), once=True)
        else:
            E, O = e.read_arrays(), o.read_arrays()
            assert E["counters"] == O["counters"] and (E["heartbeat_nodes"] == O["heartbeat_nodes"]).all()
    s = e.stats()
    assert s["ticks_count_reused"] == 0 and s["ticks_once_stream"] == 0, s
    assert (s["ticks_once"] >= 3) == once, s
    e.close()
    o.close()
