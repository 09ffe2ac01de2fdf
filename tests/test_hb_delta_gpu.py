"""GPU: the delta heartbeat stream.  A tick whose slot provably still holds the
bodies of the slot's previous tick (same arena, body count, stride, unit count
and template generation: engine_state.h, TickSlot::HbValid) rewrites only the
64-byte lines in which the two templates differ.  The risk is stale bytes, so
every case here compares EVERY heartbeat body of EVERY tick byte for byte with
the oracle (gpu_common.compare_tick), compares the whole heartbeat region -
the padding rows [len, stride) included - with an engine created under
KWOK_HB_DELTA=0 that is driven in lockstep, and asserts through the
ticks_hb_delta counter that the delta path was or was not taken where the case
says so (a test that never runs a delta tick proves nothing).

Fleets are small, with node counts around the 4-slot stream group's tail (1, 3,
5, 1027, 4100 managed nodes); half the engines run with KWOK_HB_NT=1 and half
with KWOK_HB_NT=0, sizes at which the automatic choice would be plain stores.
Some run with KWOK_TICK_STREAM_SHARE=512, so that the chain blocks write part of
the (delta) stream as they do on large fleets."""
import numpy as np
import pytest

from gpu_common import compare_tick, new_pods
from kwok_amd import abi, engine
from kwok_amd.engine import Engine, make_config
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

T0 = 1704067230  # 2024-01-01T00:00:30Z
KW = dict(cidr="10.0.0.1/16", node_ip="196.168.0.1", buckets=64, node_slots_per_bucket=160, pod_slots_per_bucket=64)
SPECS = [([("fake-pod", "fake")], [], []),
         ([("a", "img-a"), ("b", "img/b:v2")], [("init", "busybox")], ["g.io/x"])]
# (managed nodes, KWOK_HB_NT, KWOK_TICK_STREAM_SHARE or None)
FLEETS = [(1, 1, None), (3, 0, None), (5, 1, 512), (1027, 0, 512), (1027, 1, None), (4100, 1, 512), (4100, 0, None)]


class Trio:
    """the engine under test (e), an engine created with KWOK_HB_DELTA=0 (f) and
    the oracle (o), fed the same events and ticked at the same clocks"""

    def __init__(self, monkeypatch, nt, share=None, oracle=True, **cfg):
        monkeypatch.setenv("KWOK_HB_NT", str(nt))
        if share is not None:
            monkeypatch.setenv("KWOK_TICK_STREAM_SHARE", str(share))
        kw = dict(KW, **cfg)
        monkeypatch.setenv("KWOK_HB_DELTA", "0")
        self.f = Engine(make_config(**kw))
        monkeypatch.delenv("KWOK_HB_DELTA")
        self.e = Engine(make_config(**kw))
        self.o = Oracle(make_config(**KW)) if oracle else None
        self.all = [x for x in (self.e, self.f, self.o) if x is not None]
        self.rng = np.random.default_rng(11)
        self.body = None  # (a custom template: the expected body of a clock, no oracle)

    def close(self):
        for x in self.all:
            x.close()

    def specs(self, specs=SPECS):
        ids = [[x.register_pod_spec(*s) for s in specs] for x in self.all]
        assert all(i == ids[0] for i in ids)
        return ids[0]

    def nodes(self, names, op=abi.OP_UPSERT):
        ar = abi.Arena()
        ev = np.zeros(len(names), abi.NODE_EVENT_DTYPE)
        ev["op"] = op
        ev["managed"] = 1
        ev["lockable"] = 1
        for i, n in enumerate(names):
            ev[i]["name"] = ar.ref(n)
        got = [x.ingest_nodes_raw(ev, bytes(ar.buf)) for x in self.all]
        for h, s in got[1:]:
            assert (h == got[0][0]).all() and (s == got[0][1]).all()
        assert (got[0][1] == 0).all()
        return got[0][0]

    def pods(self, ev, arena=b""):
        got = [x.ingest_pods_raw(ev, arena) for x in self.all]
        for h, s, _ in got[1:]:
            assert (h == got[0][0]).all() and (s == got[0][1]).all()
        return got[0][0]

    def delta_ticks(self):
        assert self.f.stats()["ticks_hb_delta"] == 0, "KWOK_HB_DELTA=0 ran a delta tick"
        return self.e.stats()["ticks_hb_delta"]

    def check(self, now, where):
        """the collected tick of e and f: every body against the oracle, and e's
        whole heartbeat region (padding included) against f's"""
        E, F = self.e.read_arrays(), self.f.read_arrays()
        n, st, ln = len(E["heartbeat_nodes"]), E["heartbeat_stride"], E["heartbeat_len"]
        assert n == len(F["heartbeat_nodes"]) and E["heartbeat_off"] == 0
        if self.o is not None:
            compare_tick(self.e, self.o, where)
            compare_tick(self.f, self.o, where + " (KWOK_HB_DELTA=0)")
        else:
            rows = E["arena"][:n * st].reshape(n, st)[:, :ln]
            assert (rows == np.frombuffer(self.body(now), np.uint8)[None, :]).all(), where + " heartbeat bodies"
        same = E["arena"][:n * st] == F["arena"][:n * st]
        assert same.all(), "%s: byte %d of the heartbeat region differs from the KWOK_HB_DELTA=0 engine's" % (
            where, int(np.argmin(same)))
        return E, n, st, ln

    def tick(self, now, where, delta):
        """one blocking tick everywhere; delta: whether e's must have been a delta tick"""
        d0 = self.delta_ticks()
        for x in self.all:
            x.tick(now, read=False)
        assert self.delta_ticks() - d0 == (1 if delta else 0), "%s: delta path %s" % (
            where, "not taken" if delta else "taken")
        return self.check(now, where)


def blocking_clocks():
    """steps +30, +30, +1, +0, -30, +3600, +86400, a jump to the last seconds of the
    year and +30 across the year end (no step is a multiple of anything the kernel
    could assume): the first tick writes everything, every later one is a delta"""
    c = [T0]
    for step in (30, 30, 1, 0, -30, 3600, 86400):
        c.append(c[-1] + step)
    c.append(1735689585)  # 2024-12-31T23:59:45Z
    c.append(c[-1] + 30)  # 2025-01-01T00:00:15Z
    return c


def run_blocking(t, n):
    t.nodes(["node-%07d" % i for i in range(n)])
    for k, now in enumerate(blocking_clocks()):
        _, got, _, _ = t.tick(now, "blocking tick %d (n=%d)" % (k, n), delta=k > 0)
        assert got == n
    assert t.delta_ticks() == len(blocking_clocks()) - 1


def run_queued(t, n):
    """tick k+1 is submitted before tick k is collected: two slots, each one's
    previous clock two ticks back; ticks 0 and 1 write everything, 2..9 are deltas"""
    t.nodes(["node-%07d" % i for i in range(n)])
    clocks = [T0 + 30 * k for k in range(10)]
    for x in (t.e, t.f):
        x.tick_submit(clocks[0])
    for k, now in enumerate(clocks):
        for x in (t.e, t.f):
            if k + 1 < len(clocks):
                x.tick_submit(clocks[k + 1])
            x.tick_collect(read=False)
        t.o.tick(now, read=False)
        assert t.delta_ticks() == max(0, k - 1), "queued tick %d" % k
        _, got, _, _ = t.check(now, "queued tick %d (n=%d)" % (k, n))  # (slot k % 2's bodies)
        assert got == n


@pytest.mark.parametrize("n,nt,share", FLEETS)
def test_blocking_ticks_one_slot(n, nt, share, monkeypatch):
    t = Trio(monkeypatch, nt, share)
    run_blocking(t, n)
    t.close()


@pytest.mark.parametrize("n,nt,share", FLEETS)
def test_queued_two_deep(n, nt, share, monkeypatch):
    t = Trio(monkeypatch, nt, share)
    run_queued(t, n)
    t.close()


@pytest.mark.parametrize("n,nt", [(1027, 1), (4100, 0)])
def test_managed_set_changes(n, nt, monkeypatch):
    t = Trio(monkeypatch, nt)
    spec = t.specs()
    names = ["node-%07d" % i for i in range(n)]
    nh = t.nodes(names)
    now = T0
    t.tick(now, "initial", delta=False)
    t.tick(now + 30, "steady", delta=True)
    now += 60
    # the body count changes: both ticks write everything (their node inits land
    # past the region); the tick after them is a delta again
    t.nodes(names[-10:], op=abi.OP_DELETE)
    _, got, _, _ = t.tick(now, "10 nodes deleted", delta=False)
    assert got == n - 10
    t.nodes(["late-%05d" % i for i in range(20)])
    _, got, _, _ = t.tick(now + 30, "20 nodes added", delta=False)
    assert got == n + 10
    t.tick(now + 60, "unchanged set", delta=True)
    now += 90
    # shrink by 500, pod churn (the pod patches land where bodies used to be), grow
    # back by 500: the record says n + 10 - 500 bodies, so the regrown tick writes all
    t.nodes(names[:500], op=abi.OP_DELETE)
    ev, ar = new_pods(t.rng, nh[500:n - 10], 800, spec)
    t.pods(ev, ar)
    E, got, st, _ = t.tick(now, "shrunk by 500, pod churn", delta=False)
    assert got == n + 10 - 500 and len(E["pod_patch_pods"]) > 300
    assert int(E["pod_patch_off"].min()) < (n + 10) * st  # patches where bodies were
    ev, ar = new_pods(t.rng, nh[500:n - 10], 300, spec)
    t.pods(ev, ar)
    t.tick(now + 30, "more pod churn, same set", delta=True)
    t.nodes(names[:500])
    _, got, _, _ = t.tick(now + 60, "regrown by 500", delta=False)
    assert got == n + 10
    t.tick(now + 90, "after the regrowth", delta=True)
    t.close()


@pytest.mark.parametrize("n,nt", [(1027, 0), (4100, 1)])
def test_arena_growth_poisoned(n, nt, monkeypatch):
    """KWOK_DEBUG_POISON=1: a new arena reads 0xEE wherever no kernel has written.
    A larger pod spec raises the worst-case output size, so the next submit
    replaces the arena: that tick must write every byte of every body"""
    monkeypatch.setenv("KWOK_DEBUG_POISON", "1")
    t = Trio(monkeypatch, nt)
    spec = t.specs()
    nh = t.nodes(["node-%07d" % i for i in range(n)])
    ev, ar = new_pods(t.rng, nh, 500, spec)
    t.pods(ev, ar)
    t.tick(T0, "initial", delta=False)
    t.tick(T0 + 30, "steady", delta=True)
    big = ([("container-%02d" % i, "registry.example/some/long/image/name-%02d:v1.2.3" % i) for i in range(12)], [], [])
    t.specs([big])
    E, got, st, ln = t.tick(T0 + 60, "after the arena grew", delta=False)
    rows = E["arena"][:got * st].reshape(got, st)
    assert got == n and not (rows[:, :ln] == 0xEE).any(), "poison bytes in a heartbeat body"
    t.tick(T0 + 90, "steady again", delta=True)
    t.close()


@pytest.mark.parametrize("n,nt", [(5, 1), (1027, 0)])
def test_custom_heartbeat_template(n, nt, monkeypatch):
    """heartbeat_a.tpl (79 units per slot, not the default 67) goes through the same
    delta path.  The oracle renders no custom template: the bodies are compared
    with the host template compiler's (kwok_heartbeat_template_patch), as
    tests/test_custom_template_gpu.py does"""
    from test_template_cpu import tpl
    htext = tpl("heartbeat_a.tpl")
    t = Trio(monkeypatch, nt, oracle=False, node_heartbeat_template=htext)
    t.body = lambda now: engine.heartbeat_template_patch(htext, 1704067200, "196.168.0.1", now)
    t.nodes(["node-%07d" % i for i in range(n)])
    for k, now in enumerate((T0, T0 + 30, T0 + 3600)):
        _, got, st, ln = t.tick(now, "custom heartbeat tick %d" % k, delta=k > 0)
        assert got == n and ln == len(t.body(now)) and st // 16 != 67
    t.close()


@pytest.mark.parametrize("run", [run_blocking, run_queued])
def test_switch_off(run, monkeypatch):
    """KWOK_HB_DELTA=0: the same sequences, no delta tick, the same bodies (Trio's
    f engine, checked by every tick of the run against the default engine and the
    oracle); here the counter of the switched-off engine is looked at on its own"""
    t = Trio(monkeypatch, 0)
    run(t, 1027)
    assert t.f.stats()["ticks_hb_delta"] == 0 and t.f.stats()["ticks_full"] >= 10
    assert t.e.stats()["ticks_hb_delta"] >= 8
    t.close()


def test_heartbeat_once_engine(monkeypatch):
    """one body per tick (KWOK_CFG_HEARTBEAT_ONCE): never a delta tick"""
    e, o = Engine(make_config(heartbeat_once=True, **KW)), Oracle(make_config(**KW))
    ar = abi.Arena()
    ev = np.zeros(1027, abi.NODE_EVENT_DTYPE)
    ev["op"], ev["managed"], ev["lockable"] = abi.OP_UPSERT, 1, 1
    for i in range(len(ev)):
        ev[i]["name"] = ar.ref("node-%07d" % i)
    assert (e.ingest_nodes_raw(ev, bytes(ar.buf))[0] == o.ingest_nodes_raw(ev, bytes(ar.buf))[0]).all()
    for k in range(4):
        e.tick(T0 + 30 * k, read=False)
        o.tick(T0 + 30 * k, read=False)
        compare_tick(e, o, "heartbeat-once tick %d" % k, once=True)
    assert e.stats()["ticks_hb_delta"] == 0
    e.close()
    o.close()
