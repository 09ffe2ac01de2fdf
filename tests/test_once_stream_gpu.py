"""GPU: quiet ticks of an engine that writes every heartbeat body (single rank)
run k_once_stream: k_once's counting blocks (handle list, counters, per-bucket
summaries) beside the heartbeat streamers, full or delta, in one launch.  A tick
that has work after all is run again with k_tick, and a tick queued behind it
skips on the device, streamers included, and is enqueued again.

The pattern is test_hb_delta_gpu.py's: the engine under test (e), an engine
created under KWOK_ONCE_STREAM=0 and driven in lockstep (f: the same ticks
through k_tick) and the oracle.  Every tick compares every body, the handle
list, the patches, the deletes and the counters with the oracle
(gpu_common.compare_tick) and the whole heartbeat region [0, n x stride),
padding included, byte for byte with f's.  kwok_engine_stats must show the path
each case expects (ticks_once_stream, once_summary, once_redo, ticks_hb_delta):
a test that never takes the new path proves nothing.

Fleets are 64 buckets; the managed-node counts sit around the stream's 4-slot
group and the 8 waves of a 512-thread streamer block (1, 3, 5: fewer groups than
waves; 1027, 4100: many groups, a partial last one)."""
import ipaddress

import numpy as np
import pytest

from gpu_common import compare_tick, new_pods
from kwok_amd import abi, engine
from kwok_amd.engine import Engine, make_config
from oracle.oracle import Oracle
from test_hb_delta_gpu import blocking_clocks

pytestmark = pytest.mark.gpu

T0 = 1704067230  # 2024-01-01T00:00:30Z
DAY = 86400
KW = dict(cidr="10.0.0.1/16", node_ip="196.168.0.1", buckets=64, node_slots_per_bucket=160, pod_slots_per_bucket=64)
KW_PODS = dict(cidr="10.0.0.1/16", node_ip="196.168.0.1", buckets=64, node_slots_per_bucket=16, pod_slots_per_bucket=128)
SPECS = [([("fake-pod", "fake")], [], []),
         ([("a", "img-a"), ("b", "img/b:v2")], [("init", "busybox")], ["g.io/x"])]
# (managed nodes, KWOK_HB_NT, KWOK_TICK_STREAMERS, KWOK_TICK_STREAM_SHARE or None)
FLEETS = [(1, 1, 1, None), (3, 0, 3, None), (5, 1, 3, 512), (1027, 0, 1, 512), (1027, 1, 3, None), (4100, 1, 1, None),
          (4100, 0, 3, None)]
PATHS = ("ticks_once_stream", "once_summary", "once_redo", "ticks_hb_delta")


class Trio:
    """e (under test), f (KWOK_ONCE_STREAM=0) and the oracle o, fed the same events
    and ticked at the same clocks.  env: for both engines; e_env: for e alone"""

    def __init__(self, monkeypatch, env=None, e_env=None, oracle=True, **cfg):
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, str(v))
        kw = dict(KW, **cfg)
        monkeypatch.setenv("KWOK_ONCE_STREAM", "0")
        self.f = Engine(make_config(**kw))
        monkeypatch.delenv("KWOK_ONCE_STREAM")
        for k, v in (e_env or {}).items():
            monkeypatch.setenv(k, str(v))
        self.e = Engine(make_config(**kw))
        for k in (e_env or {}):
            monkeypatch.delenv(k)
        self.o = Oracle(make_config(**kw)) if oracle else None
        self.all = [x for x in (self.e, self.f, self.o) if x is not None]
        self.rng = np.random.default_rng(11)
        self.body = None  # (a custom template: the expected body of a clock, no oracle)

    def close(self):
        for x in self.all:
            x.close()

    def specs(self):
        ids = [[x.register_pod_spec(*s) for s in SPECS] for x in self.all]
        assert all(i == ids[0] for i in ids)
        return ids[0]

    def nodes(self, names, managed=1, lockable=1):
        ar = abi.Arena()
        ev = np.zeros(len(names), abi.NODE_EVENT_DTYPE)
        ev["op"] = abi.OP_UPSERT
        ev["managed"] = managed
        ev["lockable"] = lockable
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

    def paths(self):
        s = self.e.stats()
        return {k: s[k] for k in PATHS}

    def check(self, now, where):
        """the collected tick of e and f: everything against the oracle, and e's whole
        heartbeat region (padding included), handle list and counters against f's"""
        fs = self.f.stats()
        assert fs["ticks_once_stream"] == 0, "KWOK_ONCE_STREAM=0 ran k_once_stream"
        E, F = self.e.read_arrays(), self.f.read_arrays()
        n, st, ln = len(E["heartbeat_nodes"]), E["heartbeat_stride"], E["heartbeat_len"]
        assert n == len(F["heartbeat_nodes"]) and E["heartbeat_off"] == 0
        if self.o is not None:
            compare_tick(self.e, self.o, where)
            compare_tick(self.f, self.o, where + " (KWOK_ONCE_STREAM=0)")
        else:
            rows = E["arena"][:n * st].reshape(n, st)[:, :ln]
            assert (rows == np.frombuffer(self.body(now), np.uint8)[None, :]).all(), where + " heartbeat bodies"
        assert (E["heartbeat_nodes"] == F["heartbeat_nodes"]).all(), where + " heartbeat handles"
        assert E["counters"] == F["counters"], where + " counters"
        same = E["arena"][:n * st] == F["arena"][:n * st]
        assert same.all(), "%s: byte %d of the heartbeat region differs from the KWOK_ONCE_STREAM=0 engine's" % (
            where, int(np.argmin(same)))
        return E, n

    def tick(self, now, where, once, delta, summary=None, redo=False):
        """one blocking tick everywhere; what e's tick must have been: a k_once_stream
        tick (once), a delta tick, one that read the summaries, one that was redone"""
        p0 = self.paths()
        for x in self.all:
            x.tick(now, read=False)
        p1 = self.paths()
        got = {k: p1[k] - p0[k] for k in PATHS}
        want = dict(ticks_once_stream=int(once), ticks_hb_delta=int(delta), once_redo=int(redo),
                    once_summary=got["once_summary"] if summary is None else int(summary))
        assert got == want, "%s: path taken %r, expected %r" % (where, got, want)
        return self.check(now, where)

    def pair(self, now0, now1, where, want):
        """two ticks queued back to back on the engines; want: e's path counts over both"""
        p0 = self.paths()
        for x in (self.e, self.f):
            x.tick_submit(now0)
            x.tick_submit(now1)
        for q, now in enumerate((now0, now1)):
            for x in (self.e, self.f):
                x.tick_collect(read=False)
            if self.o is not None:
                self.o.tick(now, read=False)
            self.check(now, "%s (queued %d)" % (where, q))
        p1 = self.paths()
        got = {k: p1[k] - p0[k] for k in want}
        assert got == want, "%s: paths taken %r, expected %r" % (where, got, want)


def fleet_env(nt, streamers, share):
    env = {"KWOK_HB_NT": nt, "KWOK_TICK_STREAMERS": streamers}
    if share is not None:
        env["KWOK_TICK_STREAM_SHARE"] = share
    return env


@pytest.mark.parametrize("n,nt,streamers,share", FLEETS)
def test_blocking_ticks_one_slot(n, nt, streamers, share, monkeypatch):
    """the initial tick is k_tick; every later one is k_once_stream and a delta tick
    (the validity record of a k_once_stream tick is written: the next one is a delta);
    the first quiet tick builds the summaries, the later ones read them"""
    t = Trio(monkeypatch, fleet_env(nt, streamers, share))
    t.nodes(["node-%07d" % i for i in range(n)])
    for k, now in enumerate(blocking_clocks()):
        _, got = t.tick(now, "blocking tick %d (n=%d)" % (k, n), once=k > 0, delta=k > 0, summary=k > 1)
        assert got == n
    t.close()


@pytest.mark.parametrize("n,nt,streamers,share", FLEETS)
def test_queued_two_deep(n, nt, streamers, share, monkeypatch):
    """tick k+1 is submitted before tick k is collected: two slots, each one's previous
    clock two ticks back; ticks 1..9 are k_once_stream, 2..9 deltas"""
    t = Trio(monkeypatch, fleet_env(nt, streamers, share))
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
        p = t.paths()
        assert (p["ticks_once_stream"], p["ticks_hb_delta"], p["once_redo"]) == (k, max(0, k - 1), 0), "queued tick %d" % k
        _, got = t.check(now, "queued tick %d (n=%d)" % (k, n))
        assert got == n
    assert t.paths()["once_summary"] == 8
    t.close()


@pytest.mark.parametrize("n,nt", [(5, 1), (1027, 0)])
def test_custom_heartbeat_template(n, nt, monkeypatch):
    """heartbeat_a.tpl (79 units per slot): the custom-unit-count walk in the streamers,
    full and delta; bodies against the host template compiler's"""
    from test_template_cpu import tpl
    htext = tpl("heartbeat_a.tpl")
    t = Trio(monkeypatch, {"KWOK_HB_NT": nt}, oracle=False, node_heartbeat_template=htext)
    t.body = lambda now: engine.heartbeat_template_patch(htext, 1704067200, "196.168.0.1", now)
    t.nodes(["node-%07d" % i for i in range(n)])
    for k, now in enumerate((T0, T0 + 30, T0 + 3600, T0 + DAY)):
        E, got = t.tick(now, "custom heartbeat tick %d" % k, once=k > 0, delta=k > 0)
        assert got == n and E["heartbeat_len"] == len(t.body(now)) and E["heartbeat_stride"] // 16 == 79
    p = t.paths()
    assert p["ticks_once_stream"] == 3 and p["ticks_hb_delta"] == 3, p
    t.close()


def pod_fleet(t, managed_frac=1.0, lockable_frac=1.0, pods=2000, settled=True):
    rng = t.rng
    n = 300
    managed = (rng.random(n) < managed_frac).astype(np.uint8)
    lockable = (rng.random(n) < lockable_frac).astype(np.uint8)
    spec = t.specs()
    nh = t.nodes(["node-%04d" % i for i in range(n)], managed, lockable)
    ev, ar = new_pods(rng, nh, pods, spec)
    if settled:  # (no pod patched without an IP: nothing left for the second tick)
        ev["phase"] = abi.PHASE_PENDING
        ev["flags"] |= abi.POD_STATUS_NONEMPTY
    t.pods(ev, ar)
    return nh, spec, int(managed.sum())


def test_mixed_buckets(monkeypatch):
    """60% of the nodes managed, 5% not lockable, pods on all of them: n_hb is smaller
    than the node count, buckets disagree on the re-lock flag (the node-index path);
    counters and handle lists equal the oracle's (Trio.check)"""
    t = Trio(monkeypatch, **KW_PODS)
    _, _, n_managed = pod_fleet(t, 0.6, 0.95)
    _, got = t.tick(T0, "initial", once=False, delta=False)
    assert got == n_managed and got < 300
    for k in range(4):
        t.tick(T0 + 30 * (k + 1), "steady %d" % k, once=True, delta=True, summary=k > 0)
    t.pair(T0 + 150, T0 + 180, "steady", dict(ticks_once_stream=2, once_redo=0, once_summary=2))
    t.close()


def test_summaries_go_stale(monkeypatch):
    """quiet ticks (BUILD, then USE); an ingested pod batch gives a k_tick tick; the next
    quiet tick builds the summaries again and the one after it reads them"""
    t = Trio(monkeypatch, **KW_PODS)
    nh, spec, _ = pod_fleet(t)
    t.tick(T0, "initial", once=False, delta=False)
    t.tick(T0 + 30, "quiet (build)", once=True, delta=True, summary=False)
    t.tick(T0 + 60, "quiet (use)", once=True, delta=True, summary=True)
    ev, ar = new_pods(t.rng, nh, 100, spec)
    ev["phase"] = abi.PHASE_PENDING
    ev["flags"] |= abi.POD_STATUS_NONEMPTY
    t.pods(ev, ar)
    E, _ = t.tick(T0 + 90, "after the pod batch", once=False, delta=True, summary=False)
    assert len(E["pod_patch_pods"]) > 50
    t.tick(T0 + 120, "quiet again (build)", once=True, delta=True, summary=False)
    t.tick(T0 + 150, "quiet again (use)", once=True, delta=True, summary=True)
    t.close()


def test_patches_without_addresses_predict_work(monkeypatch):
    """pods created with an empty status are patched without IPs and take their Gets in
    the next tick, which follows no event: the host expects that (the tick before it
    patched pods that took no address) and runs k_tick, a delta tick, not k_once_stream
    and a redo with the whole stream"""
    t = Trio(monkeypatch, **KW_PODS)
    pod_fleet(t, settled=False)
    E, _ = t.tick(T0, "initial", once=False, delta=False)
    assert len(E["pod_patch_pods"]) > 0
    E, _ = t.tick(T0 + 30, "their Gets", once=False, delta=True, redo=False)
    assert len(E["pod_patch_pods"]) > 0
    t.tick(T0 + 60, "quiet", once=True, delta=True, summary=False)
    t.tick(T0 + 90, "quiet 2", once=True, delta=True, summary=True)
    t.close()


def cni_fleet(monkeypatch):
    """a CNI engine with pods waiting for their IPs, after quiet ticks; returns the trio
    and the next clock"""
    t = Trio(monkeypatch, **dict(KW_PODS, enable_cni=True))
    pod_fleet(t, settled=False)
    t.tick(T0, "initial", once=False, delta=False)
    for k in range(3):
        t.tick(T0 + 30 * (k + 1), "quiet %d" % k, once=True, delta=True)
    return t, T0 + 120


def cni_assign_half(t):
    pend = [x.cni_pending() for x in t.all]
    assert all((p == pend[0]).all() for p in pend) and len(pend[0]) >= 2
    take = pend[0][: len(pend[0]) // 2]
    ips = np.arange(int(ipaddress.IPv4Address("172.20.0.2")), int(ipaddress.IPv4Address("172.20.0.2")) + len(take),
                    dtype=np.uint32)
    got = [x.cni_assign(take, ips) for x in t.all]
    assert all((g == got[0]).all() for g in got)
    return len(take)


def test_redo_blocking(monkeypatch):
    """kwok_cni_assign between quiet ticks (no ingest): the counting blocks find the
    pods' patches, the tick is run again with k_tick (whole stream, no delta, no
    validity record), its outputs and region equal the oracle's and f's"""
    t, now = cni_fleet(monkeypatch)
    took = cni_assign_half(t)
    E, _ = t.tick(now + DAY, "after the assignment", once=False, delta=False, redo=True)
    assert took and len(E["pod_patch_pods"]) > 0
    # the redone tick recorded nothing: one whole stream, then deltas again
    t.tick(now + 2 * DAY, "quiet after", once=True, delta=False, summary=False)
    t.tick(now + 2 * DAY + 30, "quiet after 2", once=True, delta=True, summary=True)
    t.close()


def test_redo_queued_two_deep(monkeypatch):
    """the same with tick k+1 submitted before tick k is collected: k is redone, k+1
    skipped on the device (its streamers too) and is enqueued again.  Clocks a day
    apart: a region left as it was cannot pass.  Neither tick is a delta tick; the
    two after them write everything (no record), the next two are deltas again"""
    t, now = cni_fleet(monkeypatch)
    t.pair(now, now + 30, "quiet", dict(ticks_once_stream=2, once_redo=0))
    took = cni_assign_half(t)
    p0 = t.paths()
    for x in (t.e, t.f):
        x.tick_submit(now + DAY)
        x.tick_submit(now + 2 * DAY)
    for q, clock in enumerate((now + DAY, now + 2 * DAY)):
        for x in (t.e, t.f):
            x.tick_collect(read=False)
        t.o.tick(clock, read=False)
        E, _ = t.check(clock, "redo, queued %d" % q)
        assert took and (q or len(E["pod_patch_pods"]) > 0)
    p1 = t.paths()
    assert {k: p1[k] - p0[k] for k in PATHS} == dict(ticks_once_stream=1, once_summary=0, once_redo=1, ticks_hb_delta=0), (p0, p1)
    t.pair(now + 3 * DAY, now + 4 * DAY, "after the redo", dict(ticks_once_stream=2, ticks_hb_delta=0, once_redo=0))
    t.pair(now + 5 * DAY, now + 6 * DAY, "steady again", dict(ticks_once_stream=2, ticks_hb_delta=2, once_redo=0,
                                                              once_summary=2))
    t.close()


@pytest.mark.parametrize("e_env,cfg", [({}, dict(buckets=4, node_slots_per_bucket=2048, pod_slots_per_bucket=64)),
                                       ({"KWOK_ONCE": 0}, {})], ids=["node-slots-over-lds", "KWOK_ONCE=0"])
def test_fallbacks(e_env, cfg, monkeypatch):
    """a bucket with more node slots than k_once holds in LDS, and KWOK_ONCE=0: k_tick
    as before, the same results"""
    t = Trio(monkeypatch, e_env=e_env, **cfg)
    t.nodes(["node-%07d" % i for i in range(1027)])
    for k in range(4):
        _, got = t.tick(T0 + 30 * k, "fallback tick %d" % k, once=False, delta=k > 0, summary=False)
        assert got == 1027
    assert t.e.stats()["ticks_full"] == 4
    t.close()


def test_no_stream_diagnostic(monkeypatch):
    """KWOK_TICK_NO_STREAM=1 (bodies not written): the path is not taken"""
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
    for k in range(3):
        e.tick(T0 + 30 * k, read=False)
        o.tick(T0 + 30 * k, read=False)
        E, O = e.read_arrays(), o.read_arrays()
        assert E["counters"] == O["counters"] and (E["heartbeat_nodes"] == O["heartbeat_nodes"]).all()
    s = e.stats()
    assert s["ticks_once_stream"] == 0 and s["ticks_hb_delta"] == 0 and s["ticks_full"] == 3, s
    e.close()
    o.close()
