"""GPU: the drop-in controller with the engine's pod uid directory
(Controller(..., uid_directory=True): kwok_ingest_pods_framed_uid, kwok_uid_lookup,
kwok_uid_bind; include/kwok_watch.h) against the same controller
with its host uid map (uid_directory=False), each on its own fake clientset driven
with the same cluster events: the reference's node and pod controller tests, the
create / modify / delete scenario and the same-interval IP case through feed_watch
(lines cut at arbitrary byte positions), a relist with Replace with the echoes of
the controller's own patches among its items, and the scenario with typed on_event
steps and raw-byte steps mixed.  Every write, body for body, and the final
apiserver state must be identical; the directory run keeps no pod_by_uid."""
import json

import pytest

import test_controller_cpu as T
import test_resync_controller_gpu as R
import test_watch_controller_gpu as W
from fake_clientset import FakeClientset
from kwok_amd.controller import Config, Controller
from kwok_amd.engine import Engine

pytestmark = pytest.mark.gpu

BOTH = (True, False)


def feed_controller(cs, uid_directory, chunking="random", suppress=True, backend=None, geometry=T.SMALL, mixed=False, **kw):
    """W.feed_controller with the directory switch; gate[0] = False loses the watches (R.close_watch);
    mixed: the pod watch alternates, step by step, between typed events and raw bytes"""
    c = Controller(Config(client_set=cs, **kw), backend=Engine, suppress_echoes=suppress, geometry=geometry,
                   uid_directory=uid_directory)
    f = W.Feeder(c, chunking)
    gate = [True, f]
    typed = [False]
    step = c.step

    def stepped(now):
        f.flush()
        if mixed:  # (what arrived so far belongs to this step; the echoes it causes go the other way already)
            typed[0] = not typed[0]
        return step(now)
    c.step = stepped
    raw_pods = f.callback(False)

    def pods(typ, obj):
        if typed[0]:
            c.on_event(False, typ, json.loads(json.dumps(obj)))
        else:
            raw_pods(typ, obj)

    def gated(cb):
        return lambda typ, obj: gate[0] and cb(typ, obj)
    cs.watch("nodes", gated(f.callback(True)), label_selector=c.conf.manage_nodes_with_label_selector)
    cs.watch("pods", gated(pods), field_selector="spec.nodeName!=")
    c.gate = gate
    return c


def same_end(ca, cb, csa, csb, engines=True):
    assert csa.store == csb.store
    if engines:
        da, db = ca.eng.dump_pods(0, R.N_SLOTS), cb.eng.dump_pods(0, R.N_SLOTS)
        assert all((x == y).all() for x, y in zip(da, db))
    assert ca.pod_ref == cb.pod_ref and ca.pod_uid == cb.pod_uid and ca.node_handle == cb.node_handle
    assert ca.pod_by_uid == {} and len(cb.pod_by_uid) >= len(cb.pod_uid)
    assert (ca.stats.pod_records, ca.stats.pod_runs, ca.stats.rejected) == (cb.stats.pod_records, cb.stats.pod_runs,
                                                                           cb.stats.rejected)


@pytest.mark.parametrize("name", ["test_reference_node_controller", "test_reference_pod_controller"])
def test_reference_tests(name, monkeypatch):
    runs = []
    for uid in BOTH:
        made = []

        def factory(cs, _uid=uid, **kw):
            made.append((cs, feed_controller(cs, _uid, **kw)))
            return made[-1][1]
        monkeypatch.setattr(T, "controller", factory)
        getattr(T, name)()
        runs.append(made[0])
    (csa, ca), (csb, cb) = runs
    assert csa.calls == csb.calls and len(csa.calls) > 3
    assert ca.stats.watch_frames > 0 and ca.stats.watch_bad_frames == 0
    same_end(ca, cb, csa, csb, engines=False)  # (the reference tests close their controller)
    if name.endswith("pod_controller"):
        assert ca.stats.pod_records > 0 and ca.pod_uid


@pytest.mark.parametrize("mixed", [False, True], ids=["raw", "typed-and-raw"])
@pytest.mark.parametrize("deliver", ["sync", "queued"])
def test_scenario(deliver, mixed):
    """nodes and pods created, modified and deleted over 5 ticks (Added + Modified and Added + Deleted within
    one interval: several runs per batch); mixed: the pod watch is typed events in every other step, whose
    creates the typed path binds and whose known pods it resolves through the directory"""
    csa, csb = FakeClientset(deliver=deliver), FakeClientset(deliver=deliver)
    kw = dict(manage_nodes_with_annotation_selector=T.MANAGE, cidr="10.0.0.1/24", mixed=mixed)
    ca, cb = feed_controller(csa, True, **kw), feed_controller(csb, False, **kw)
    a, b = T.scenario(csa, ca), T.scenario(csb, cb)
    for t, (x, y) in enumerate(zip(a, b)):
        assert x == y, "tick %d" % t
    assert sum(len(x) for x in a) > 100 and ca.stats.pod_runs > 5
    assert ca.stats.echoes_at_flush == cb.stats.echoes_at_flush
    same_end(ca, cb, csa, csb)
    s = ca.eng.uid_stats()
    assert (s["cuts"] > 0 or mixed) and s["hits"] > 0
    assert (s["unbound"] > 0) == mixed  # (typed creates carry no uid; they are bound right after)
    ca.close()
    cb.close()


@pytest.mark.parametrize("deliver", ["sync", "queued"])
def test_same_interval_ip(deliver):
    csa, csb = FakeClientset(deliver=deliver), FakeClientset(deliver=deliver)
    kw = dict(manage_nodes_with_annotation_selector=T.MANAGE, node_ip="10.0.0.254", cidr="10.0.0.1/24")
    ca, cb = feed_controller(csa, True, **kw), feed_controller(csb, False, **kw)
    a, b = T.empty_status_scenario(csa, ca), T.empty_status_scenario(csb, cb)
    assert a == b and len(a[0]) == 5 and a[1] == a[2] == []
    assert ca.stats.reentered == cb.stats.reentered == 2  # (the re-entered pods go the typed way: lookup, bind)
    same_end(ca, cb, csa, csb)
    ca.close()
    cb.close()


@pytest.mark.parametrize("per_page", [2, 500])
def test_relist_with_replace(per_page):
    """R's relist: the watch closed over a gap of deletions and creations, then the full List pages with
    replace=True - on both controllers; the sweep removes the same pods, and later steps write the same"""
    csa, csb = FakeClientset(), FakeClientset()
    ca, cb = feed_controller(csa, True, **R.CONF), feed_controller(csb, False, **R.CONF)
    for cs in (csa, csb):
        R.populate(cs)
    for t in (1, 2):
        for c in (ca, cb):
            c.step(T.S0 + 30 * t)
    for c, cs in ((ca, csa), (cb, csb)):
        R.close_watch(c, c.gate)
        R.gap(cs)
        c.gate[0] = True
        R.feed_pages(c, cs, per_page, True)
    for t in (3, 4, 5):
        for c in (ca, cb):
            c.step(T.S0 + 30 * t)
        assert csa.calls == csb.calls, "step %d" % t
    assert ca.stats.resync_swept_pods == cb.stats.resync_swept_pods == R.N_GONE_PODS
    assert ca.stats.resync_swept_nodes == cb.stats.resync_swept_nodes == len(R.GONE_NODES)
    assert ca.stats.resync_skipped == cb.stats.resync_skipped == 0
    assert ca.eng.resync_stats() == cb.eng.resync_stats()
    same_end(ca, cb, csa, csb)
    ca.close()
    cb.close()


def test_relist_whose_items_are_echoes():
    """a step with the watch closed: the list items of the patched objects ARE the echoes of the controller's
    own patches; they are dropped before the ingest and marked by the handle kwok_uid_lookup gives"""
    res = []
    for uid in BOTH:
        cs = FakeClientset()
        c = feed_controller(cs, uid, **R.CONF)
        R.populate(cs)
        c.step(T.S0 + 30)
        R.close_watch(c, c.gate)
        c.step(T.S0 + 60)
        cs.delete("pods", ("default", "pod-0007"))
        c.gate[0] = True
        used = R.used_pods(c)
        R.feed_pages(c, cs, 500, True)
        c.step(T.S0 + 90)
        assert c.stats.resync_swept_pods == 1 and R.used_pods(c) == used - 1 and c.stats.resync_swept_nodes == 0
        res.append((cs.calls, cs.store, c.stats.echoes_at_flush, c.eng.resync_stats()))
        c.close()
    assert res[0] == res[1] and res[0][3]["marked"] > 0
