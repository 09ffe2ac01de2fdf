"""GPU: the drop-in controller with the engine's node uid directory
(Controller(..., uid_directory=True, echo_ledger=True, ref_directory=True, node_directory=True):
kwok_node_lookup, kwok_node_bind, the nodes' uids from kwok_refs_lookup; include/kwok_watch.h,
DESIGN.md §26) against the same controller with the first three directories and its
node_handle / node_uid maps, each on its own fake clientset driven with the same cluster
events, through the drivers of test_uid_controller_gpu.py.  Every write, body for body, the
final apiserver state, the engine's pod state and the echo ledger's counters must be
identical, and the new controller ends with no per-object map at all:
node_handle == node_uid == pod_ref == pod_uid == node_name == {}.

Not tested: the refusal on a multi-rank engine (no one-process fixture, as for the other
directories)."""
import functools

import pytest

import test_controller_cpu as T
import test_resync_controller_gpu as R
import test_uid_controller_gpu as U
from fake_clientset import FakeClientset
from kwok_amd.controller import Config, Controller
from kwok_amd.engine import Engine

pytestmark = pytest.mark.gpu

BOTH = (True, False)


def feed_controller(cs, node_dir, **kw):
    """U.feed_controller(uid_directory=True) with the ledger and the reference directory on and the node directory switch"""
    plain = U.Controller
    U.Controller = functools.partial(Controller, echo_ledger=True, ref_directory=True, node_directory=node_dir)
    try:
        return U.feed_controller(cs, True, **kw)
    finally:
        U.Controller = plain


def same_end(ca, cb, csa, csb, engines=True):
    assert csa.store == csb.store
    if engines:
        da, db = ca.eng.dump_pods(0, R.N_SLOTS), cb.eng.dump_pods(0, R.N_SLOTS)
        assert all((x == y).all() for x, y in zip(da, db))
        assert ca.eng.echo_stats() == cb.eng.echo_stats()
        assert cb.eng.node_dir_stats() == dict.fromkeys(cb.eng.node_dir_stats(), 0)
    assert ca.node_dir and not cb.node_dir and ca.refs and cb.refs
    # no per-object map is left; the three-directory controller still keeps the two node maps
    assert ca.node_handle == ca.node_uid == ca.pod_ref == ca.pod_uid == ca.node_name == {}
    assert ca.pod_by_uid == cb.pod_by_uid == cb.pod_ref == cb.pod_uid == cb.node_name == {}
    assert ca.stats == cb.stats and ca.stats.refs_missing == 0
    assert ca.echo.rv == {} and ca.echo_q == []


def test_the_directory_needs_the_other_three():
    for kw in (dict(), dict(uid_directory=True), dict(uid_directory=True, echo_ledger=True),
               dict(uid_directory=True, ref_directory=False, echo_ledger=True)):
        with pytest.raises(ValueError):
            Controller(Config(client_set=FakeClientset()), backend=Engine, geometry=T.SMALL, node_directory=True, **kw)


@pytest.mark.parametrize("name", ["test_reference_node_controller", "test_reference_pod_controller"])
def test_reference_tests(name, monkeypatch):
    runs = []
    for node_dir in BOTH:
        made = []

        def factory(cs, _nd=node_dir, **kw):
            made.append((cs, feed_controller(cs, _nd, **kw)))
            return made[-1][1]
        monkeypatch.setattr(T, "controller", factory)
        getattr(T, name)()
        runs.append(made[0])
    (csa, ca), (csb, cb) = runs
    assert csa.calls == csb.calls and len(csa.calls) > 3
    assert ca.stats.watch_frames > 0 and ca.stats.watch_bad_frames == 0
    same_end(ca, cb, csa, csb, engines=False)  # (the reference tests close their controller)
    if name.endswith("node_controller"):
        assert cb.node_handle and cb.node_uid  # (what the switch removes)


@pytest.mark.parametrize("mixed", [False, True], ids=["raw", "typed-and-raw"])
@pytest.mark.parametrize("deliver", ["sync", "queued"])
def test_scenario(deliver, mixed):
    """nodes and pods created, modified and deleted over 5 ticks; mixed: the pod watch is typed events in every
    other step"""
    csa, csb = FakeClientset(deliver=deliver), FakeClientset(deliver=deliver)
    kw = dict(manage_nodes_with_annotation_selector=T.MANAGE, cidr="10.0.0.1/24", mixed=mixed)
    ca, cb = feed_controller(csa, True, **kw), feed_controller(csb, False, **kw)
    a, b = T.scenario(csa, ca), T.scenario(csb, cb)
    for t, (x, y) in enumerate(zip(a, b)):
        assert x == y, "tick %d" % t
    assert sum(len(x) for x in a) > 100 and ca.stats.pod_runs > 5
    n0 = len(csa.calls)
    for c in (ca, cb):  # (test_echo_controller_gpu.py: one more step with the watches closed flushes what waits)
        c.gate[0] = False
        c.step(T.S0 + 30 * 6)
    assert csa.calls == csb.calls and len(csa.calls) > n0
    same_end(ca, cb, csa, csb)
    s = ca.eng.node_dir_stats()
    assert s["notes"] > 0 and s["lookups"] > 0 and s["hits"] > 0  # (creates from frames; the heartbeat echoes' handles)
    assert cb.node_handle and cb.node_uid
    # every node the three-directory controller knows answers the same handle and uid from the device
    names = sorted(cb.node_handle)
    assert list(ca.eng.node_lookup(names)) == [cb.node_handle[n] for n in names]
    hs = sorted(cb.node_uid)
    got = Engine.ref_items(*ca.eng.refs_lookup(0, hs))
    assert [g[3].decode() for g in got] == [cb.node_uid[h] for h in hs]
    ca.close()
    cb.close()


@pytest.mark.parametrize("deliver", ["sync", "queued"])
def test_same_interval_ip(deliver):
    csa, csb = FakeClientset(deliver=deliver), FakeClientset(deliver=deliver)
    kw = dict(manage_nodes_with_annotation_selector=T.MANAGE, node_ip="10.0.0.254", cidr="10.0.0.1/24")
    ca, cb = feed_controller(csa, True, **kw), feed_controller(csb, False, **kw)
    a, b = T.empty_status_scenario(csa, ca), T.empty_status_scenario(csb, cb)
    assert a == b and len(a[0]) == 5 and a[1] == a[2] == []
    assert ca.stats.reentered == cb.stats.reentered == 2
    same_end(ca, cb, csa, csb)
    ca.close()
    cb.close()


@pytest.mark.parametrize("per_page", [2, 500])
def test_relist_with_replace_sweeps_nodes(per_page):
    """R's relist: the swept nodes' uids come from the device (kwok_refs_lookup, KWOK_REFS_ANY_SLOT) and their
    forgets reach the ledger as the host map's do"""
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
    assert ca.stats.resync_swept_nodes == cb.stats.resync_swept_nodes == len(R.GONE_NODES)
    assert ca.stats.resync_swept_pods == cb.stats.resync_swept_pods == R.N_GONE_PODS
    assert ca.stats.resync_skipped == cb.stats.resync_skipped == 0
    assert ca.eng.resync_stats() == cb.eng.resync_stats()
    same_end(ca, cb, csa, csb)  # (kwok_echo_stats equal: the swept nodes' forgets)
    ca.close()
    cb.close()
