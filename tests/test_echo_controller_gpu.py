"""GPU: the drop-in controller with the engine's echo ledger
(Controller(..., uid_directory=True, echo_ledger=True): kwok_ingest_pods_framed_echo,
kwok_ingest_nodes_framed_echo, kwok_echo_match, kwok_echo_update; include/kwok_watch.h,
DESIGN.md §24) against the same controller with its host Echoes (uid_directory=True),
each on its own fake clientset driven with the same cluster events, through the drivers
of test_uid_controller_gpu.py.  Every write, body for body, the final apiserver state and
the engine's pod state must be identical; the echoes dropped are as many (the ledger
controller decides all of them at flush), its host Echoes stays empty and the device
counted every drop."""
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


def feed_controller(cs, ledger, **kw):
    """U.feed_controller(uid_directory=True) with the ledger switch"""
    plain = U.Controller
    U.Controller = functools.partial(Controller, echo_ledger=ledger)
    try:
        return U.feed_controller(cs, True, **kw)
    finally:
        U.Controller = plain


def echoes(c):
    return c.stats.echoes_on_arrival + c.stats.echoes_at_flush


def ledger_side(c):
    """what only the ledger controller shows: no decision on arrival, an empty host Echoes, every drop counted
    by the device, no note refused"""
    assert c.ledger and c.echo.rv == {} and c.echo_q == []
    assert c.stats.echoes_on_arrival == 0 and c.stats.echo_notes_refused == 0
    s = c.eng.echo_stats()
    assert s["dropped"] == c.stats.echoes_at_flush
    return s


def same_end(ca, cb, csa, csb, engines=True):
    assert csa.store == csb.store
    if engines:
        da, db = ca.eng.dump_pods(0, R.N_SLOTS), cb.eng.dump_pods(0, R.N_SLOTS)
        assert all((x == y).all() for x, y in zip(da, db))
    assert ca.pod_ref == cb.pod_ref and ca.pod_uid == cb.pod_uid and ca.node_handle == cb.node_handle
    assert ca.node_name == cb.node_name and ca.node_uid == cb.node_uid
    assert ca.pod_by_uid == cb.pod_by_uid == {}
    assert echoes(ca) == echoes(cb)
    sa, sb = ca.stats, cb.stats
    assert (sa.pod_records, sa.pod_runs, sa.node_records, sa.rejected, sa.watch_frames, sa.watch_bad_frames, sa.watch_skipped,
            sa.reentered, sa.bodies) == (sb.pod_records, sb.pod_runs, sb.node_records, sb.rejected, sb.watch_frames,
                                         sb.watch_bad_frames, sb.watch_skipped, sb.reentered, sb.bodies)


@pytest.mark.parametrize("name", ["test_reference_node_controller", "test_reference_pod_controller"])
def test_reference_tests(name, monkeypatch):
    runs = []
    for ledger in BOTH:
        made = []

        def factory(cs, _ledger=ledger, **kw):
            made.append((cs, feed_controller(cs, _ledger, **kw)))
            return made[-1][1]
        monkeypatch.setattr(T, "controller", factory)
        getattr(T, name)()
        runs.append(made[0])
    (csa, ca), (csb, cb) = runs
    assert csa.calls == csb.calls and len(csa.calls) > 3
    assert ca.stats.watch_frames > 0 and ca.stats.watch_bad_frames == 0
    assert ca.ledger and not cb.ledger and ca.echo.rv == {} and ca.stats.echoes_on_arrival == 0
    same_end(ca, cb, csa, csb, engines=False)  # (the reference tests close their controller)


@pytest.mark.parametrize("mixed", [False, True], ids=["raw", "typed-and-raw"])
@pytest.mark.parametrize("deliver", ["sync", "queued"])
def test_scenario(deliver, mixed):
    csa, csb = FakeClientset(deliver=deliver), FakeClientset(deliver=deliver)
    kw = dict(manage_nodes_with_annotation_selector=T.MANAGE, cidr="10.0.0.1/24", mixed=mixed)
    ca, cb = feed_controller(csa, True, **kw), feed_controller(csb, False, **kw)
    a, b = T.scenario(csa, ca), T.scenario(csb, cb)
    for t, (x, y) in enumerate(zip(a, b)):
        assert x == y, "tick %d" % t
    assert sum(len(x) for x in a) > 100 and ca.stats.pod_runs > 5
    # deliver=queued hands the last tick's echoes over after the last step: the host controller dropped the typed
    # ones on arrival, the ledger controller decides them at its next flush.  One more step with the watches
    # closed (its own echoes reach neither side) flushes what waits; the counts are compared after it
    n0 = len(csa.calls)
    for c in (ca, cb):
        c.gate[0] = False
        c.step(T.S0 + 30 * 6)
    assert csa.calls == csb.calls and len(csa.calls) > n0
    same_end(ca, cb, csa, csb)
    s = ledger_side(ca)
    assert s["dropped"] > 20 and s["notes"] >= s["matched"]
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
    ledger_side(ca)
    ca.close()
    cb.close()


@pytest.mark.parametrize("per_page", [2, 500])
def test_relist_with_replace(per_page):
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
    ledger_side(ca)
    ca.close()
    cb.close()


def test_relist_whose_items_are_echoes():
    """a step with the watch closed: the list items of the patched objects ARE the echoes of the controller's
    own patches; the device drops them and the controller marks the handles it answered"""
    res = []
    for ledger in BOTH:
        cs = FakeClientset()
        c = feed_controller(cs, ledger, **R.CONF)
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
        if ledger:
            ledger_side(c)
        res.append((cs.calls, cs.store, echoes(c), c.eng.resync_stats()))
        c.close()
    assert res[0] == res[1] and res[0][3]["marked"] > 0 and res[0][2] > 0


def test_the_ledger_needs_the_engine_and_the_directory():
    with pytest.raises(ValueError):
        Controller(Config(client_set=FakeClientset()), backend=Engine, geometry=T.SMALL, echo_ledger=True)
