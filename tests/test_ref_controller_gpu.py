"""GPU: the drop-in controller with the engine's reference directory
(Controller(..., uid_directory=True, echo_ledger=True, ref_directory=True): kwok_read_refs,
kwok_refs_lookup, kwok_refs_bind; include/kwok_watch.h) against the same
controller with its host maps (uid_directory=True, echo_ledger=True), each on its own fake
clientset driven with the same cluster events, through the drivers of
test_uid_controller_gpu.py.  Every write, body for body, the final apiserver state and the
engine's pod state must be identical, and the new controller ends with no per-pod and no
per-node-handle map: pod_ref == pod_uid == node_name == {}."""
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


def feed_controller(cs, refs, **kw):
    """U.feed_controller(uid_directory=True) with the ledger on and the reference directory switch"""
    plain = U.Controller
    U.Controller = functools.partial(Controller, echo_ledger=True, ref_directory=refs)
    try:
        return U.feed_controller(cs, True, **kw)
    finally:
        U.Controller = plain


class RecordingCNI:
    def __init__(self):
        self.calls, self.n = [], 0

    def setup(self, uid, name, namespace):
        self.n += 1
        self.calls.append(("setup", uid, name, namespace))
        return ["172.20.%d.%d" % (self.n // 250, self.n % 250 + 2)]

    def remove(self, uid, name, namespace):
        self.calls.append(("remove", uid, name, namespace))


def same_end(ca, cb, csa, csb, engines=True):
    assert csa.store == csb.store
    if engines:
        da, db = ca.eng.dump_pods(0, R.N_SLOTS), cb.eng.dump_pods(0, R.N_SLOTS)
        assert all((x == y).all() for x, y in zip(da, db))
    # the maps the directory replaces stay empty; the ones out of its scope are the host controller's
    assert ca.refs and not cb.refs
    assert ca.pod_ref == ca.pod_uid == ca.node_name == {} and ca.pod_by_uid == cb.pod_by_uid == {}
    assert ca.node_handle == cb.node_handle and ca.node_uid == cb.node_uid
    assert ca.stats == cb.stats and ca.stats.refs_missing == 0
    assert ca.echo.rv == {} and ca.echo_q == []


def test_the_directory_needs_the_other_two():
    for kw in (dict(), dict(uid_directory=True), dict(echo_ledger=False, uid_directory=True)):
        with pytest.raises(ValueError):
            Controller(Config(client_set=FakeClientset()), backend=Engine, geometry=T.SMALL, ref_directory=True, **kw)


@pytest.mark.parametrize("name", ["test_reference_node_controller", "test_reference_pod_controller"])
def test_reference_tests(name, monkeypatch):
    runs = []
    for refs in BOTH:
        made = []

        def factory(cs, _refs=refs, **kw):
            made.append((cs, feed_controller(cs, _refs, **kw)))
            return made[-1][1]
        monkeypatch.setattr(T, "controller", factory)
        getattr(T, name)()
        runs.append(made[0])
    (csa, ca), (csb, cb) = runs
    assert csa.calls == csb.calls and len(csa.calls) > 3
    assert ca.stats.watch_frames > 0 and ca.stats.watch_bad_frames == 0
    same_end(ca, cb, csa, csb, engines=False)  # (the reference tests close their controller)
    if name.endswith("pod_controller"):
        assert ca.stats.pod_records > 0 and cb.pod_uid


@pytest.mark.parametrize("mixed", [False, True], ids=["raw", "typed-and-raw"])
@pytest.mark.parametrize("deliver", ["sync", "queued"])
def test_scenario(deliver, mixed):
    """nodes and pods created, modified and deleted over 5 ticks; mixed: the pod watch is typed events in every
    other step, whose creates the typed path names with kwok_refs_bind"""
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
    s = ca.eng.refs_stats()
    assert s["notes"] > 0 and s["reads"] > 100 and s["not_found"] == 0
    assert (s["unnamed"] > 0) == mixed and (s["binds"] > 0 or not mixed)  # (typed creates carry no name; they are bound right after)
    assert cb.eng.refs_stats() == dict.fromkeys(s, 0)
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
def test_relist_with_replace_and_cni(per_page):
    """R's relist with EnableCNI: cni.Setup is called for the pods that wait for an address and cni.Remove for
    the swept pods on managed nodes, by the names and uids the device hands back"""
    csa, csb = FakeClientset(), FakeClientset()
    cna, cnb = RecordingCNI(), RecordingCNI()
    ca = feed_controller(csa, True, enable_cni=True, cni=cna, **R.CONF)
    cb = feed_controller(csb, False, enable_cni=True, cni=cnb, **R.CONF)
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
    assert cna.calls == cnb.calls
    assert sum(c[0] == "setup" for c in cna.calls) > 20 and sum(c[0] == "remove" for c in cna.calls) > 2
    same_end(ca, cb, csa, csb)
    ca.close()
    cb.close()
