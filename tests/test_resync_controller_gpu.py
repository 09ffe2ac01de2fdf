"""GPU: the drop-in controller relisting with Replace (Controller.feed_list(...,
replace=True): kwok_resync_begin / _mark / _sweep, include/kwok_watch.h, DESIGN.md
§22) against the same controller that saw every change of the gap as watch
lines, DELETED included, each on its own fake clientset driven with the same
cluster events.  Controller A's watch callbacks are gated off for the gap (a
watch closed with 410 Gone: the reference reopens it and loses the gap,
pod_controller.go:280-290, node_controller.go:235-245); it then gets the full
List pages with replace=True, B the same pages with replace=False.  From that
step on every write and the final apiserver state must be identical, and so must
the engines' pod state."""
import pytest

import test_controller_cpu as T
import test_watch_controller_gpu as W
from fake_clientset import FakeClientset
from kwok_amd.controller import Config, Controller
from kwok_amd.engine import Engine
from test_list_controller_gpu import pages

pytestmark = pytest.mark.gpu

CONF = dict(manage_nodes_with_annotation_selector=T.MANAGE, cidr="10.0.0.1/24")
N_SLOTS = T.SMALL["buckets"] * T.SMALL["pod_slots_per_bucket"]


def gated_controller(cs, **kw):
    """W.feed_controller whose watches can be closed (close_watch: the lines not yet framed and every
    later event are lost) and reopened (gate[0] = True)"""
    c = Controller(Config(client_set=cs, **dict(CONF, **kw)), backend=Engine, geometry=T.SMALL)
    f = W.Feeder(c, "random")
    gate = [True]
    step = c.step

    def stepped(now):
        f.flush()
        return step(now)
    c.step = stepped

    def gated(cb):
        return lambda typ, obj: gate[0] and cb(typ, obj)
    cs.watch("nodes", gated(f.callback(True)), label_selector=c.conf.manage_nodes_with_label_selector)
    cs.watch("pods", gated(f.callback(False)), field_selector="spec.nodeName!=")
    gate.append(f)
    return c, gate


def close_watch(c, gate):
    """410 Gone: the connection ends; what it had not delivered yet never arrives"""
    gate[0] = False
    gate[1].held = {True: b"", False: b""}
    c.raw = {True: bytearray(), False: bytearray()}
    c.fed = set()


def populate(cs, nodes=12, pods=40):
    for i in range(nodes):
        cs.create(T.node("node-%03d" % i, managed=i % 5 != 4))
    for k in range(pods):
        cs.create(T.pod("pod-%04d" % k, "node-%03d" % (k % nodes), status={"phase": "Pending"}))


GONE_PODS = ["pod-%04d" % k for k in (0, 3, 4, 17, 28, 39)]  # on managed and unmanaged nodes
GONE_NODES = ["node-002", "node-004", "node-011"]             # 002 and the unmanaged 004 keep pods (zombies)


def gap(cs):
    """what happens while A's watch is closed: deletions and creations of nodes and pods"""
    for name in GONE_PODS:
        cs.delete("pods", ("default", name))
    for k in (11, 23, 35):  # every pod of node-011 goes with it: its entry is freed
        if "pod-%04d" % k not in GONE_PODS:
            cs.delete("pods", ("default", "pod-%04d" % k))
    for name in GONE_NODES:
        cs.delete("nodes", name)
    cs.create(T.node("node-new", managed=True))
    for k in range(5):
        cs.create(T.pod("late-%d" % k, "node-new" if k % 2 else "node-001", status={"phase": "Pending"}))
    q = cs.get("pods", ("default", "pod-0001"))
    q["metadata"].setdefault("labels", {})["touched"] = "yes"
    cs.update(q)


N_GONE_PODS = len(GONE_PODS) + 3


def feed_pages(c, cs, per_page, replace, kinds=("nodes", "pods")):
    for kind in kinds:
        for body in pages(cs, kind, per_page):
            c.feed_list(kind == "nodes", body, replace=replace)


def used_pods(c):
    return int(c.eng.dump_pods(0, N_SLOTS)[0].sum())


@pytest.mark.parametrize("per_page", [2, 500])
def test_relist_with_replace_equals_the_watch_that_saw_the_deletes(per_page):
    csa, csb = FakeClientset(), FakeClientset()
    (a, ga), (b, _gb) = gated_controller(csa), gated_controller(csb)
    for cs in (csa, csb):
        populate(cs)
    for t in (1, 2):
        for c in (a, b):
            c.step(T.S0 + 30 * t)
    assert csa.calls == csb.calls and len(csa.calls) > 40
    close_watch(a, ga)
    for cs in (csa, csb):
        gap(cs)
    ga[0] = True  # (the watch reopened at the list's version)
    feed_pages(a, csa, per_page, True)
    feed_pages(b, csb, per_page, False)
    n0 = len(csa.calls)
    for t in (3, 4, 5):
        for c in (a, b):
            c.step(T.S0 + 30 * t)
        assert csa.calls[n0:] == csb.calls[n0:], "step %d" % t
    assert len(csa.calls) > n0 + 10
    assert csa.store == csb.store
    da, db = a.eng.dump_pods(0, N_SLOTS), b.eng.dump_pods(0, N_SLOTS)
    assert all((x == y).all() for x, y in zip(da, db))
    assert a.size() == b.size()
    assert a.stats.resync_swept_pods == N_GONE_PODS and a.stats.resync_swept_nodes == len(GONE_NODES)
    assert a.stats.resync_skipped == 0
    assert (b.stats.resync_swept_pods, b.stats.resync_swept_nodes) == (0, 0)
    # the host maps forgot the swept objects and learned the listed ones
    assert a.pod_by_uid == b.pod_by_uid and a.pod_ref == b.pod_ref and a.node_handle == b.node_handle
    assert a.eng.resync_stats()["sessions"] == 2
    a.close()
    b.close()


def test_an_echo_of_the_controllers_own_patch_is_not_swept():
    """a step with the watch closed: the echoes of its heartbeat and pod patches never arrive, so the list
    items of those objects ARE the echoes and are dropped before the ingest - marked by their known handle"""
    cs = FakeClientset()
    c, gate = gated_controller(cs)
    populate(cs)
    c.step(T.S0 + 30)
    close_watch(c, gate)
    c.step(T.S0 + 60)  # heartbeats: their echoes are lost, as are those of the first step's pod patches
    cs.delete("pods", ("default", "pod-0007"))
    gate[0] = True
    size, used, dropped = c.size(), used_pods(c), c.stats.echoes_at_flush
    feed_pages(c, cs, 500, True)
    c.step(T.S0 + 90)
    assert c.stats.echoes_at_flush - dropped >= size  # (every managed node's item was an echo)
    assert c.stats.resync_swept_nodes == 0 and c.size() == size
    assert c.stats.resync_swept_pods == 1 and used_pods(c) == used - 1
    c.close()


def test_a_truncated_page_skips_the_sweep_and_a_clean_relist_sweeps():
    cs = FakeClientset()
    c, gate = gated_controller(cs)
    populate(cs)
    c.step(T.S0 + 30)
    c.step(T.S0 + 60)
    close_watch(c, gate)
    gap(cs)
    gate[0] = True
    used = used_pods(c)
    bodies = pages(cs, "pods", 7)
    assert len(bodies) > 3
    for k, body in enumerate(bodies):
        c.feed_list(False, body[:-9] if k == 1 else body, replace=True)
    c.step(T.S0 + 90)
    assert c.stats.resync_skipped == 1 and c.stats.list_bad_bodies == 1 and c.stats.resync_swept_pods == 0
    assert used_pods(c) >= used  # nothing deleted (the listed new pods came in)
    feed_pages(c, cs, 7, True, kinds=("pods",))
    c.step(T.S0 + 120)
    assert c.stats.resync_skipped == 1 and c.stats.resync_swept_pods == N_GONE_PODS
    assert used_pods(c) == len(cs.list("pods"))
    c.close()


class RecordingCNI:
    def __init__(self):
        self.removed, self.n = [], 0

    def setup(self, uid, name, namespace):
        self.n += 1
        return ["172.20.%d.%d" % (self.n // 250, self.n % 250 + 2)]

    def remove(self, uid, name, namespace):
        self.removed.append((uid, name, namespace))


def test_enable_cni_removes_exactly_the_swept_pods_on_managed_nodes():
    cs, cni = FakeClientset(), RecordingCNI()
    c, gate = gated_controller(cs, enable_cni=True, cni=cni)
    populate(cs)
    c.step(T.S0 + 30)
    c.step(T.S0 + 60)
    close_watch(c, gate)
    gone = ["pod-%04d" % k for k in (0, 3, 4, 17, 28, 39)]  # pod-0004 and -0028: on the unmanaged node-004
    uids = {n: cs.get("pods", ("default", n))["metadata"]["uid"] for n in gone}
    for n in gone:
        cs.delete("pods", ("default", n))
    gate[0] = True
    feed_pages(c, cs, 500, True, kinds=("pods",))
    c.step(T.S0 + 90)
    assert c.stats.resync_swept_pods == len(gone)
    managed = [n for n in gone if (int(n[4:]) % 12) % 5 != 4]
    assert sorted(cni.removed) == sorted((uids[n], n, "default") for n in managed) and len(managed) == 4
    c.close()


def test_a_session_spanning_two_steps_keeps_a_pod_the_watch_created_meanwhile():
    cs = FakeClientset()
    c, gate = gated_controller(cs)
    populate(cs)
    c.step(T.S0 + 30)
    c.step(T.S0 + 60)
    close_watch(c, gate)
    for n in GONE_PODS:
        cs.delete("pods", ("default", n))
    gate[0] = True
    first, *rest = pages(cs, "pods", 9)
    assert rest
    c.feed_list(False, first, replace=True)
    c.step(T.S0 + 90)
    assert c.resync[False] is not None and c.stats.resync_swept_pods == 0
    cs.create(T.pod("between", "node-001", status={"phase": "Pending"}))  # not in any page: a watch ADDED line
    c.step(T.S0 + 120)
    for body in rest:
        c.feed_list(False, body, replace=True)
    c.step(T.S0 + 150)
    assert c.resync[False] is None and c.stats.resync_swept_pods == len(GONE_PODS)
    assert used_pods(c) == len(cs.list("pods"))
    assert cs.get("pods", ("default", "between"))["status"].get("phase") == "Running"
    c.close()
