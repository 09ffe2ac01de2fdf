"""GPU: the drop-in controller fed with raw watch bytes (Controller.feed_watch:
kwok_frame_watch_gpu + kwok_ingest_*_framed) against the same controller fed
with typed events (on_event), each on its own fake clientset driven with the
same cluster events: the reference's node and pod controller tests
(node_controller_test.go:37-155, pod_controller_test.go:37-194 as
tests/test_controller_cpu.py restates them), the create / modify / delete
scenario and the same-interval IP case.  The watch lines reach feed_watch in
chunks cut at arbitrary byte positions - mid-line, and byte by byte.  Every
write (patches with their bodies, deletes) and the final apiserver state must be
identical."""
import json
import random

import pytest

import test_controller_cpu as T
from fake_clientset import FakeClientset
from kwok_amd.controller import Config, Controller
from kwok_amd.engine import Engine

pytestmark = pytest.mark.gpu


class Feeder:
    """the two watch responses as byte streams: every event one line, handed to
    feed_watch in chunks; everything written so far has arrived when a step begins"""

    def __init__(self, c, chunking, seed=5):
        self.c, self.chunking, self.rng = c, chunking, random.Random(seed)
        self.held = {True: b"", False: b""}

    def callback(self, nodes):
        def cb(typ, obj):
            self.held[nodes] += b'{"type":"%s","object":%s}\n' % (typ.encode(),
                                                                 json.dumps(obj, separators=(",", ":")).encode())
            self.deliver(nodes, self.rng.randrange(len(self.held[nodes]) + 1))  # (often ends mid-line)
        return cb

    def deliver(self, nodes, n):
        data, self.held[nodes] = self.held[nodes][:n], self.held[nodes][n:]
        while data:
            k = 1 if self.chunking == "bytes" else self.rng.randint(1, 700)
            self.c.feed_watch(nodes, data[:k])
            data = data[k:]

    def flush(self):
        for nodes in (True, False):
            self.deliver(nodes, len(self.held[nodes]))


def feed_controller(cs, chunking="random", suppress=True, backend=None, geometry=T.SMALL, **kw):
    """T.controller, but the watches deliver raw bytes"""
    c = Controller(Config(client_set=cs, **kw), backend=Engine, suppress_echoes=suppress, geometry=geometry)
    f = Feeder(c, chunking)
    step = c.step

    def stepped(now):
        f.flush()
        return step(now)
    c.step = stepped
    cs.watch("nodes", f.callback(True), label_selector=c.conf.manage_nodes_with_label_selector)
    cs.watch("pods", f.callback(False), field_selector="spec.nodeName!=")
    return c


_controller = T.controller  # (the reference tests' factory is replaced below)


def event_controller(cs, **kw):
    kw.pop("backend", None)
    return _controller(cs, backend=Engine, **kw)


@pytest.mark.parametrize("chunking", ["random", "bytes"])
@pytest.mark.parametrize("name", ["test_reference_node_controller", "test_reference_pod_controller"])
def test_reference_tests_fed_as_watch_streams(name, chunking, monkeypatch):
    """the reference tests once through on_event and once through feed_watch: their
    own assertions hold both times, and the two clientsets saw the same writes"""
    runs = []
    for make in (event_controller, lambda cs, **kw: feed_controller(cs, chunking, **kw)):
        made = []

        def factory(cs, _make=make, **kw):
            made.append((cs, _make(cs, **kw)))
            return made[-1][1]
        monkeypatch.setattr(T, "controller", factory)
        getattr(T, name)()
        (cs, c), = made
        runs.append((cs.calls, cs.store, c.stats))
    assert runs[0][0] == runs[1][0] and len(runs[0][0]) > 3
    assert runs[0][1] == runs[1][1]
    assert runs[1][2].watch_frames > 0 and runs[1][2].watch_bad_frames == 0 and runs[0][2].watch_frames == 0
    assert runs[0][2].pod_runs == runs[1][2].pod_runs


@pytest.mark.parametrize("chunking", ["random", "bytes"])
@pytest.mark.parametrize("deliver", ["sync", "queued"])
def test_scenario_fed_as_watch_streams(deliver, chunking):
    """nodes and pods created, modified and deleted over 5 ticks (Added + Modified and
    Added + Deleted within one interval: several runs per batch), an external node
    status change: every write equal tick by tick, the same echoes dropped"""
    ce, cf = FakeClientset(deliver=deliver), FakeClientset(deliver=deliver)
    e = event_controller(ce, manage_nodes_with_annotation_selector=T.MANAGE, cidr="10.0.0.1/24")
    f = feed_controller(cf, chunking, manage_nodes_with_annotation_selector=T.MANAGE, cidr="10.0.0.1/24")
    a, b = T.scenario(ce, e), T.scenario(cf, f)
    for t, (x, y) in enumerate(zip(a, b)):
        assert x == y, "tick %d" % t
    assert sum(len(x) for x in a) > 100
    assert ce.store == cf.store
    # the same events were dropped as echoes: the records ingested are the same (below).  The
    # counts agree when the echoes overtake their patch (sync: both drop them at the next
    # step); queued, on_event drops the last tick's echoes on arrival, after the last step,
    # while their bytes wait for a step that never comes
    dropped = e.stats.echoes_on_arrival + e.stats.echoes_at_flush
    assert 50 < f.stats.echoes_at_flush <= dropped and f.stats.echoes_on_arrival == 0
    if deliver == "sync":
        assert f.stats.echoes_at_flush == dropped
    assert (e.stats.node_records, e.stats.pod_records, e.stats.pod_runs) == \
        (f.stats.node_records, f.stats.pod_records, f.stats.pod_runs)
    assert f.stats.pod_runs > 5 and f.stats.rejected == e.stats.rejected
    e.close()
    f.close()


@pytest.mark.parametrize("deliver", ["sync", "queued"])
def test_same_interval_ip_fed_as_watch_streams(deliver):
    """controller.py's step 6 (an IP-less pod patch re-enters within the interval)
    with the watches as byte streams: the same pod writes in the same steps"""
    ce, cf = FakeClientset(deliver=deliver), FakeClientset(deliver=deliver)
    kw = dict(manage_nodes_with_annotation_selector=T.MANAGE, node_ip="10.0.0.254", cidr="10.0.0.1/24")
    e, f = event_controller(ce, **kw), feed_controller(cf, "random", **kw)
    a, b = T.empty_status_scenario(ce, e), T.empty_status_scenario(cf, f)
    assert a == b and len(a[0]) == 5 and a[1] == a[2] == []
    assert e.stats.reentered == f.stats.reentered == 2
    assert ce.store == cf.store
    e.close()
    f.close()


def test_tail_mixing_and_skipped_frames():
    """a line cut by a step waits for its rest; malformed lines, BOOKMARK and ERROR
    frames are counted and skipped; on_event and feed_watch do not mix for one kind
    within a step (the other kind is free)"""
    cs = FakeClientset()
    c = Controller(Config(client_set=cs, manage_all_nodes=True), backend=Engine, geometry=T.SMALL)
    obj = cs.create(T.node("n0")) or cs.get("nodes", "n0")
    line = b'{"type":"ADDED","object":%s}\n' % json.dumps(obj, separators=(",", ":")).encode()
    c.feed_watch(True, b'{"type":"BOOKMARK","object":{"metadata":{"resourceVersion":"3"}}}\n\r\n{"type":"ADDED"}\nnot json\n'
                       b'{"type":"ERROR","object":{"kind":"Status","code":410}}\n' + line[:37])
    with pytest.raises(ValueError):
        c.on_event(True, "ADDED", obj)
    c.on_event(False, "ADDED", cs.create(T.pod("p0", "n0", status={"phase": "Pending"})))
    with pytest.raises(ValueError):
        c.feed_watch(False, b"\n")
    c.step(T.S0 + 30)
    s = c.stats
    assert (s.watch_frames, s.watch_bad_frames, s.watch_skipped, s.node_records) == (5, 2, 2, 0)
    assert c.size() == 0 and bytes(c.raw[True]) == line[:37]
    c.feed_watch(True, line[37:])
    c.step(T.S0 + 60)
    assert c.size() == 1 and c.has("n0") and c.stats.node_records == 1 and not c.raw[True]
    assert cs.get("nodes", "n0")["status"].get("phase") == "Running"
    c.on_event(True, "MODIFIED", cs.get("nodes", "n0"))  # a new step: either way again
    c.step(T.S0 + 90)
    c.close()
