"""GPU: the drop-in controller told of the objects that exist before Start by
List pages (Controller.feed_list: kwok_frame_list_gpu + kwok_ingest_*_framed,
the reference's ListNodes / ListPods at Start, node_controller.go:282-296,
pod_controller.go:357-368) against the same controller told of them by watch
ADDED events, each on its own fake clientset: the reference's node and pod
controller tests as tests/test_controller_cpu.py restates them.  Later changes
reach both as watch bytes.  Every write (patches with their bodies, deletes) and
the final apiserver state must be identical."""
import json

import pytest

import test_controller_cpu as T
import test_watch_controller_gpu as W
from fake_clientset import FakeClientset
from kwok_amd.controller import Config, Controller
from kwok_amd.engine import Engine

pytestmark = pytest.mark.gpu


def pages(cs, kind, per_page):
    """the List response of the fake for one kind, paged: bodies whose continue token names the next page"""
    objs = cs.list(kind)
    if kind == "pods":  # the controller's field selector, spec.nodeName!=
        objs = [o for o in objs if (o.get("spec") or {}).get("nodeName")]
    out = []
    for k in range(0, max(len(objs), 1), per_page):
        md = {"resourceVersion": str(cs.rv)}
        if k + per_page < len(objs):
            md["continue"] = "page-%d" % (k + per_page)
        out.append(json.dumps({"kind": "NodeList" if kind == "nodes" else "PodList", "apiVersion": "v1", "metadata": md,
                               "items": objs[k:k + per_page]}, separators=(",", ":")).encode())
    return out


def list_controller(cs, per_page, cursors, suppress=True, backend=None, geometry=T.SMALL, **kw):
    """W.feed_controller, but what exists at Start arrives as List pages and the watches
    open after them (their replay of the existing objects is not delivered)"""
    c = Controller(Config(client_set=cs, **kw), backend=Engine, suppress_echoes=suppress, geometry=geometry)
    flush = c._flush_list

    def flushed(nodes, body):
        flush(nodes, body)
        cursors.append(("nodes" if nodes else "pods", dict(c.list_cursor.get("nodes" if nodes else "pods", {}))))
    c._flush_list = flushed
    for kind in ("nodes", "pods"):
        for body in pages(cs, kind, per_page):
            c.feed_list(kind == "nodes", body)
    f = W.Feeder(c, "random")
    step = c.step

    def stepped(now):
        f.flush()
        return step(now)
    c.step = stepped
    opened = []

    def after_open(cb):
        return lambda typ, obj: opened and cb(typ, obj)
    cs.watch("nodes", after_open(f.callback(True)), label_selector=c.conf.manage_nodes_with_label_selector)
    cs.watch("pods", after_open(f.callback(False)), field_selector="spec.nodeName!=")
    opened.append(True)
    return c


@pytest.mark.parametrize("per_page", [2, 500])
@pytest.mark.parametrize("name", ["test_reference_node_controller", "test_reference_pod_controller"])
def test_reference_tests_started_from_list_pages(name, per_page, monkeypatch):
    """the reference tests once with the existing objects as watch ADDED lines and
    once as List pages: their own assertions hold both times, and the two
    clientsets saw the same writes"""
    runs, cursors = [], []
    for make in (lambda cs, **kw: W.feed_controller(cs, "random", **kw),
                 lambda cs, **kw: list_controller(cs, per_page, cursors, **kw)):
        made = []

        def factory(cs, _make=make, **kw):
            made.append((cs, _make(cs, **kw), cs.rv, {k: len(v) for k, v in cs.store.items()}))
            return made[-1][1]
        monkeypatch.setattr(T, "controller", factory)
        getattr(T, name)()
        (cs, c, rv0, n0), = made
        runs.append((cs.calls, cs.store, c.stats))
    assert runs[0][0] == runs[1][0] and len(runs[0][0]) > 3
    assert runs[0][1] == runs[1][1]
    a, b = runs[0][2], runs[1][2]
    assert a.list_items == 0 and b.list_items >= 2 and b.list_host_items == 0 and b.list_bad_bodies == 0
    assert a.watch_frames == b.watch_frames + b.list_items  # the same objects, by the other road
    assert (a.node_records, a.pod_records) == (b.node_records, b.pod_records)
    # the cursor after every page: the fake's resourceVersion at the list, the token of the next page
    for kind in ("nodes", "pods"):
        got = [cur for k, cur in cursors if k == kind]
        n = n0[kind]  # (every pod of these tests has a node name: all are listed)
        want_tokens = ["page-%d" % k for k in range(per_page, n, per_page)] + [""]
        assert [g["continue_"] for g in got] == want_tokens, (kind, got)
        assert all(g["resource_version"] == str(rv0) and g["kind"] == ("NodeList" if kind == "nodes" else "PodList") for g in got)


def test_a_truncated_page_is_counted_and_changes_nothing():
    cs = FakeClientset(T.node("n0"), T.node("n1"), T.node("n2"))
    c = Controller(Config(client_set=cs, manage_all_nodes=True), backend=Engine, geometry=T.SMALL)
    good, = pages(cs, "nodes", 500)
    rv = str(cs.rv)
    c.feed_list(True, good[:-7])
    c.step(T.S0 + 30)
    assert c.stats.list_bad_bodies == 1 and c.stats.list_items == 0 and c.size() == 0 and cs.calls == []
    assert "nodes" not in c.list_cursor
    c.feed_list(True, good[:-7])   # a bad page and a good one in one step: the good one still applies
    c.feed_list(True, good)
    c.step(T.S0 + 60)
    assert c.stats.list_bad_bodies == 2 and c.stats.list_items == 3 and c.size() == 3
    assert c.list_cursor["nodes"] == dict(kind="NodeList", resource_version=rv, continue_="")
    assert all(cs.get("nodes", n)["status"].get("phase") == "Running" for n in ("n0", "n1", "n2"))
    assert len(cs.calls) >= 3
    c.feed_list(True, good)        # the same page again: upserts of known nodes, nothing is deleted
    c.feed_list(False, b'{"kind":"PodList","metadata":{"resourceVersion":"9"},"items":[]}')
    c.step(T.S0 + 90)
    assert c.size() == 3 and c.list_cursor["pods"] == dict(kind="PodList", resource_version="9", continue_="")
    c.close()
