"""GPU: the drop-in controller with node_status_gpu=True (the device canonicalises the status blobs of the node
documents it decodes; include/kwok_canon.h) against the same controller with
node_status_gpu=False, each on its own in-memory apiserver.

The first life: nodes registered with and without resources arrive as watch bytes, kwok patches them.  Then the
controller restarts: a new one is told of the nodes by List pages - every one of them now holds the status kwok
patched, addresses in struct order and all - and goes on from the watch.  Equal in both runs: the clientset's
requests and final objects and every statistic but node_docs_host / node_docs_canon.  With the feature on the
restart leaves no node document to the host codec."""
import json

import pytest

import test_controller_cpu as T
import watch_frames as wf
from fake_clientset import FakeClientset
from kwok_amd import abi
from kwok_amd import controller as ctl
from kwok_amd.controller import Config, Controller
from kwok_amd.engine import Engine
from response_bodies import compact
from test_list_controller_gpu import pages
from test_response_controller_gpu import JsonSpy

pytestmark = pytest.mark.gpu

N_NODES = 9
DIRS = dict(uid_directory=True, echo_ledger=True, ref_directory=True, node_directory=True)


class Life:
    """one controller on the clientset, fed the raw bytes of its node watch"""

    def __init__(self, cs, on, dirs, listed):
        self.cs = cs
        self.c = Controller(Config(client_set=cs, manage_nodes_with_annotation_selector=T.MANAGE, node_ip="10.0.0.254",
                                   cidr="10.0.0.1/24"), backend=Engine, geometry=T.SMALL, node_status_gpu=on,
                            **(DIRS if dirs else {}))
        self.decodes = 0
        inner = self.c.codec.decode_nodes

        def spied(*a, **kw):  # the Python road to the host codec's node decode
            self.decodes += 1
            return inner(*a, **kw)
        self.c.codec.decode_nodes = spied
        self.raw = bytearray()
        if listed:  # what exists arrives as List pages; the watch opens behind them (its replay is not delivered)
            for body in pages(cs, "nodes", 4):
                self.c.feed_list(True, body)
        opened = []
        cs.watch("nodes", lambda typ, obj: opened and self.raw.extend(wf.wrap(compact(obj), typ)))
        opened.append(True)

    def step(self, now):
        self.cs.pump()
        if self.raw:
            self.c.feed_watch(True, bytes(self.raw))
            self.raw.clear()
        return self.c.step(now)


def run(on, dirs, monkeypatch):
    cs = FakeClientset(deliver="sync")
    first = Life(cs, on, dirs, listed=False)
    res = {"cpu": "4", "memory": "8Gi", "pods": "110"}
    for k in range(N_NODES):
        st = None
        if k % 3 == 1:  # registered with resources, addresses in struct order
            st = {"addresses": [{"type": "InternalIP", "address": "10.1.0.%d" % k}, {"type": "Hostname", "address": "n%d" % k}],
                  "capacity": dict(res, cpu=str(k)), "allocatable": dict(res)}
        cs.create(T.node("n%d" % k, status=st))
    sent = [first.step(T.S0 + 30), first.step(T.S0 + 60)]
    stats1 = first.c.stats
    canon1 = first.c.eng.canon_stats()
    first.c.close()
    # every node holds the status kwok patched
    for k in range(N_NODES):
        st = cs.store["nodes"]["n%d" % k]["status"]
        assert st["phase"] == "Running" and st["addresses"] and st["allocatable"], k
    spy = JsonSpy()
    monkeypatch.setattr(ctl, "json", spy)
    second = Life(cs, on, dirs, listed=True)
    sent += [second.step(T.S0 + 90)]
    monkeypatch.setattr(ctl, "json", json)
    cs.create(T.node("late", status={"capacity": dict(res), "allocatable": dict(res)}))
    sent += [second.step(T.S0 + 120), second.step(T.S0 + 150)]
    out = dict(calls=list(cs.calls), store=cs.store, sent=sent,
               stats1=stats1, stats2=second.c.stats, canon1=canon1, canon2=second.c.eng.canon_stats(),
               decodes=first.decodes + second.decodes, loads=spy.loads_calls)
    second.c.close()
    return out


def same_stats(a, b):
    da, db = dict(vars(a)), dict(vars(b))
    for k in ("node_docs_host", "node_docs_canon"):
        da.pop(k), db.pop(k)
    return da == db


@pytest.mark.parametrize("dirs", [False, True], ids=["plain", "directories"])
def test_restart_needs_no_host_node_decode(dirs, monkeypatch):
    a = run(True, dirs, monkeypatch)
    b = run(False, dirs, monkeypatch)
    assert a["calls"] == b["calls"] and len(a["calls"]) > N_NODES
    assert a["store"] == b["store"]
    assert a["sent"] == b["sent"]
    assert same_stats(a["stats1"], b["stats1"]) and same_stats(a["stats2"], b["stats2"])
    # the restart: every listed node holds blobs; none goes to the host codec with the feature on
    assert a["stats2"].list_items == N_NODES
    assert a["stats2"].node_docs_host == 0 and b["stats2"].node_docs_host > N_NODES
    assert a["stats2"].node_docs_canon == a["canon2"]["docs"] > N_NODES and a["canon2"]["docs_host"] == 0
    assert a["stats1"].node_docs_host == 0 and b["stats1"].node_docs_host >= N_NODES // 3
    assert a["stats1"].node_docs_canon == a["canon1"]["docs"] >= N_NODES // 3
    # off is off: nothing of the feature ran
    zero = dict.fromkeys(abi.CANON_STATS, 0)
    assert b["canon1"] == zero and b["canon2"] == zero
    assert b["stats1"].node_docs_canon == 0 and b["stats2"].node_docs_canon == 0
    # no host node decode: not through the Python codec, and the controller decoded no JSON of its own at the relist
    assert a["decodes"] == 0 and a["loads"] == b["loads"] == 0


def test_node_status_gpu_needs_the_engine_backend():
    from oracle.oracle import Oracle
    with pytest.raises(ValueError):
        Controller(Config(client_set=FakeClientset()), backend=Oracle, geometry=T.SMALL, node_status_gpu=True)
