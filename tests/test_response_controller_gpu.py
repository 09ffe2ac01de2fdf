"""GPU: the drop-in controller with response_bytes=True (the responses to the engine's own patches framed on
the device, the ledger's notes and the same-interval re-entry taken from the resident bytes)
against the same controller with response_bytes=False, every directory on in both, each on its own fake
clientset behind tests/response_bodies.RawClientset and fed the raw bytes of its watches.

The fleet: 3 nodes, 40 pods - pods created with an empty status (they re-enter and get their podIP in the
same interval: two patches of one pod, the second while the first one's echo is undelivered), pods with
finalizers that are deleted (the forget goes between the status patch's note and the finalizer patch's), and
with deliver="queued" two steps without a pump between them (a node's second heartbeat is noted while the echo
of its first is undelivered).  Equal in both runs: the clientset's request sequence and final objects,
stats.bodies, stats.echoes_at_flush, stats.reentered, kwok_echo_stats."""
import json

import pytest

import test_controller_cpu as T
import watch_frames as wf
from fake_clientset import FakeClientset
from kwok_amd import controller as ctl
from kwok_amd.controller import Config, Controller
from kwok_amd.engine import Engine
from response_bodies import RawClientset, compact

pytestmark = pytest.mark.gpu

N_PODS = 40


class JsonSpy:
    """stands in for the controller module's `json`: counts what the controller decodes and encodes"""

    def __init__(self):
        self.loads_calls = self.dumps_calls = 0

    def loads(self, *a, **kw):
        self.loads_calls += 1
        return json.loads(*a, **kw)

    def dumps(self, *a, **kw):
        self.dumps_calls += 1
        return json.dumps(*a, **kw)


def make(deliver, resp, mangle=None):
    cs = RawClientset(FakeClientset(deliver=deliver), mangle)
    c = Controller(Config(client_set=cs, manage_nodes_with_annotation_selector=T.MANAGE, node_ip="10.0.0.254", cidr="10.0.0.1/24"),
                   backend=Engine, geometry=T.SMALL, uid_directory=True, echo_ledger=True, ref_directory=True,
                   node_directory=True, response_bytes=resp)
    raw = {True: bytearray(), False: bytearray()}
    cs.watch("nodes", lambda typ, obj: raw[True].extend(wf.wrap(compact(obj), typ)))
    cs.watch("pods", lambda typ, obj: raw[False].extend(wf.wrap(compact(obj), typ)), field_selector="spec.nodeName!=")

    def step(now, pump=True):
        if pump:
            cs.pump()
        for nodes in (True, False):
            if raw[nodes]:
                c.feed_watch(nodes, bytes(raw[nodes]))
                raw[nodes].clear()
        return c.step(now)
    return cs, c, step


def drive(cs, step, mangle_step=None):
    """the cluster's events and the controller's steps; returns the bodies sent per step"""
    sent = []
    for k in range(3):
        cs.create(T.node("n%d" % k))
    sent.append(step(T.S0 + 30))
    for k in range(N_PODS):
        fin = ["kwok.x-k8s.io/x"] if k % 5 == 0 else []
        status = {} if k % 4 == 1 else {"phase": "Pending"}
        cs.create(T.pod("p%02d" % k, "n%d" % (k % 3), status=status, **({"finalizers": fin} if fin else {})))
    sent.append(step(T.S0 + 60))
    sent.append(step(T.S0 + 90, pump=False))  # the echoes of the step before stay undelivered: heartbeats are noted again
    for k in range(0, N_PODS, 3):             # deleted: every third pod, finalizers or not
        p = cs.get("pods", ("default", "p%02d" % k))
        p["metadata"]["deletionTimestamp"] = "2024-01-01T00:02:00Z"
        cs.update(p)
    for k in (50, 51):                        # late pods with an empty status: another re-entry
        cs.create(T.pod("p%02d" % k, "n1"))
    sent.append(step(T.S0 + 120))
    sent.append(step(T.S0 + 150))
    sent.append(step(T.S0 + 180))
    return sent


@pytest.mark.parametrize("deliver", ["sync", "queued"])
def test_response_bytes_equals_the_decoded_path(deliver, monkeypatch):
    spy = JsonSpy()
    runs = {}
    for resp in (True, False):
        cs, c, step = make(deliver, resp)
        if resp:
            monkeypatch.setattr(ctl, "json", spy)
        sent = drive(cs, step)
        if resp:
            monkeypatch.setattr(ctl, "json", json)
        runs[resp] = (cs, c, step, sent)
    (csa, ca, stepa, a), (csb, cb, stepb, b) = runs[True], runs[False]
    assert a == b and sum(a) > 80
    assert csa.inner.calls == csb.inner.calls
    assert csa.inner.store == csb.inner.store
    for k in ("bodies", "echoes_at_flush", "reentered"):
        assert getattr(ca.stats, k) == getattr(cb.stats, k), k
    assert ca.eng.echo_stats() == cb.eng.echo_stats()
    # the scenario holds what it is about: re-entries, finalizer deletes, echoes dropped at flush
    assert ca.stats.reentered == N_PODS // 4 + 2
    fin_deletes = [x for x in csa.inner.calls if x[0] == "patch_merge"]
    assert len(fin_deletes) == len([k for k in range(0, N_PODS, 3) if k % 5 == 0]) > 0
    assert ca.stats.echoes_at_flush > N_PODS
    # every deleted pod is deleted once: the finalizer patch's echo was dropped (its note stood behind the forget)
    deletes = [x[2] for x in csa.inner.calls if x[0] == "delete"]
    assert len(deletes) == len(set(deletes)) == len(range(0, N_PODS, 3))
    for k in range(N_PODS):
        if k % 3:
            st = csa.inner.store["pods"][("default", "p%02d" % k)]["status"]
            assert st["phase"] == "Running" and st["podIP"].startswith("10.0.0."), k
    # the response path: one frame per successful patch, none decoded on the host, no JSON in the controller
    patches = [x for x in csa.inner.calls if x[0] in ("patch_status", "patch_merge")]
    assert ca.stats.responses_framed == len(patches) == csa.raw_calls
    assert ca.stats.responses_host == 0 and ca.stats.response_bytes > 100 * len(patches)
    assert (spy.loads_calls, spy.dumps_calls) == (0, 0)
    rs = ca.eng.response_stats()
    assert rs["frames"] == len(patches) and rs["host_frames"] == 0 and rs["notes"] == ca.eng.echo_stats()["notes"]
    # response_bytes=False: nothing of the new path was called, launched or allocated
    assert csb.raw_calls == 0 and cb.eng.response_stats() == dict.fromkeys(rs, 0)
    assert (cb.stats.responses_framed, cb.stats.responses_host, cb.stats.response_bytes) == (0, 0, 0)
    assert ca.echo_q == [] and ca.reenter == [] and ca.rq["off"] == []

    # one more step: a response whose uid is spelt with a \\u escape takes the host fallback
    def mangle(obj):
        uid = obj["metadata"]["uid"]
        if obj.get("kind") == "Pod" and obj["metadata"]["name"] == "p60":
            return compact(obj).replace(b'"uid":"%s"' % uid.encode(), b'"uid":"\\u0075%s"' % uid[1:].encode()) + b"\n"
        return None
    csa.mangle = mangle
    for cs in (csa, csb):
        cs.create(T.pod("p60", "n2", status={"phase": "Pending"}))
    n0 = ca.stats.responses_host
    assert stepa(T.S0 + 210) == stepb(T.S0 + 210)
    assert ca.stats.responses_host - n0 == 1
    assert stepa(T.S0 + 240) == stepb(T.S0 + 240) == 3  # its echo was dropped: heartbeats only
    assert csa.inner.calls == csb.inner.calls and csa.inner.store == csb.inner.store
    assert ca.eng.echo_stats() == cb.eng.echo_stats()
    for k in ("bodies", "echoes_at_flush", "reentered"):
        assert getattr(ca.stats, k) == getattr(cb.stats, k), k
    ca.close()
    cb.close()


def test_response_bytes_needs_the_directories():
    for kw in (dict(), dict(uid_directory=True), dict(echo_ledger=False, uid_directory=True)):
        with pytest.raises(ValueError):
            Controller(Config(client_set=FakeClientset()), backend=Engine, geometry=T.SMALL, response_bytes=True, **kw)
