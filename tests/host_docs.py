"""Pod documents that k_json_pods lists for the host (json.hip; json_complete in
kwok_amd/csrc/engine.cpp completes them), as small watch batches, and the reference they
are checked against: the host codec's records fed to the CPU oracle, specs registered in
document order.

A batch is a list of Line(type, doc, kind, status, ...).  kind states why the device hands
the document to the host, or "dev" when it decides the document itself:
  host   JSON_HOST: an escape in a compared string (phase, a condition type, a label key
         under a label selector), or a codec whose selectors exceed the device tables
         (every document of the call)
  spec   JSON_SPEC: an upsert whose pod spec the device's table does not answer: not
         registered when the call starts
  spec2  JSON_SPEC too: registered, but its key is shared by two registered specs (the
         table answers -2 for it), which only KWOK_DEBUG_SPEC_KEY_BITS brings about here
  specx  JSON_SPEC_X: the spec key hits one registered spec whose strings differ
status is the per-document status every entry point must answer (the host codec's, or
KWOK_EDOMAIN for a spec kwok_register_pod_spec refuses).  A batch states n_host, the number
of documents listed, and the number of lines of each kind; tests/test_host_docs_cpu.py
proves all of it against the host codec and the oracle without a GPU, and
tests/test_json_host_docs_gpu.py holds every JSON entry point of the engine to it.

Uids are unique within a batch (the by-uid entries then send one run per call, so a spec
registered by the call is not yet known to any document of it).  Pods that a later batch
modifies or deletes arrive holding their addresses (a podIP of the CIDR far above what the
pool hands out here), so a restated document is what the apiserver would send."""
import json
from collections import Counter, namedtuple

import numpy as np

from harness import pod_doc
from kwok_amd import abi
from kwok_amd.codec import Codec
from kwok_amd.engine import KwokError, make_config
from oracle.oracle import Oracle

T0 = 1704067230
# the geometry of tests/test_uid_ingest_gpu.py
KW = dict(cidr="10.0.0.1/16", node_ip="196.168.0.1", buckets=64, node_slots_per_bucket=32, pod_slots_per_bucket=512)
NODES = ["node-%03d" % i for i in range(12)]
TIER = dict(manage_all_nodes=True, disregard_status_with_label_selector="tier=custom")
# nine requirements: more than the device's selector table holds (JSEL_REQ = 8)
NINE = dict(manage_all_nodes=True,
            disregard_status_with_label_selector="tier in (custom),!s1,!s2,!s3,!s4,!s5,!s6,!s7,!s8")

A = ((("fake-pod", "fake"),), (), ())
B = ((("a", "img-a"), ("b", "img/b:v2")), (("init", "busybox"),), ("g.io/x",))
C_ = ((("web", "nginx:1.25"),), (), ("g.io/ready",))
D = ((("side", "envoy:v1"), ("app", "app:3")), (), ())
E = ((("fake-pod", "fake:2"),), (), ())  # an image bump that only a Deleted line's object shows
# 32 containers with long names and images: the pod patch is longer than 64 KiB, which
# kwok_register_pod_spec refuses with KWOK_EDOMAIN (the host codec accepts the document)
BIG = (tuple(("c%02d-" % k + "n" * 200, "registry.example/" + "i" * 1900 + "-%02d" % k) for k in range(32)), (), ())

ESCAPES = {"phase": (b'"phase":"Running"', b'"phase":"Runn\\u0069ng"'),
           "cond": (b'"type":"Ready"', b'"type":"Re\\u0061dy"'),
           "tier": (b'"tier":', b'"t\\u0069er":'),
           "app": (b'"app":', b'"\\u0061pp":')}

Line = namedtuple("Line", "type doc kind status uid spec esc refused")
Batch = namedtuple("Batch", "name lines n_host kinds create_only")
Scenario = namedtuple("Scenario", "name codec_kw key_bits pre_specs batches unseen")


def canon_bytes(spec):
    """the string kwok_spec_key hashes (engine.cpp json_spec_canon)"""
    c, i, g = spec
    o = b""
    for n, im in c:
        o += n.encode() + b"\x1f" + im.encode() + b"\x1e"
    o += b"\x1d"
    for n, im in i:
        o += n.encode() + b"\x1f" + im.encode() + b"\x1e"
    o += b"\x1d"
    for x in g:
        o += x.encode() + b"\x1e"
    return o


def fnv_key(spec, bits=64):
    """kwok_spec_key (FNV-1a 64 of the canonical string), cut to its low `bits` bits"""
    h = 0xCBF29CE484222325
    for ch in canon_bytes(spec):
        h = ((h ^ ch) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h & ((1 << bits) - 1)


class Docs:
    """the documents of one scenario; pods that hold addresses take them from one counter"""

    def __init__(self):
        self.ips = 0
        self.pods = {}  # key -> the arguments of its create (a later line restates the pod)

    def line(self, typ, key, spec=A, kind="dev", status=abi.OK, esc=None, carrier=False, conforms=False, tier=False,
             no_ctime=False, node=None, refused=False, doc_spec=None):
        """carrier: the pod holds hostIP and podIP and is Running (conforms: with the status the template
        renders); tier: labelled tier=custom (disregarded under TIER / NINE); doc_spec: the spec the document
        shows where it differs from the pod's (a Deleted line after an image bump)"""
        if typ == "ADDED":
            ip = None
            if carrier:
                ip = "10.0.%d.%d" % (200 + self.ips // 250, 1 + self.ips % 250)
                self.ips += 1
            self.pods[key] = dict(spec=spec, carrier=carrier, conforms=conforms, tier=tier, ip=ip,
                                  node=node or NODES[len(self.pods) % len(NODES)])
        p = self.pods[key]
        shown = doc_spec or p["spec"]
        ev = dict(key=key, node=p["node"], disregard=False, deleting=False, finalizers=0, creation=T0 - 90, phase="Pending",
                  status_nonempty=False, conforms=False, hostIP="", podIP="",
                  spec={"containers": [list(x) for x in shown[0]], "init": [list(x) for x in shown[1]], "gates": list(shown[2])})
        if p["carrier"]:
            ev.update(phase="Running", status_nonempty=True, conforms=p["conforms"], hostIP=KW["node_ip"], podIP=p["ip"])
        d = pod_doc(ev)
        if p["tier"]:
            d["metadata"]["labels"]["tier"] = "custom"
        if no_ctime:
            del d["metadata"]["creationTimestamp"]
        raw = json.dumps(d, separators=(",", ":")).encode()
        if esc:
            old, new = ESCAPES[esc]
            assert raw.count(old) >= 1, (key, esc)
            raw = raw.replace(old, new, 1)
        return Line(typ, raw, kind, status, ("u-" + key).encode(), shown, esc, refused)


def batch(name, lines, n_host, **kinds):
    """n_host and the per-kind counts are stated by the caller, not derived from the lines"""
    assert len(set(l.uid for l in lines)) == len(lines), name + ": a uid twice in one batch"
    return Batch(name, lines, n_host, dict(kinds), all(l.type == "ADDED" for l in lines))


def escapes():
    """JSON_HOST by escape - phase, condition type, label key - as creates, as modifies of existing pods and
    as the objects of Deleted lines, among device-decided documents; JSON_SPEC creates with repeats; a
    JSON_HOST upsert that brings a new spec, and a plain document of that spec behind it; a host-rejected
    listed document; a listed Deleted line whose object shows a spec never registered"""
    m = Docs()
    b0 = [m.line("ADDED", "s%d" % k, (A, B, C_)[k % 3], "spec") for k in range(12)]
    b1 = [m.line("ADDED", "c1-0"),
          m.line("ADDED", "ep", A, "host", esc="phase", carrier=True),
          m.line("ADDED", "car-0", B, carrier=True, conforms=True),
          m.line("ADDED", "ec", B, "host", esc="cond", carrier=True, conforms=True),
          m.line("ADDED", "el", C_, "host", esc="tier", tier=True),
          m.line("ADDED", "dl", C_, tier=True),
          m.line("ADDED", "ea", A, "host", esc="app"),
          m.line("ADDED", "ed", D, "host", esc="phase", carrier=True),
          m.line("ADDED", "car-1", A, carrier=True, conforms=True),
          m.line("ADDED", "bad", A, "host", abi.EDOMAIN, esc="phase", carrier=True, no_ctime=True),
          m.line("ADDED", "d-plain", D, "spec")]
    b2 = [m.line("MODIFIED", "ep", kind="host", esc="phase"), m.line("MODIFIED", "car-0"),
          m.line("MODIFIED", "ec", kind="host", esc="cond"), m.line("MODIFIED", "el", kind="host", esc="tier"),
          m.line("MODIFIED", "car-1"), m.line("MODIFIED", "ed", kind="host", esc="phase")]
    b3 = [m.line("DELETED", "ep", kind="host", esc="phase"), m.line("DELETED", "car-0"),
          m.line("DELETED", "ec", kind="host", esc="cond"), m.line("DELETED", "el", kind="host", esc="tier"),
          m.line("DELETED", "car-1", kind="host", esc="phase", doc_spec=E)]
    return Scenario("escapes", TIER, None, [], [batch("new specs", b0, 12, spec=12),
                                                batch("escaped creates", b1, 7, dev=4, host=6, spec=1),
                                                batch("escaped modifies", b2, 4, dev=2, host=4),
                                                batch("escaped deletes", b3, 4, dev=1, host=4)], [E])


def all_host():
    """a codec whose selector has nine requirements: every document of every call is JSON_HOST"""
    m = Docs()
    b0 = [m.line("ADDED", "h%d" % k, (A, B)[k % 2], "host", carrier=k < 8, conforms=k < 8, tier=k % 3 == 0) for k in range(16)]
    b1 = ([m.line("MODIFIED", "h%d" % k, kind="host") for k in range(4)] +
          [m.line("ADDED", "n%d" % k, C_, "host", tier=k == 1) for k in range(2)] +
          [m.line("DELETED", "h%d" % k, kind="host") for k in (4, 5)] +
          [m.line("ADDED", "n%d" % k, C_, "host") for k in (2, 3)])
    return Scenario("all-host", NINE, None, [], [batch("creates", b0, 16, host=16), batch("mixed", b1, 10, host=10)], [])


def refused_spec():
    """one document whose spec kwok_register_pod_spec refuses, listed documents before and after it"""
    m = Docs()
    b0 = [m.line("ADDED", "r0", C_, "spec"), m.line("ADDED", "r1"),
          m.line("ADDED", "r2", A, "host", esc="phase", carrier=True),
          m.line("ADDED", "big", BIG, "spec", abi.EDOMAIN, refused=True),
          m.line("ADDED", "r3", C_, "spec"), m.line("ADDED", "r4"), m.line("ADDED", "r5", D, "spec"),
          m.line("ADDED", "r6", B, "host", esc="cond", carrier=True, conforms=True), m.line("ADDED", "r7", D, "spec")]
    return Scenario("refused-spec", TIER, None, [A], [batch("around the refused spec", b0, 7, dev=2, host=2, spec=5)], [])


def keyed_specs(bits=1):
    """P (key 1, registered first), X1 and X2 (key 1 too: they collide with it) and S0 (key 0, which the
    device's table never answers), found by their FNV keys"""
    by = {0: [], 1: []}
    for k in range(64):
        s = ((("k%d" % k, "img"),), (), ())
        by[fnv_key(s, bits)].append(s)
    return by[1][0], by[1][1], by[1][2], by[0][0]


def spec_collisions():
    """KWOK_DEBUG_SPEC_KEY_BITS=1: batch 1 registers one spec; batch 2 brings three further specs, two of
    which share its key (JSON_SPEC_X, the first of them ahead of every JSON_SPEC and JSON_HOST document),
    each repeated; batch 3 restates all four once the key is shared by registered specs (all JSON_SPEC)"""
    P, X1, X2, S0 = keyed_specs()
    m = Docs()
    b0 = [m.line("ADDED", "p0", P, "spec"), m.line("ADDED", "p1", P, "spec")]
    b1 = [m.line("ADDED", "x1-0", X1, "specx"), m.line("ADDED", "s0-0", S0, "spec"),
          m.line("ADDED", "e0", P, "host", esc="phase", carrier=True), m.line("ADDED", "x2-0", X2, "specx"),
          m.line("ADDED", "p2", P), m.line("ADDED", "x1-1", X1, "specx"), m.line("ADDED", "s0-1", S0, "spec"),
          m.line("ADDED", "x2-1", X2, "specx"), m.line("ADDED", "p3", P)]
    b2 = [m.line("ADDED", "p4", P, "spec2"), m.line("ADDED", "x1-2", X1, "spec2"), m.line("ADDED", "s0-2", S0, "spec2"),
          m.line("ADDED", "x2-2", X2, "spec2"), m.line("DELETED", "e0")]
    return Scenario("spec-collisions", TIER, 1, [], [batch("one spec", b0, 2, spec=2),
                                                    batch("colliding specs", b1, 7, dev=2, host=1, spec=2, specx=4),
                                                    batch("a shared key", b2, 4, dev=1, spec2=4)], [])


EDGES = (1, 2, 255, 256, 257)


def block_edges():
    """1, 2, 255, 256 and 257 listed documents per call (k_json_gather / k_json_scatter: 256 threads a
    block): a new spec per call, every seventh listed document a JSON_HOST one instead, a device-decided
    document after every fourth"""
    m = Docs()
    out = []
    for k in EDGES:
        s = ((("edge-%d" % k, "img:%d" % k),), (), ())
        lines, host = [], 0
        for j in range(k):
            if j % 7 == 3:
                lines.append(m.line("ADDED", "g%d-%d" % (k, j), s, "host", esc="phase", carrier=True))
                host += 1
            else:
                lines.append(m.line("ADDED", "g%d-%d" % (k, j), s, "spec"))
            if j % 4 == 3:
                lines.append(m.line("ADDED", "g%d-%d-dev" % (k, j)))
        out.append(batch("%d listed" % k, lines, k, dev=k // 4, host=(k + 3) // 7, spec=k - (k + 3) // 7))
        assert host == (k + 3) // 7
    return Scenario("block-edges", TIER, None, [A], out, [])


SCENARIOS = {"escapes": escapes, "all-host": all_host, "refused-spec": refused_spec, "spec-collisions": spec_collisions,
             "block-edges": block_edges}


def node_events(names=NODES):
    ar = abi.Arena()
    ev = np.zeros(len(names), abi.NODE_EVENT_DTYPE)
    ev["op"], ev["managed"], ev["lockable"] = abi.OP_UPSERT, 1, 1
    for i, n in enumerate(names):
        ev[i]["name"] = ar.ref(n)
    return ev, bytes(ar.buf)


class Ref:
    """the reference of one scenario: the host codec's records through the CPU oracle, specs registered in
    document order (as Lock.send in tests/test_uid_ingest_gpu.py builds them), and the uid -> handle map a
    caller of the by-handle entries keeps"""

    def __init__(self, sc):
        self.sc = sc
        self.o = Oracle(make_config(**KW))
        self.codec = Codec(**sc.codec_kw)
        self.spec_id = {}   # spec -> id, in registration order
        for s in sc.pre_specs:
            self.register(s)
        h, st = self.o.ingest_nodes_raw(*node_events())
        assert not st.any()
        self.node_handles = h
        self.by_uid = {}
        self.n_slots = KW["buckets"] * KW["pod_slots_per_bucket"]

    def close(self):
        self.o.close()
        self.codec.close()

    def register(self, s):
        if s not in self.spec_id:
            self.spec_id[s] = self.o.register_pod_spec([tuple(x) for x in s[0]], [tuple(x) for x in s[1]], list(s[2]))
        return self.spec_id[s]

    def expect(self, b):
        """-> (handles the caller sends, handles, statuses, released addresses, the host codec's statuses)
        of the batch, by document; the map follows"""
        lines = b.lines
        n = len(lines)
        dec = self.codec.decode_pods([l.doc for l in lines], strict=False)
        sent = np.array([self.by_uid.get(l.uid, -1) for l in lines], np.int32)
        hs, st, rel = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint32)
        recs = np.zeros(n, abi.POD_EVENT_DTYPE)
        keep = []
        for k, l in enumerate(lines):
            if dec.status[k] != abi.OK:
                st[k] = dec.status[k]
                continue
            d = dec.pods[k]
            recs[k] = np.frombuffer(bytes(d.ev), abi.POD_EVENT_DTYPE)[0]
            recs[k]["op"] = abi.OP_DELETE if l.type == "DELETED" else abi.OP_UPSERT
            recs[k]["handle"] = sent[k]
            recs[k]["node_handle"] = -1
            if l.type != "DELETED":
                s = (tuple((dec.text(c.name), dec.text(c.image)) for c in d.containers[:d.n_containers]),
                     tuple((dec.text(c.name), dec.text(c.image)) for c in d.init_containers[:d.n_init_containers]),
                     tuple(dec.text(g) for g in d.readiness_gates[:d.n_readiness_gates]))
                assert s == l.spec, (b.name, k)
                try:
                    recs[k]["spec_id"] = self.register(s)
                except KwokError as err:
                    st[k] = err.code
                    continue
            keep.append(k)
        if keep:
            h, s, r = self.o.ingest_pods_raw(recs[keep], bytes(dec.buf))
            hs[keep], st[keep], rel[keep] = h, s, r
        for k, l in enumerate(lines):
            if st[k] == abi.OK and l.type == "DELETED":
                self.by_uid.pop(l.uid, None)
            elif st[k] == abi.OK:
                self.by_uid[l.uid] = int(hs[k])
        return sent, hs, st, rel, list(dec.status)
