"""GPU: the node status blob canonicaliser (include/kwok_canon.h; json.hip k_json_nodes_canon,
k_canon_len, k_canon) against the host codec path it replaces.  With kwok_canon_enable every output of the
device node decodes is what the host codec gives - statuses, record bytes, the arena kwok_decode_nodes_gpu
returns, handles and the following tick - and the documents whose blobs are inside the device domain are
decoded with no host codec call (n_host counts only the others).

The expected host count of every case comes from verdict() below: the device domain restated in Python over the
document's own bytes (never from what the engine answers).  A blob is clean when it holds no backslash, no
`<` `>` `&`, no byte >= 0x80, only plain integers as numbers, no duplicate key, at most CANON_MAX_MEMBERS
members per object, and nests no deeper than the kernel's shapes: addresses a list of scalars and of objects
of scalars, allocatable / capacity objects of scalars."""
import json
import os
import random
import re

import numpy as np
import pytest

import harness
import watch_frames as wf
from harness import DISREGARD, MANAGE, node_doc, pod_doc
from kwok_amd import abi
from kwok_amd.codec import Codec
from kwok_amd.engine import Engine, make_config
from test_codec import scramble
from test_json_nodes_gpu import SELECTORS, compare, golden_node_docs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "kwok_amd", "csrc", "json.hip")).read()
BOUND = int(re.search(r"CANON_MAX_MEMBERS = (\d+)", _SRC).group(1))
DEPTH = int(re.search(r"CANON_MAX_DEPTH = (\d+)", _SRC).group(1))
BLOBS = ("addresses", "allocatable", "capacity")
KW = dict(buckets=64, node_slots_per_bucket=16, pod_slots_per_bucket=128)
T0 = 1704067230


def compare_ticks(a, b, where):
    """every output of two engines' ticks (gpu_common.compare takes an oracle's layout on its right)"""
    assert list(a.heartbeat_nodes) == list(b.heartbeat_nodes), where + " heartbeat handles"
    assert [a.heartbeat_body(i) for i in range(len(a.heartbeat_nodes))] == \
           [b.heartbeat_body(i) for i in range(len(b.heartbeat_nodes))], where + " heartbeat bytes"
    assert a.node_inits == b.node_inits, where + " node inits"
    assert a.pod_patches == b.pod_patches, where + " pod patches"
    assert a.deletes == b.deletes, where + " deletes"
    assert a.counters == b.counters and a.local_counters == b.local_counters, where + " counters"


# ---- the device domain, restated ----
class _Obj(list):
    pass


class _Int(str):
    pass


class _Float(str):
    pass


def _scalar(v):
    return v is None or v is True or v is False or isinstance(v, _Int) or (isinstance(v, str) and not isinstance(v, _Float))


def _flat_obj(v):
    keys = [k for k, _x in v]
    return len(keys) <= BOUND and len(set(keys)) == len(keys) and all(_scalar(x) for _k, x in v)


def blob_clean(raw, is_list):
    """raw: the bytes of a non-empty blob value"""
    if any(c >= 0x80 or c in b"\\<>&" for c in raw):
        return False
    v = json.loads(raw.decode(), object_pairs_hook=_Obj, parse_int=_Int, parse_float=_Float)
    assert DEPTH == 2  # (the shapes below are the kernel's: the blob's container and, in the list, one more)
    if is_list:
        return all(_scalar(x) or (isinstance(x, _Obj) and _flat_obj(x)) for x in v)
    return _flat_obj(v)


def blob_values(doc):
    """the raw bytes of the first status.addresses / allocatable / capacity of a decodable document that are
    non-empty containers of the right kind"""
    text = doc.decode("latin-1")
    out = []
    st = wf._first(wf._members(text, text.index("{")), "status")
    if st is None or text[st[0]] != "{":
        return out
    mm = wf._members(text, st[0])
    for k, key in enumerate(BLOBS):
        v = wf._first(mm, key)
        if v is None or text[v[0]] != ("[" if k == 0 else "{"):
            continue
        raw = doc[v[0]:v[1]]
        if len(json.loads(raw.decode("latin-1"))):
            out.append((k, raw))
    return out


def verdict(doc):
    """'none': no non-empty blob; 'clean': the device canonicalises the document; 'host': a blob is outside its domain"""
    bl = blob_values(doc)
    if not bl:
        return "none"
    return "clean" if all(blob_clean(raw, k == 0) for k, raw in bl) else "host"


def counts(docs):
    v = [verdict(d) for d in docs]
    return v.count("clean"), v.count("host")


@pytest.fixture(scope="module")
def eng():
    e = Engine(make_config(**KW))
    e.canon_enable()
    yield e
    e.close()


def checked(eng, codec, docs, where, errors=0):
    """compare() with the restated host count; the stats move by the restated counts (errors: documents with a
    blob whose decode fails elsewhere - on no list)"""
    clean, host = counts(docs)
    before = eng.canon_stats()
    compare(eng, codec, docs, want_host=host, where=where)
    after = eng.canon_stats()
    assert after["docs"] - before["docs"] == clean - errors, (where, before, after)
    assert after["docs_host"] - before["docs_host"] == host, (where, before, after)
    assert after["calls"] - before["calls"] == (1 if clean + host - errors else 0), (where, before, after)
    return clean, host


# ---- 1. the golden documents: no host codec call ----
@pytest.mark.parametrize("sel", range(len(SELECTORS)))
def test_golden_documents_need_no_host_decode(eng, sel):
    """fails without the feature: at the parent every document with a blob is listed for the host"""
    rng = random.Random(11)
    canon, scr = golden_node_docs(rng)
    codec = Codec(**SELECTORS[sel])
    with_blob = 0
    for docs, where in ((canon, "compact"), (scr, "scrambled")):
        clean, host = checked(eng, codec, docs, where)
        assert host == 0, "golden documents outside the device domain: %d" % host  # (every golden blob is clean)
        with_blob += clean
        st = eng.canon_stats()
        assert st["bytes_out"] <= st["bytes_in"] and st["blobs"] >= st["docs"]
    assert with_blob > 0
    eng.canon_enable(True)  # idempotent
    codec.close()


# ---- 2. the domain's edges ----
def node(status, name="node-1", **md):
    meta = {"name": name, "annotations": {"kwok.x-k8s.io/node": "fake"}, "labels": {"type": "kwok"}}
    meta.update(md)
    return {"metadata": meta, "status": status}


def dumps(d, **kw):
    return json.dumps(d, separators=(",", ":"), **kw).encode()


def spaced(d):
    """whitespace before and after every token"""
    s = json.dumps(d, separators=(",", ":"))
    out, in_str, esc = [], False, False
    for ch in s:
        if in_str:
            out.append(ch)
            if esc:
                esc = False
            elif ch == "\\":
                esc = True
            elif ch == '"':
                in_str = False
                out.append(" \t")
        elif ch == '"':
            in_str = True
            out.append("\r\n " + ch)
        elif ch in "{}[],:":
            out.append(" \n" + ch + "\t ")
        else:
            out.append(ch)
    return "".join(out).encode()


def edge_cases():
    """(name, document, documents with a blob that fail elsewhere)"""
    c = []
    keys = lambda n: ["k%02d" % i for i in range(n)]  # noqa: E731
    for n in (1, 2, BOUND - 1, BOUND, BOUND + 1):
        ks = keys(n)
        for order, kk in (("sorted", ks), ("reversed", ks[::-1]), ("rotated", ks[n // 2:] + ks[:n // 2])):
            c.append(("%d members %s" % (n, order), dumps(node({"allocatable": {k: str(i) for i, k in enumerate(kk)},
                                                                     "capacity": {k: i for i, k in enumerate(kk)}}))))
    c.append(("prefix keys", dumps(node({"capacity": {"cpu2": "b", "cpu": "a", "cp": "c", "cpu20": "d", "c": "e"}}))))
    for ln in (15, 16, 17, 31, 32, 33):
        stem = "x" * (ln - 1)
        for pad in (0, 7):  # (the keys at two positions of the reader's 16-byte window)
            c.append(("keys of %d bytes, pad %d" % (ln, pad),
                      dumps(node({"allocatable": {stem + "b": "1", stem + "a": "2", stem: "3", stem + "c": 4}}, name="n" * (pad + 1)))))
    c.append(("duplicate key", b'{"metadata":{"name":"d1"},"status":{"capacity":{"cpu":"1","pods":"2","cpu":"3"}}}'))
    c.append(("duplicate key in an address", b'{"metadata":{"name":"d2"},"status":{"addresses":[{"type":"a","type":"a"}]}}'))
    c.append(("empty key", dumps(node({"allocatable": {"b": "1", "": "0", "a": "2"}}))))
    c.append(("two empty keys", b'{"metadata":{"name":"d3"},"status":{"allocatable":{"":"0","":"1"}}}'))
    for name, raw in (("string 0", b'"0"'), ("minus zero", b"-0"), ("minus seven", b"-7"), ("zero", b"0"), ("float", b"1.5"),
                      ("exponent", b"1e3"), ("true", b"true"), ("false", b"false"), ("null", b"null"), ("empty string", b'""'),
                      ("nested object", b'{"a":1}'), ("nested list", b"[1]"), ("nested empty object", b"{}")):
        c.append(("value " + name, b'{"metadata":{"name":"v1"},"status":{"capacity":{"pods":"1","x":' + raw + b',"a":"z"}}}'))
        c.append(("address field " + name, b'{"metadata":{"name":"v2"},"status":{"addresses":[{"type":"T","address":' + raw + b"}]}}"))
    c.append(("object two levels into the list", b'{"metadata":{"name":"v3"},"status":{"addresses":[{"type":{"a":{"b":1}}}]}}'))
    c.append(("list in the list", b'{"metadata":{"name":"v4"},"status":{"addresses":[[{"type":"a"}]]}}'))
    for n in (1, 2, 5):  # struct order, as the apiserver writes them
        c.append(("%d addresses in struct order" % n, dumps(node({"addresses": [
            {"type": "InternalIP" if i % 2 == 0 else "Hostname", "address": "10.0.%d.%d" % (n, i)} for i in range(n)]}))))
    c.append(("scalar address", dumps(node({"addresses": ["10.0.0.1", 7, None, True, {"type": "x", "address": "y"}, "z"]}))))
    c.append(("float address", dumps(node({"addresses": [{"type": "x", "address": "y"}, 1.5]}))))
    for what, ch in (("lt", b"<"), ("gt", b">"), ("amp", b"&"), ("high byte", b"\xc3\xa9"), ("u escape", b"\\u0041"), ("slash escape", b"\\/")):
        c.append((what + " in a key", b'{"metadata":{"name":"x1"},"status":{"allocatable":{"cpu":"4","a' + ch + b'b":"1"}}}'))
        c.append((what + " in a value", b'{"metadata":{"name":"x2"},"status":{"allocatable":{"cpu":"4","ab":"1' + ch + b'"}}}'))
        c.append((what + " in an address", b'{"metadata":{"name":"x3"},"status":{"addresses":[{"type":"T' + ch + b'","address":"a"}]}}'))
    c.append(("an escaped key alone", b'{"metadata":{"name":"x4"},"status":{"capacity":{"\\u0041":"1"}}}'))
    full = node({"phase": "Running", "addresses": [{"type": "InternalIP", "address": "10.1.2.3"}, {"type": "Hostname", "address": "h"}],
                 "allocatable": {"pods": "110", "cpu": "4", "memory": "1Gi"}, "capacity": {"pods": 110, "cpu": "8"},
                 "nodeInfo": {"kubeletVersion": "fake", "osImage": "x"}})
    for ind in (1, 2, 4, "\t"):
        c.append(("indented %r" % ind, json.dumps(full, indent=ind).encode()))
    c.append(("spaced", spaced(full)))
    c.append(("blob last", b'{"metadata":{"name":"l1"},"status":{"phase":"Running","capacity":{"b":"1","a":"2"}}}'))
    c.append(("blob last, spaces", b'{"metadata":{"name":"l2"},"status":{"capacity":{"b":"1","a":"2"} } } '))
    c.append(("status first", b'{"status":{"allocatable":{"b":"1","a":"2"}},"metadata":{"name":"l3"}}'))
    c.append(("clean and unclean", dumps(node({"allocatable": {"b": "1", "a": "2"}, "capacity": {"pods": 1.5, "a": "1"}}))))
    c.append(("unclean and clean", dumps(node({"addresses": [{"type": "a<b"}], "capacity": {"z": "1", "a": "1"}}))))
    c.append(("clean, clean, unclean", dumps(node({"addresses": [{"type": "b", "address": "a"}], "allocatable": {"b": "1", "a": "2"},
                                                   "capacity": {"b": {"c": 1}}}))))
    c.append(("repeated addresses", b'{"metadata":{"name":"r1"},"status":{"addresses":[{"type":"b","address":"a"}],'
                                    b'"addresses":[{"type":"<"}],"capacity":{"b":"1","a":"2"},"capacity":{"x":1.5}}}'))
    c.append(("repeated addresses, unclean first", b'{"metadata":{"name":"r2"},"status":{"addresses":[{"type":"<"}],'
                                                   b'"addresses":[{"type":"b","address":"a"}]}}'))
    c.append(("empty, null and clean", dumps(node({"addresses": [], "allocatable": None, "capacity": {"b": "1", "a": "2"}}))))
    c = [(n, d, 0) for n, d in c]
    # a clean blob beside a nodeInfo wrong-type error: KWOK_EDOMAIN, nothing written, nothing listed
    c.append(("clean blob, nodeInfo error", dumps(node({"allocatable": {"b": "1", "a": "2"}, "nodeInfo": {"architecture": 1}})), 1))
    c.append(("clean blob, wrong-type blob", dumps(node({"allocatable": {"b": "1", "a": "2"}, "capacity": [1]})), 1))
    c.append(("clean blob, no name", b'{"metadata":{},"status":{"allocatable":{"b":"1","a":"2"}}}', 1))
    return c


def test_domain_edges(eng):
    cases = edge_cases()
    assert len(set(n for n, _d, _e in cases)) == len(cases)
    codec = Codec(**SELECTORS[1])
    seen = set()
    for name, doc, errors in cases:
        clean, host = checked(eng, codec, [doc], name, errors)
        seen.add("host" if host else "clean" if clean else "none")
    assert seen == {"host", "clean"}
    # what the restatement says of a few of them, spelled out
    want = {"%d members sorted" % BOUND: "clean", "%d members reversed" % (BOUND + 1): "host", "duplicate key": "host",
            "empty key": "clean", "value minus zero": "clean", "value float": "host", "value exponent": "host",
            "value nested object": "host", "value nested empty object": "host", "scalar address": "clean",
            "u escape in a key": "host", "slash escape in a value": "host", "high byte in a value": "host", "spaced": "clean",
            "clean and unclean": "host", "repeated addresses": "clean", "repeated addresses, unclean first": "host",
            "an escaped key alone": "host", "list in the list": "host", "object two levels into the list": "host"}
    by_name = {n: d for n, d, _e in cases}
    for n, v in want.items():
        assert verdict(by_name[n]) == v, n
    # all of them in one call, under every selector
    docs = [d for _n, d, _e in cases]
    for sel in SELECTORS:
        c2 = Codec(**sel)
        checked(eng, c2, docs, "all cases %r" % sel, errors=sum(e for _n, _d, e in cases))
        c2.close()
    codec.close()


def test_mutated_golden_documents(eng):
    """400 byte-flipped and truncated golden documents, mutated as tests/test_json_nodes_gpu.py mutates them"""
    rng = random.Random(3)
    canon, scr = golden_node_docs(rng)
    # every golden document, compact and scrambled, once; the ones that hold a blob again until there are 200
    src = canon + scr
    blob = [d for d in src if verdict(d) != "none"]
    src += [blob[k % len(blob)] for k in range(200 - len(src))]
    mut = []
    for d in src:
        b = bytearray(d)
        i = rng.randrange(len(b))
        b[i] = rng.choice(b'{}[]",:\\ 0a')
        mut.append(bytes(b))
        mut.append(d[:rng.randrange(1, len(d))])
    assert len(mut) == 400
    for sel in SELECTORS[:2]:
        codec = Codec(**sel)
        compare(eng, codec, mut, where="mutated")
        codec.close()


# ---- 3. launch edges ----
def mixed_docs(n, rng):
    """zero-status, clean-blob and host-listed documents"""
    docs = []
    for i in range(n):
        r = i % 4
        if r == 0:
            st = {"nodeInfo": {"kubeletVersion": "fake"}}
        elif r == 1:
            st = {"addresses": [{"type": "InternalIP", "address": "10.%d.%d.%d" % (i >> 16, (i >> 8) & 255, i & 255)}],
                  "allocatable": {"pods": "110", "cpu": str(i)}, "capacity": {"memory": "%dGi" % i, "cpu": i}}
        elif r == 2:
            st = {"capacity": {"pods": "1%d" % i, "cpu": 1.5}}  # a float: the host decides
        else:
            st = {"allocatable": {"b" * (i % 40 + 1): "1", "a": "2"}}
        d = node(st, name="mx-%d" % i)
        docs.append(scramble(d, rng) if i % 3 == 0 else dumps(d))
    return docs


def test_launch_edges(eng):
    rng = random.Random(5)
    codec = Codec(**SELECTORS[1])
    for n in (1, 63, 64, 65, 257):
        checked(eng, codec, mixed_docs(n, rng), "%d documents" % n)
    # arenas of len % 16 in {0, 1, 15}: the last document's blob is the arena's last value
    for rem in (0, 1, 15):
        docs = mixed_docs(9, rng)
        tail = b'{"metadata":{"name":"t"},"status":{"capacity":{"b":"1","a":"'
        total = sum(len(d) for d in docs) + len(tail) + 4
        fill = (rem - total) % 16
        docs.append(tail + b"x" * fill + b'"}}}')
        assert sum(len(d) for d in docs) % 16 == rem
        checked(eng, codec, docs, "arena %% 16 == %d" % rem)
    # no blob document: the canon kernels are not launched
    before = eng.canon_stats()
    zero = [dumps(node({"nodeInfo": {"osImage": "x"}}, name="z-%d" % i)) for i in range(70)]
    compare(eng, codec, zero, want_host=0, where="no blob")
    assert eng.canon_stats() == before
    codec.close()


# ---- 4. the ingest entries ----
def fleet_docs(rng, n=70):
    """non-conforming statuses (no phase): every node's init patch carries its canonical blobs; a few host-listed and
    zero-status documents among them"""
    docs = []
    for i in range(n):
        st = {"addresses": [{"type": "InternalIP", "address": "10.9.%d.%d" % (i // 200, i % 200)}, {"type": "Hostname", "address": "cn-%d" % i}],
              "allocatable": {"pods": "110", "cpu": str(i % 7 + 1), "memory": "%dGi" % (i % 5 + 1)},
              "capacity": {"pods": 110, "cpu": str(i % 7 + 2)},
              "nodeInfo": {"kubeletVersion": "fake", "architecture": "amd64"}}
        if i % 10 == 3:
            st["capacity"]["note"] = "café"   # (json.dumps writes a \u escape: the host decides, and decodes it)
        if i % 10 == 7:
            st = {}
        d = node(st, name="cn-%d" % i)
        d["metadata"]["uid"] = "uid-cn-%d" % i
        d["metadata"]["resourceVersion"] = "5"
        docs.append(scramble(d, rng))
    return docs


def one_line(doc):
    """the document without newlines (a dict keeps the document's key order: the scrambled order survives)"""
    return json.dumps(json.loads(doc), separators=(", ", ": ")).encode()


def host_records(codec, docs):
    dec = codec.decode_nodes(docs, strict=False)
    assert not any(dec.status)
    recs = np.zeros(len(docs), abi.NODE_EVENT_DTYPE)
    for q in range(len(docs)):
        recs[q] = np.frombuffer(bytes(dec.nodes[q]), abi.NODE_EVENT_DTYPE)[0]
        recs[q]["op"] = abi.OP_UPSERT
    return recs, bytes(dec.buf)


ENTRIES = ["json", "watch", "list", "echo"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_ingest_entries_equal_the_host_records(entry):
    rng = random.Random(17)
    docs = [one_line(d) for d in fleet_docs(rng)]  # (a watch line holds no newline; the key order stays scrambled)
    codec = Codec(**SELECTORS[1])
    clean, host = counts(docs)
    assert clean > 40 and host > 3
    a, b = Engine(make_config(**KW)), Engine(make_config(**KW))
    a.canon_enable()
    if entry == "echo":
        a.uid_dir_enable(), a.echo_enable(), a.refs_enable(), a.node_dir_enable()
    idx = np.arange(len(docs))

    def feed():
        if entry == "json":
            arena, offs, lens = Engine._docs(docs)
            return a.ingest_nodes_json(codec, arena, offs, lens, np.full(len(docs), abi.OP_UPSERT, np.uint8))
        if entry == "list":
            body = b'{"kind":"NodeList","apiVersion":"v1","metadata":{"resourceVersion":"7"},"items":[' + b",".join(docs) + b"]}"
            frames, _info, _nh, sid = a.frame_list(body)
        else:
            frames, _used, _nh, sid = a.frame_watch(b"".join(wf.wrap(d, "ADDED") for d in docs))
        assert len(frames) == len(docs) and not frames["status"].any()
        out = []
        for _round in range(2):  # the same frames again: the resident stream was not rewritten
            if entry == "echo":
                h, s, nh, ne = a.ingest_nodes_framed_echo(codec, sid, idx)
                assert ne == 0
            else:
                h, s, nh = a.ingest_nodes_framed(codec, sid, idx)
            out.append((list(h), list(s), nh))
        assert out[0] == out[1], "the second ingest of the same frames differs"
        return out[1]

    before = a.canon_stats()
    ha, sa, nh = feed()
    recs, arena = host_records(codec, docs)
    hb, sb = b.ingest_nodes_raw(recs, arena)
    assert list(sa) == list(sb) == [0] * len(docs) and list(ha) == list(hb)
    assert nh == host, "documents the host codec decoded: %d, restated %d" % (nh, host)
    rounds = 1 if entry == "json" else 2
    after = a.canon_stats()
    assert after["docs"] - before["docs"] == rounds * clean and after["docs_host"] - before["docs_host"] == rounds * host
    assert b.canon_stats() == dict.fromkeys(abi.CANON_STATS, 0)
    for k in range(2):
        oa, ob = a.tick(T0 + 30 * k), b.tick(T0 + 30 * k)
        compare_ticks(oa, ob, "%s tick %d" % (entry, k))
        if k == 0:
            assert len(oa.node_inits) >= clean + host  # (no status conforms: every such node is patched, blobs and all)
            assert any(b'"allocatable":{"cpu":"3","memory":' in body for _h, body in oa.node_inits)
    codec.close()
    a.close()
    b.close()


def _op(ev):
    return abi.OP_DELETE if ev["op"] == "delete" else abi.OP_UPSERT


@pytest.mark.parametrize("name", harness.TRACES)
def test_golden_trace_through_both_gpu_codecs_with_canon(name):
    """tests/test_json_nodes_gpu.py's replay with the feature on: the golden fixtures, and no node document left to
    the host codec"""
    fx = harness.load_trace(name)
    e = Engine(harness.config_for(fx))
    e.canon_enable()
    codec = Codec(manage_all_nodes=False, manage_nodes_with_annotation_selector=MANAGE,
                  disregard_status_with_annotation_selector=DISREGARD)
    last = {}
    for ti, t in enumerate(fx["ticks"]):
        nev = t["node_events"]
        if nev:
            docs = []
            for ev in nev:
                if ev["op"] == "delete":
                    d = last.get(ev["name"]) or {"metadata": {"name": ev["name"]}}
                else:
                    d = last[ev["name"]] = node_doc(ev)
                docs.append(json.dumps(d).encode())
            arena, offs, lens = Engine._docs(docs)
            hs, st, nh = e.ingest_nodes_json(codec, arena, offs, lens, np.array([_op(x) for x in nev], np.uint8))
            assert list(st) == [0] * len(st), (ti, list(st))
            want = sum(1 for ev, d in zip(nev, docs) if ev["op"] != "delete" and verdict(d) == "host")
            assert nh == want == 0, (ti, nh, want)
        evs = t["pod_events"]
        if evs:
            arena, offs, lens = Engine._docs([pod_doc(ev) for ev in evs])
            ops = np.array([_op(ev) for ev in evs], np.uint8)
            handles = np.array([ev.get("handle", -1) for ev in evs], np.int32)
            hs, st, _rel, _nh = e.ingest_pods_json(codec, arena, offs, lens, ops, handles)
            assert list(st) == [0] * len(st), (ti, list(st))
            assert list(hs) == [ev["expect_handle"] for ev in evs], ti
        out = e.tick(t["now"])
        harness.compare_tick(fx["name"], ti, t["expect"], out)
    codec.close()
    e.close()


def test_custom_node_template_still_completes_on_the_host():
    """custom_node: enabling is accepted, every record still goes through the host completion; the init patches
    equal those of the engine without the feature"""
    from test_template_cpu import tpl
    rng = random.Random(23)
    docs = [one_line(d) for d in fleet_docs(rng, 24)]
    codec = Codec(**SELECTORS[1])
    outs = []
    for on in (True, False):
        e = Engine(make_config(node_init_template=tpl("node_a.tpl"), **KW))
        if on:
            e.canon_enable()
        arena, offs, lens = Engine._docs(docs)
        h, s, nh = e.ingest_nodes_json(codec, arena, offs, lens, np.full(len(docs), abi.OP_UPSERT, np.uint8))
        outs.append((list(h), list(s), e.tick(T0)))
        clean, host = counts(docs)
        assert nh == (host if on else clean + host)
        e.close()
    assert outs[0][:2] == outs[1][:2]
    compare_ticks(outs[0][2], outs[1][2], "custom node template")
    assert len(outs[0][2].node_inits) > 0
    codec.close()


# ---- 5. off is off ----
def test_off_is_off():
    rng = random.Random(29)
    docs = mixed_docs(65, rng)
    clean, host = counts(docs)
    codec = Codec(**SELECTORS[1])
    e = Engine(make_config(**KW))
    zero = dict.fromkeys(abi.CANON_STATS, 0)
    compare(e, codec, docs, want_host=clean + host, where="never enabled")  # as at the parent: every blob document
    arena, offs, lens = Engine._docs(docs)
    _h, _s, nh = e.ingest_nodes_json(codec, arena, offs, lens, np.full(len(docs), abi.OP_UPSERT, np.uint8))
    assert nh == clean + host and e.canon_stats() == zero
    e.canon_enable()
    compare(e, codec, docs, want_host=host, where="enabled")
    on = e.canon_stats()
    assert on["docs"] == clean and on["docs_host"] == host and on["calls"] == 1
    e.canon_enable(False)
    compare(e, codec, docs, want_host=clean + host, where="disabled again")
    assert e.canon_stats() == on
    codec.close()
    e.close()
