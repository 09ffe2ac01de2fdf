"""Test infrastructure for the response framer (include/kwok_watch.h): the
named bodies both framers are run over, the two oracles of the host framer - the watch
framer over the same object in a MODIFIED envelope, and a Python restatement of the rules
for what the envelope cannot express - the count of documents with an escaped routed key,
and a clientset that answers the engine's own patches with raw bytes."""
import json

import numpy as np

import harness
import watch_frames as wf
from kwok_amd import abi
from kwok_amd.codec import frame_watch

WS = b" \t\r\n"
PREFIX = b'{"type":"MODIFIED","object":'
SPAN_KEYS = ("uid", "resource_version", "name", "namespace_")
_dec = json.JSONDecoder()


def golden_docs():
    """the pod and node documents of the golden traces, each with a uid and a resourceVersion"""
    docs = []
    for name in harness.TRACES:
        for t in harness.load_trace(name)["ticks"]:
            docs += [harness.pod_doc(ev) for ev in t["pod_events"]]
            docs += [harness.node_doc(ev) for ev in t["node_events"] if ev["op"] != "delete"]
    for k, d in enumerate(docs):
        d["metadata"].setdefault("uid", "u-" + d["metadata"]["name"])
        d["metadata"]["resourceVersion"] = str(1000 + k)
    return docs


def compact(d):
    return json.dumps(d, separators=(",", ":")).encode()


def _nest(n):
    """a body whose containers nest n deep (the root object is 1)"""
    return b'{"a":' + b"[" * (n - 1) + b"]" * (n - 1) + b"}"


# what a case is checked against: W the envelope oracle, P the Python oracle
W, P = 1, 2


def cases():
    """[(name, body, documents the device lists for the host framer, oracles)]"""
    docs = golden_docs()
    pod = next(d for d in docs if d["kind"] == "Pod")
    node = next(d for d in docs if d["kind"] == "Node")
    md = pod["metadata"]
    c = []
    for k, d in enumerate(docs[:24]):
        c.append(("golden_%d" % k, compact(d), 0, W | P))
    c.append(("pod", compact(pod), 0, W | P))
    c.append(("node", compact(node), 0, W | P))
    c.append(("spaces_and_newline", b"  \t" + compact(pod) + b"\n", 0, W | P))
    c.append(("crlf_tail", compact(node) + b" \r\n", 0, W | P))
    c.append(("pretty", json.dumps(pod, indent=2).encode() + b"\n", 0, W | P))
    c.append(("pretty_node", json.dumps(node, indent=1).encode(), 0, W | P))
    c.append(("metadata_missing", b'{"kind":"Pod","spec":{"nodeName":"n"},"status":{}}', 0, W | P))
    c.append(("metadata_array", b'{"metadata":["uid"],"spec":{}}', 0, W | P))
    c.append(("metadata_null", b'{"metadata":null}', 0, W | P))
    c.append(("metadata_string", b'{"metadata":"uid","kind":"Pod"}', 0, W | P))
    c.append(("uid_number", b'{"metadata":{"uid":7,"resourceVersion":"12","name":"p","namespace":null}}', 0, W | P))
    c.append(("uid_empty", b'{"metadata":{"uid":"","resourceVersion":"","name":"p"}}', 0, W | P))
    c.append(("duplicate_metadata", b'{"metadata":{"name":"first","uid":"u1"},"metadata":{"name":"third","uid":"u3","resourceVersion":"9"}}',
              0, W | P))
    c.append(("duplicate_metadata_scalar_first", b'{"metadata":1,"metadata":{"name":"second","uid":"u"}}', 0, W | P))
    c.append(("duplicate_uid", b'{"metadata":{"uid":"first","uid":"second","name":"a","name":"b"}}', 0, W | P))
    c.append(("deeper_metadata_only", b'{"kind":"Deployment","spec":{"template":{"metadata":{"uid":"inner","name":"t"}}}}', 0, W | P))
    c.append(("deeper_metadata_too", b'{"spec":{"template":{"metadata":{"uid":"inner","name":"t"}}},"metadata":{"uid":"outer"}}',
              0, W | P))
    c.append(("metadata_in_array", b'{"items":[{"metadata":{"uid":"no"}}],"metadata":{"name":"yes"}}', 0, W | P))
    esc = dict(pod, metadata=dict(md, uid="u\\-\"q\"", name="café", namespace="d"))
    c.append(("escaped_uid_name", json.dumps(esc, separators=(",", ":")).encode(), 0, W | P))
    c.append(("escaped_rv_ns", b'{"metadata":{"resourceVersion":"4\\u0031","namespace":"a\\/b","uid":"u","name":"n"}}', 0, W | P))
    c.append(("escaped_key_metadata", b'{"met\\u0061data":{"uid":"u"}}', 1, W | P))
    c.append(("escaped_key_uid", b'{"metadata":{"u\\u0069d":"u","n\\u0061me":"n"}}', 1, W | P))
    c.append(("escaped_key_root", b'{"metadata":{"labels":{"\\u0061":"b"}},"sp\\u0065c":{}}', 1, W | P))
    c.append(("escaped_key_unrouted", b'{"metadata":{"labels":{"\\u0061":"b"},"uid":"u"},"spec":{"\\u0061":1}}', 0, W | P))
    c.append(("status_error", compact({"kind": "Status", "apiVersion": "v1", "metadata": {}, "status": "Failure",
                                       "message": 'pods "pod-0" not found', "reason": "NotFound",
                                       "details": {"name": "pod-0", "kind": "pods"}, "code": 404}) + b"\n", 0, W | P))
    c.append(("empty_object", b"{}", 0, W | P))
    for k, bad in enumerate([b"[]", b"null", b'"x"', b"17", b'[{"metadata":{"uid":"u"}}]', compact(pod)[:-7],
                             compact(pod)[:40], b"{}{}", compact(pod) + b" x", compact(pod) + compact(pod), b'{"a":1,}',
                             b"{", b"}"]):
        c.append(("invalid_%d" % k, bad, 0, W | P))
    c.append(("truncated_escaped_key", b'{"met\\u0061data":{"uid":"u"}', 0, W | P))  # malformed first: never listed
    c.append(("empty", b"", 0, P))
    c.append(("whitespace", b" \t\r\n \n", 0, P))
    c.append(("depth_65", _nest(65), 0, P))   # (one level more than a watch line's object may hold)
    c.append(("depth_66", _nest(66), 0, P))
    c.append(("depth_64", _nest(64), 0, W | P))
    return c


def pack(bodies, gap=b"#", pad_to=None):
    """the bodies in one buffer with `gap` between them (bytes no span covers): (buf, offs, lens).
    pad_to = (m, r): the gap before the last body is stretched so that len(buf) % m == r; the
    last body ends exactly at len(buf)"""
    parts, offs, lens, at = [], [], [], 0
    for k, b in enumerate(bodies):
        g = gap if k else b""
        if pad_to and k == len(bodies) - 1:
            m, r = pad_to
            g = g + b"#" * ((r - (at + len(g) + len(b))) % m)
        parts += [g, b]
        at += len(g)
        offs.append(at)
        lens.append(len(b))
        at += len(b)
    return b"".join(parts), np.array(offs, np.uint64), np.array(lens, np.uint32)


def zero_frame(status=abi.OK, line_off=0):
    return dict(line_off=line_off, doc_off=0, doc_len=0, type=abi.WATCH_NONE, flags=0, status=status,
                uid=(0, 0), resource_version=(0, 0), name=(0, 0), namespace_=(0, 0))


def envelope_frame(buf, off, dlen):
    """oracle 1: the body in a MODIFIED envelope through kwok_frame_watch, rebased to the body.  A body's
    newlines (whitespace outside strings in every case it is used for) become spaces: the same offsets"""
    body = bytes(buf[off:off + dlen]).replace(b"\n", b" ")
    frames, used = frame_watch(PREFIX + body + b"}\n")
    assert len(frames) == 1 and used == len(PREFIX) + len(body) + 2
    w = wf.as_dict(frames[0])
    f = zero_frame(w["status"], off)
    if w["status"] != abi.OK:
        return f
    assert w["type"] == abi.WATCH_MODIFIED
    shift = off - len(PREFIX)
    f.update(type=abi.WATCH_MODIFIED, flags=w["flags"], doc_off=w["doc_off"] + shift, doc_len=w["doc_len"])
    for k in SPAN_KEYS:
        if w[k][1]:
            f[k] = (w[k][0] + shift, w[k][1])
    return f


def members_raw(text, i):
    """the members of the object whose '{' is text[i]: (raw key text inside its quotes, value start, value end)"""
    out = []
    i += 1
    while True:
        while text[i] in " \t\r\n":
            i += 1
        if text[i] == "}":
            return out
        _, e = _dec.raw_decode(text, i)
        raw = text[i + 1:e - 1]
        i = e
        while text[i] in " \t\r\n":
            i += 1
        assert text[i] == ":"
        i += 1
        while text[i] in " \t\r\n":
            i += 1
        _, end = _dec.raw_decode(text, i)
        out.append((raw, i, end))
        i = end
        while text[i] in " \t\r\n":
            i += 1
        if text[i] == ",":
            i += 1


def _parse(body):
    """the body's text if it is one JSON object within the depth limit, else None"""
    try:
        text = body.decode()
        root = json.loads(text)
    except (ValueError, RecursionError):
        return None
    if not isinstance(root, dict) or wf._depth(text) > 65:
        return None
    return text


def python_frame(buf, off, dlen):
    """oracle 2: the rules of kwok_watch.h restated with json (ASCII bodies: byte offsets are character offsets)"""
    if off > len(buf) or dlen > len(buf) - off:
        return zero_frame(abi.EINVAL)
    f = zero_frame(abi.OK, off)
    body = bytes(buf[off:off + dlen])
    if not body.strip(WS):
        return f
    f["status"] = abi.EINVAL
    text = _parse(body)
    if text is None:
        return f
    assert len(text) == len(body)
    lo = text.index("{")
    f.update(status=abi.OK, type=abi.WATCH_MODIFIED, doc_off=off + lo, doc_len=len(text.rstrip(" \t\r\n")) - lo)
    md = wf._first(wf._members(text, lo), "metadata")
    if md is None or text[md[0]] != "{":
        return f
    mm = wf._members(text, md[0])
    for key, field, bit in wf.META_KEYS:
        v = wf._first(mm, key)
        if v is None or text[v[0]] != '"':
            continue
        raw = text[v[0] + 1:v[1] - 1]
        if raw:
            f[field] = (off + v[0] + 1, len(raw))
        if "\\" in raw:
            f["flags"] |= bit
    return f


def escaped_routed_key(body):
    """True when a valid body spells a key the scan routes on with an escape: any key of the root, any key of
    the root's first `metadata` when that is an object (the device lists exactly these for the host framer)"""
    text = _parse(bytes(body))
    if text is None:
        return False
    top = members_raw(text, text.index("{"))
    if any("\\" in k for k, _a, _b in top):
        return True
    md = next(((a, b) for k, a, b in top if k == "metadata"), None)
    if md is None or text[md[0]] != "{":
        return False
    return any("\\" in k for k, _a, _b in members_raw(text, md[0]))


class RawClientset:
    """a clientset that also answers the engine's own patches with the response BODY (client-go:
    Patch(...).Do(ctx).Raw()), around tests/fake_clientset.FakeClientset: patch_*_raw return the patched
    object as the bytes an apiserver writes (compact JSON and a newline).  mangle(obj) -> bytes or None lets a
    test spell one response differently (the same object)."""

    def __init__(self, inner, mangle=None):
        self.inner = inner
        self.mangle = mangle
        self.raw_calls = 0

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def _raw(self, obj):
        self.raw_calls += 1
        body = self.mangle(obj) if self.mangle else None
        return body if body is not None else compact(obj) + b"\n"

    def patch_node_status_raw(self, name, body):
        return self._raw(self.inner.patch_node_status(name, body))

    def patch_pod_status_raw(self, ns, name, body):
        return self._raw(self.inner.patch_pod_status(ns, name, body))

    def patch_pod_raw(self, ns, name, body):
        return self._raw(self.inner.patch_pod(ns, name, body))
