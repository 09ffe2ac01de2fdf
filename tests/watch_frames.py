"""Test infrastructure for the watch stream framer (include/kwok_watch.h): a
Python framer written from the framing rules (json.loads per line, first key
wins, depth <= 64) that the host framer is checked against, the named cases
both framers are run over, and the comparison of two frame arrays."""
import json

import numpy as np

from kwok_amd import abi

WS = b" \t\r\n"
META_KEYS = [("uid", "uid", abi.FRAME_ESC_UID), ("resourceVersion", "resource_version", abi.FRAME_ESC_RV),
             ("name", "name", abi.FRAME_ESC_NAME), ("namespace", "namespace_", abi.FRAME_ESC_NS)]
_dec = json.JSONDecoder()


def wrap(obj, typ="MODIFIED"):
    """one watch line as the apiserver writes it (compact, type first)"""
    raw = obj if isinstance(obj, (bytes, bytearray)) else json.dumps(obj, separators=(",", ":")).encode()
    return b'{"type":"%s","object":%s}\n' % (typ.encode(), raw)


def _depth(text):
    """deepest container nesting of a JSON text (the root container is depth 1)"""
    d = best = 0
    in_str = esc = False
    for ch in text:
        if in_str:
            if esc:
                esc = False
            elif ch == "\\":
                esc = True
            elif ch == '"':
                in_str = False
        elif ch == '"':
            in_str = True
        elif ch in "{[":
            d += 1
            best = max(best, d)
        elif ch in "}]":
            d -= 1
    return best


def _members(text, i):
    """the members of the object whose '{' is text[i]: (decoded key, value start, value end)"""
    out = []
    i += 1
    while True:
        while text[i] in " \t\r\n":
            i += 1
        if text[i] == "}":
            return out
        key, i = _dec.raw_decode(text, i)
        while text[i] in " \t\r\n":
            i += 1
        assert text[i] == ":"
        i += 1
        while text[i] in " \t\r\n":
            i += 1
        _, end = _dec.raw_decode(text, i)
        out.append((key, i, end))
        i = end
        while text[i] in " \t\r\n":
            i += 1
        if text[i] == ",":
            i += 1


def _first(members, key):
    for k, a, b in members:
        if k == key:
            return a, b
    return None


def py_frame(stream, lo, hi):
    """the frame of line stream[lo:hi] by the rules of kwok_watch.h, as a dict of the record's fields"""
    f = dict(line_off=lo, doc_off=0, doc_len=0, type=abi.WATCH_NONE, flags=0, status=abi.OK,
             uid=(0, 0), resource_version=(0, 0), name=(0, 0), namespace_=(0, 0))
    line = stream[lo:hi]
    if not line.strip(WS):
        return f
    f["status"] = abi.EINVAL
    try:
        text = line.decode()  # (the cases are ASCII: byte offsets are character offsets)
        assert len(text) == len(line)
        root = json.loads(text)
    except (ValueError, AssertionError, RecursionError):
        return f
    if not isinstance(root, dict) or _depth(text) > 65:  # depth <= 64 below the root value (depth 0)
        return f
    top = _members(text, text.index("{"))
    ty, ob = _first(top, "type"), _first(top, "object")
    if ty is None or ob is None:
        return f
    tv = json.loads(text[ty[0]:ty[1]])
    if not isinstance(tv, str) or tv not in abi.WATCH_TYPES or text[ob[0]] != "{":
        return f
    f.update(status=abi.OK, type=abi.WATCH_TYPES[tv], doc_off=lo + ob[0], doc_len=ob[1] - ob[0])
    md = _first(_members(text, ob[0]), "metadata")
    if md is None or text[md[0]] != "{":
        return f
    mm = _members(text, md[0])
    for key, field, bit in META_KEYS:
        v = _first(mm, key)
        if v is None or text[v[0]] != '"':
            continue
        raw = text[v[0] + 1:v[1] - 1]
        if raw:
            f[field] = (lo + v[0] + 1, len(raw))
        if "\\" in raw:
            f["flags"] |= bit
    return f


def py_frames(stream):
    """(frames as dicts, consumed) of a whole stream"""
    out, lo = [], 0
    while True:
        hi = stream.find(b"\n", lo)
        if hi < 0:
            return out, lo
        out.append(py_frame(stream, lo, hi))
        lo = hi + 1


def as_dict(rec):
    d = {k: int(rec[k]) for k in ("line_off", "doc_off", "doc_len", "type", "flags", "status")}
    for k in ("uid", "resource_version", "name", "namespace_"):
        d[k] = (int(rec[k]["off"]), int(rec[k]["len"]))
    return d


def assert_frames_equal(got, want, where=""):
    """two WATCH_FRAME_DTYPE arrays, record for record and byte for byte"""
    assert len(got) == len(want), (where, len(got), len(want))
    if got.tobytes() == want.tobytes():
        return
    for i in range(len(got)):
        assert got[i].tobytes() == want[i].tobytes(), "%s: frame %d: %r vs %r" % (where, i, as_dict(got[i]), as_dict(want[i]))


POD = {"apiVersion": "v1", "kind": "Pod",
       "metadata": {"name": "pod-0", "namespace": "default", "uid": "u-pod-0", "resourceVersion": "41",
                    "creationTimestamp": "2024-01-01T00:00:00Z", "labels": {"app": "fake"}},
       "spec": {"nodeName": "node-0", "containers": [{"name": "c", "image": "img"}]}, "status": {}}


def _nest(n):
    """a line whose containers nest n deep (the root object is 1)"""
    return b'{"type":"ADDED","object":{"a":' + b"[" * (n - 2) + b"]" * (n - 2) + b"}}\n"


def cases():
    """name -> (stream, lines the device lists for the host framer)"""
    pod = json.dumps(POD, separators=(",", ":")).encode()
    c = {}
    c["all_types"] = (b"".join(wrap(pod, t) for t in ("ADDED", "MODIFIED", "DELETED", "BOOKMARK", "ERROR")), 0)
    c["object_first"] = (b'{"object":' + pod + b',"type":"DELETED"}\n', 0)
    c["inner_whitespace"] = (b' \t{ "type" :\t"ADDED" , "object" : ' + json.dumps(POD, indent=1).replace("\n", " ").encode()
                             + b' } \r\n', 0)
    c["blank_lines"] = (b"\n" + wrap(pod) + b"\r\n \t \r\n" + wrap(pod, "ADDED")[:-1] + b"\r\n\n", 0)
    c["unterminated_tail"] = (wrap(pod) + wrap(pod, "DELETED") + wrap(pod)[:40], 0)
    c["only_tail"] = (wrap(pod)[:-1], 0)
    c["empty"] = (b"", 0)
    c["one_newline"] = (b"\n", 0)
    esc = dict(POD, metadata=dict(POD["metadata"], uid="u\\-\"q\"", name="café", namespace="d"))
    c["escaped_uid_name"] = (wrap(json.dumps(esc, separators=(",", ":")).encode(), "ADDED"), 0)  # (ensure_ascii: é)
    c["escaped_rv_ns"] = (wrap(b'{"metadata":{"resourceVersion":"4\\u0031","namespace":"a\\/b","uid":"","name":7}}'), 0)
    c["duplicate_type"] = (b'{"type":"ADDED","type":"DELETED","object":' + pod + b',"object":[1]}\n', 0)
    c["duplicate_metadata"] = (wrap(b'{"metadata":{"name":"first","name":"second"},"metadata":{"name":"third","uid":"u"}}'), 0)
    c["non_object_lines"] = (b'[1,2]\n"ADDED"\n17\nnull\n{"type":"ADDED","object":' + pod + b'} x\n{"type":"ADDED"\n', 0)
    c["unknown_type"] = (wrap(pod, "added") + wrap(pod, "PATCHED") + b'{"type":3,"object":{}}\n{"type":["ADDED"],"object":{}}\n', 0)
    c["missing_object"] = (b'{"type":"ADDED"}\n{"object":{}}\n{"type":"ADDED","Object":{}}\n', 0)
    c["object_array"] = (b'{"type":"ADDED","object":[{"metadata":{}}]}\n{"type":"ADDED","object":"x"}\n'
                         b'{"type":"ADDED","object":null}\n', 0)
    c["metadata_not_object"] = (wrap(b'{"metadata":["uid"],"spec":{"metadata":{"uid":"inner"}}}') +
                                wrap(b'{"spec":{"metadata":{"uid":"inner"}}}') + wrap(b'{"metadata":null}'), 0)
    c["depth"] = (_nest(64) + _nest(65) + _nest(66) + _nest(67), 0)
    # an escape in the type string or in a routed key: the host framer decides the line
    c["escaped_type"] = (b'{"type":"ADD\\u0045D","object":' + pod + b'}\n' + wrap(pod), 1)
    c["escaped_keys"] = (b'{"ty\\u0070e":"ADDED","object":' + pod + b'}\n' +
                         b'{"type":"ADDED","\\u006fbject":' + pod + b'}\n' +
                         wrap(b'{"met\\u0061data":{"uid":"u"}}') +
                         wrap(b'{"metadata":{"u\\u0069d":"u","n\\u0061me":"n"}}') +
                         wrap(b'{"metadata":{"labels":{"\\u0061":"b"}},"sp\\u0065c":{}}') +  # one routed (depth 1), one not
                         wrap(b'{"metadata":{"labels":{"\\u0061":"b"}}}') +                  # not routed: the device's
                         b'{"type":"ADDED","extr\\u0061":1,"object":{}}\n', 6)
    return c


def stream_of_cases():
    """every case's stream made whole lines and joined, with the listed-line total"""
    parts, nh = [], 0
    for name, (s, h) in cases().items():
        if s and not s.endswith(b"\n"):
            s = s[:s.rfind(b"\n") + 1]
        parts.append(s)
        nh += h
    return b"".join(parts), nh


def frames_array(dicts):
    a = np.zeros(len(dicts), abi.WATCH_FRAME_DTYPE)
    for i, d in enumerate(dicts):
        for k in ("line_off", "doc_off", "doc_len", "type", "flags", "status"):
            a[i][k] = d[k]
        for k in ("uid", "resource_version", "name", "namespace_"):
            a[i][k]["off"], a[i][k]["len"] = d[k]
    return a
