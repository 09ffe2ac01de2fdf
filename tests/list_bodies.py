"""Test infrastructure for the List body framer (include/kwok_watch.h): a Python
framer written from the rules (json.loads over the body, first key wins, depth
<= 64), the named cases both framers are run over with what the device leaves to
the host, the boundary sweeps of the device's split, and the byte mutations."""
import json
import random

import numpy as np

from kwok_amd import abi
from watch_frames import META_KEYS, POD, _dec, _depth, _first, _members

WS = " \t\r\n"
TILE = abi.WATCH_TILE
INFO_KEYS = [("kind", abi.LIST_ESC_KIND), ("resource_version", abi.LIST_ESC_RV), ("continue_", abi.LIST_ESC_CONTINUE)]


def _elements(text, i):
    """the elements of the array whose '[' is text[i]: (start, end)"""
    out = []
    i += 1
    while True:
        while text[i] in WS:
            i += 1
        if text[i] == "]":
            return out
        _, end = _dec.raw_decode(text, i)
        out.append((i, end))
        i = end
        while text[i] in WS:
            i += 1
        if text[i] == ",":
            i += 1


def _str_span(text, v):
    """(span inside the quotes, escaped) of the member value v when it is a string"""
    if v is None or text[v[0]] != '"':
        return (0, 0), False
    raw = text[v[0] + 1:v[1] - 1]
    return ((v[0] + 1, len(raw)) if raw else (0, 0)), "\\" in raw


def py_item(text, a, b):
    f = dict(line_off=a, doc_off=a, doc_len=b - a, type=abi.WATCH_ADDED, flags=0, status=abi.OK,
             uid=(0, 0), resource_version=(0, 0), name=(0, 0), namespace_=(0, 0))
    md = _first(_members(text, a), "metadata")
    if md is None or text[md[0]] != "{":
        return f
    mm = _members(text, md[0])
    for key, field, bit in META_KEYS:
        f[field], esc = _str_span(text, _first(mm, key))
        if esc:
            f["flags"] |= bit
    return f


def py_list(body):
    """(status, frames as dicts, info as a dict) of a List body by the rules of kwok_watch.h"""
    info = dict(kind=(0, 0), resource_version=(0, 0), continue_=(0, 0), items=(0, 0), flags=0)
    bad = (abi.EINVAL, [], dict(info))
    try:
        text = body.decode()  # (the cases are ASCII: byte offsets are character offsets)
        assert len(text) == len(body)
        root = json.loads(text)
    except (ValueError, AssertionError, RecursionError):
        return bad
    if not isinstance(root, dict) or _depth(text) > 65:  # depth <= 64 below the root value (depth 0)
        return bad
    top = _members(text, text.index("{"))
    it = _first(top, "items")
    frames = []
    if it is not None and text[it[0]:it[1]] != "null":
        if text[it[0]] != "[":
            return bad
        spans = _elements(text, it[0])
        if any(text[a] != "{" for a, _ in spans):
            return bad
        frames = [py_item(text, a, b) for a, b in spans]
        info["items"] = (it[0], it[1] - it[0])
    info["kind"], esc = _str_span(text, _first(top, "kind"))
    info["flags"] |= abi.LIST_ESC_KIND if esc else 0
    md = _first(top, "metadata")
    if md is not None and text[md[0]] == "{":
        mm = _members(text, md[0])
        info["resource_version"], esc = _str_span(text, _first(mm, "resourceVersion"))
        info["flags"] |= abi.LIST_ESC_RV if esc else 0
        info["continue_"], esc = _str_span(text, _first(mm, "continue"))
        info["flags"] |= abi.LIST_ESC_CONTINUE if esc else 0
    return abi.OK, frames, info


def info_dict(info):
    d = {k: (getattr(info, k).off, getattr(info, k).len) for k in ("kind", "resource_version", "continue_", "items")}
    d["flags"] = info.flags
    return d


def cj(obj):
    return json.dumps(obj, separators=(",", ":")).encode()


def pod(k, **meta):
    md = dict(POD["metadata"], name="pod-%d" % k, uid="u-pod-%d" % k, resourceVersion=str(100 + k))
    md.update(meta)
    return cj(dict(POD, metadata=md))


def node(k):
    return cj({"apiVersion": "v1", "kind": "Node",
               "metadata": {"name": "node-%d" % k, "uid": "u-node-%d" % k, "resourceVersion": str(7 + k),
                            "annotations": {"kwok.x-k8s.io/node": "fake"}},
               "spec": {}, "status": {"phase": "Running"}})


def body_of(items, kind="PodList", rv="1234", cont=None, sep=b","):
    md = {"resourceVersion": rv}
    if cont is not None:
        md["continue"] = cont
    return (b'{"kind":"%s","apiVersion":"v1","metadata":%s,"items":[' % (kind.encode(), cj(md)) + sep.join(items) + b"]}")


def _nest_item(n):
    """a one-item body whose containers nest n deep (the root object is 1, the array 2, the item 3)"""
    return b'{"items":[{"a":' + b"[" * (n - 3) + b"]" * (n - 3) + b"}]}"


def cases():
    """name -> (body, items the device lists for the host, 1 when the body is the host framer's whole)"""
    p = [pod(k) for k in range(4)]
    c = {}
    c["pod_list"] = (body_of(p[:3]), 0, 0)
    c["node_list"] = (body_of([node(k) for k in range(3)], kind="NodeList", rv="99"), 0, 0)
    c["items_first"] = (b'{"items":[' + p[0] + b"," + p[1] + b'],"kind":"PodList","metadata":{"resourceVersion":"8"}}', 0, 0)
    c["whitespace"] = (b' \r\n{ "kind" : "PodList" ,\t"metadata" : { "resourceVersion" :\n"5" , "continue" : "" } , "items" : [ ' +
                       json.dumps(POD, indent=1).encode() + b" \t,\r\n" + json.dumps(POD, indent=2).encode() +
                       b" \n] \t} \r\n", 0, 0)
    c["items_absent"] = (b'{"kind":"PodList","metadata":{"resourceVersion":"5"}}', 0, 1)
    c["items_null"] = (b'{"kind":"PodList","metadata":{"resourceVersion":"5"},"items":null}', 0, 1)
    c["items_empty"] = (body_of([]), 0, 0)
    c["items_empty_ws"] = (b'{"kind":"NodeList","items":[ \r\n\t ],"metadata":{"resourceVersion":"3"}}', 0, 0)
    c["one_item"] = (body_of(p[:1]), 0, 0)
    c["no_metadata"] = (body_of([b"{}", b'{"spec":{"metadata":{"uid":"inner"}}}', b'{"metadata":null}', b'{"metadata":["uid"]}',
                                 b'{"metadata":{"uid":7,"name":null,"namespace":{"name":"x"},"resourceVersion":""}}']), 0, 0)
    c["root_metadata_array"] = (b'{"kind":7,"metadata":["resourceVersion"],"items":[' + p[0] + b"]}", 0, 1)  # two root arrays
    c["root_metadata_number"] = (b'{"kind":null,"metadata":7,"items":[' + p[0] + b"]}", 0, 0)
    c["duplicate_items"] = (b'{"items":[' + p[0] + b'],"items":[' + p[1] + b"," + p[2] + b"]}", 0, 1)
    c["duplicate_items_null_later"] = (b'{"items":[' + p[0] + b'],"items":null,"kind":"PodList"}', 0, 0)
    c["duplicate_items_null_first"] = (b'{"items":null,"items":[' + p[0] + b'],"kind":"PodList"}', 0, 1)
    c["duplicate_metadata"] = (b'{"metadata":{"resourceVersion":"1","resourceVersion":"2","continue":"a"},'
                               b'"metadata":{"resourceVersion":"3","continue":"b"},"kind":"PodList","kind":"NodeList","items":['
                               b'{"metadata":{"uid":"first","uid":"second","name":"n"},"metadata":{"uid":"third","namespace":"x"}}]}',
                               0, 0)
    c["escaped_values"] = (body_of([pod(0, uid='u\\-"q"', name="café", namespace="d"),
                                    b'{"metadata":{"resourceVersion":"4\\u0031","namespace":"a\\/b","uid":"","name":7}}']), 0, 0)
    c["escaped_item_keys"] = (body_of([b'{"met\\u0061data":{"uid":"u"}}', p[0],
                                       b'{"metadata":{"u\\u0069d":"u","n\\u0061me":"n"}}',
                                       b'{"metadata":{"labels":{"\\u0061":"b"}},"sp\\u0065c":{}}',  # one routed key, one not
                                       b'{"metadata":{"labels":{"\\u0061":"b"},"uid":"dev"}}']), 3, 0)  # not routed: the device's
    c["escaped_items_key"] = (b'{"kind":"PodList","\\u0069tems":[' + p[0] + b"," + p[1] + b"]}", 0, 1)
    c["escaped_root_keys"] = (b'{"k\\u0069nd":"PodList","met\\u0061data":{"resourceV\\u0065rsion":"12"},"items":[' + p[0] + b"]}", 0, 0)
    c["brackets_in_strings"] = (body_of([b'{"a":"}{[]","b":"\\"","c":"\\\\","d":"\\\\\\"","}{":"][","metadata":{"name":"]}","uid":"{["}}',
                                         b'{"\\"":"x\\\\","metadata":{"uid":"\\\\\\\\","name":"a\\"}"}}', p[0]]), 1, 0)  # (the key \" is at an item's routed level)
    c["continue_token"] = (body_of(p[:2], cont="eyJ2IjoibWV0YS5rOHMuaW8vdjEiLCJydiI6MTIzNH0"), 0, 0)
    c["continue_escaped"] = (b'{"metadata":{"continue":"abc\\u003d\\u003d","resourceVersion":"1\\u0032"},"kind":"Pod\\u004cist",'
                             b'"items":[' + p[0] + b"]}", 0, 0)
    c["objects_beside_items"] = (b'{"metadata":{"resourceVersion":"1","managed":{"a":{"b":{}}},"x":[{"y":{}}]},"items":[' + p[0] + b"," +
                                 p[1] + b'],"status":{"details":{"causes":{}}},"z":{"arr":[{"q":{}}]}}', 0, 0)
    for n in (64, 65, 66, 67):
        c["depth_%d" % n] = (_nest_item(n), 0, 0)
    c["item_number"] = (b'{"items":[1]}', 0, 0)
    c["item_then_number"] = (b'{"items":[' + p[0] + b" 1]}", 0, 0)
    c["item_nested_array"] = (b'{"items":[[{}]]}', 0, 0)
    c["item_trailing_comma"] = (b'{"items":[' + p[0] + b",]}", 0, 0)
    c["item_leading_comma"] = (b'{"items":[,' + p[0] + b"]}", 0, 0)
    c["items_no_comma"] = (b'{"items":[' + p[0] + p[1] + b"]}", 0, 0)
    c["items_two_commas"] = (b'{"items":[' + p[0] + b",," + p[1] + b"]}", 0, 0)
    c["items_object"] = (b'{"items":{"a":1}}', 0, 1)
    c["items_string"] = (b'{"kind":"PodList","items":"[{}]"}', 0, 1)
    c["body_array"] = (b'[{"items":[]}]', 0, 1)
    c["body_empty"] = (b"", 0, 0)
    c["body_whitespace"] = (b" \n", 0, 1)
    c["trailing_garbage"] = (body_of(p[:1]) + b" x", 0, 0)
    c["trailing_object"] = (body_of(p[:1]) + b"{}", 0, 0)
    c["two_root_arrays"] = (b'{"items":[' + p[0] + b'],"other":[1,2]}', 0, 1)
    c["root_array_not_items"] = (b'{"kind":"PodList","Items":[' + p[0] + b"]}", 0, 1)
    c["bad_item_inside"] = (body_of([p[0], b'{"a":tru}', p[1]]), 0, 0)
    c["mismatched_close"] = (b'{"items":[' + p[0] + b"}}", 0, 0)
    return c


PREFIX_BODY = body_of([pod(0), b'{"metadata":{"name":"a\\"b","uid":"}{"},"s":"\\\\"}'], rv="77", cont="tok")


# ---- the boundary sweeps of the device's split ---------------------------------
def _run_item(L):
    """an item holding a string with a run of L backslashes (odd: the quote after it is escaped), then brackets"""
    run = b"\\" * L + (b'"' if L & 1 else b"")
    return b'{"metadata":{"name":"n","uid":"u' + (b"%d" % L) + b'"},"s":"a' + run + b'}{[]","t":"][}{\\"]["}'


def _padded(items, pad_at, pad):
    """a body with `pad` spaces put in front of byte pad_at of its unpadded text"""
    b = body_of(items)
    return b[:pad_at] + b" " * pad + b[pad_at:]


def sweep_bodies():
    out = []
    items = [_run_item(L) for L in (1, 2, 3, 4, 5)] + [b"{}", pod(1)]
    plain = body_of(items)
    first_member = 1                       # padding here moves everything, the items `[` included
    for k in range(16):                    # every residue mod 16 for every quote, run, brace and the `[`
        out.append(_padded(items, first_member, k))
    feats = [plain.index(b'"items":[') + 8]                      # the items `[`
    it0 = plain.index(items[0])
    feats += [it0, it0 + len(items[0]) - 1, it0 + 1]             # an item's `{`, its `}`, a quote
    for L, it in zip((1, 2, 3, 4, 5), items):                    # each run's first backslash
        feats.append(plain.index(it) + it.index(b"\\"))
    for edge in (1024, 4096, TILE, 2 * TILE):                    # a wave step, a block step, a tile
        for f in feats[:4]:
            for d in (-1, 0):                                    # the byte on both sides of the edge
                out.append(_padded(items, first_member, edge + d - f))
        for L, f in zip((1, 2, 3, 4, 5), feats[4:]):             # a run straddling the edge every way
            for d in range(-L - 1, 2):
                out.append(_padded(items, first_member, edge + d - f))
    blob = b"}{[]" * (2 * TILE // 4 + 700)                       # a string longer than two tiles, no quote inside
    out.append(body_of([pod(0), b'{"blob":"' + blob + b'","metadata":{"uid":"after-blob"}}', pod(1), b"{}"]))
    out.append(body_of([b'{"blob":"' + blob + b'\\\\"}', pod(2)]))
    wide = b'{"metadata":{"uid":"wide"},' + b" " * TILE + b'"a":{"b":[{}]},' + b"\n" * (TILE + 100) + b'"z":"}"}'
    out.append(body_of([pod(0), wide, pod(1)]))                  # an item spanning three tiles
    out.append(body_of([b"{}"] * 6000))                          # five opens to a window
    out.append(body_of([b"{}"] * 6000, sep=b" ,\n"))
    for total in (15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 5):
        small = b'{"items":[{}]}'
        out.append(small[:10] + b" " * (total - len(small)) + small[10:])
        assert len(out[-1]) == total
    return out


def mutated_bodies(n, seed):
    """byte-mutated and truncated bodies"""
    rng = random.Random(seed)
    pool = [pod(0), pod(1, uid='q"\\'), node(0), b"{}", _run_item(3), _run_item(2), b'{"metadata":{"uid":"}{"}}']
    out = []
    for _ in range(n):
        b = bytearray(body_of(rng.sample(pool, rng.randint(0, 4)), cont=rng.choice([None, "t"])))
        for _ in range(rng.randint(0, 4)):
            b[rng.randrange(len(b))] = rng.choice(b'{}[]",:\\0123456789tfnul \n\r\x00\xff')
        out.append(bytes(b)[:len(b) if rng.random() < 0.7 else rng.randrange(1, len(b) + 1)])
    return out


def frames_array(dicts):
    a = np.zeros(len(dicts), abi.WATCH_FRAME_DTYPE)
    for i, d in enumerate(dicts):
        for k in ("line_off", "doc_off", "doc_len", "type", "flags", "status"):
            a[i][k] = d[k]
        for k in ("uid", "resource_version", "name", "namespace_"):
            a[i][k]["off"], a[i][k]["len"] = d[k]
    return a
