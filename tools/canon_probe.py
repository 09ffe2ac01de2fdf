#!/usr/bin/env python3
"""The node status blob canonicaliser at the shape it is for: kwok_ingest_nodes_json over N node
documents as an apiserver returns nodes kwok has patched - the three status blobs (addresses in struct order,
distinct per node), the ten nodeInfo strings, phase, five conditions, and a few KB of images and managedFields.

Two engines in one process, fed the same arena in alternating calls: one with kwok_canon_enable (the "on" leg),
one without (the "off" leg: every document goes through the host codec's DOM, as at the parent commit).  Per
leg: 2 warm-up calls, then the median, minimum and maximum wall time of 10 calls (the call ends in a device
synchronise).  After the first call the nodes exist: the timed calls are upserts of known nodes, as a relist
is.  Handles and statuses of the two legs are compared.  The engine's own stamps (KWOK_INGEST_PROF: the
"[kwok json]", "[kwok canon]" and "[kwok ingest]" lines) go to stderr beside the numbers.

The off leg uses only entries the parent commit has: run the probe with KWOK_ENGINE_LIB naming a build of the
parent for the baseline; the on leg is skipped when the library lacks kwok_canon_enable.  The last line on
stdout is one JSON object.

usage: canon_probe.py [--nodes 100000] [--calls 10] [--warmup 2]   (its own time limit: --limit seconds)"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("KWOK_INGEST_PROF", "1")
import torch  # noqa: E402,F401  (the HIP runtime the engine binds)

from kwok_amd import abi, engine as keng  # noqa: E402
from kwok_amd.codec import Codec  # noqa: E402

CONDITIONS = [("Ready", "True", "KubeletReady", "kubelet is posting ready status"),
              ("MemoryPressure", "False", "KubeletHasSufficientMemory", "kubelet has sufficient memory available"),
              ("DiskPressure", "False", "KubeletHasNoDiskPressure", "kubelet has no disk pressure"),
              ("PIDPressure", "False", "KubeletHasSufficientPID", "kubelet has sufficient PID available"),
              ("NetworkUnavailable", "False", "RouteCreated", "RouteController created a route")]
NODE_INFO = {"architecture": "amd64", "bootID": "", "containerRuntimeVersion": "", "kernelVersion": "", "kubeProxyVersion": "fake",
             "kubeletVersion": "fake", "machineID": "", "operatingSystem": "linux", "osImage": "", "systemUUID": ""}


def node_documents(n):
    """(arena, offsets, lengths): n documents, compact, keys in the apiserver's struct order"""
    ts = "2024-01-01T00:00:30Z"
    fields = {"f:status": {"f:addresses": {".": {}, 'k:{"type":"InternalIP"}': {".": {}, "f:address": {}, "f:type": {}}},
                           "f:allocatable": {".": {}, "f:cpu": {}, "f:memory": {}, "f:pods": {}},
                           "f:capacity": {".": {}, "f:cpu": {}, "f:memory": {}, "f:pods": {}},
                           "f:conditions": {".": {}, **{'k:{"type":"%s"}' % c[0]: {".": {}, "f:lastHeartbeatTime": {}, "f:lastTransitionTime": {},
                                                                                   "f:message": {}, "f:reason": {}, "f:status": {}, "f:type": {}}
                                                        for c in CONDITIONS}},
                           "f:nodeInfo": {"f:architecture": {}, "f:kubeProxyVersion": {}, "f:kubeletVersion": {}, "f:operatingSystem": {}},
                           "f:phase": {}}}
    managed = [{"manager": "kwok", "operation": "Update", "apiVersion": "v1", "time": ts, "fieldsType": "FieldsV1", "fieldsV1": fields,
                "subresource": "status"},
               {"manager": "kubectl-create", "operation": "Update", "apiVersion": "v1", "time": "2024-01-01T00:00:00Z", "fieldsType": "FieldsV1",
                "fieldsV1": {"f:metadata": {"f:annotations": {".": {}, "f:kwok.x-k8s.io/node": {}, "f:node.alpha.kubernetes.io/ttl": {}},
                                            "f:labels": {".": {}, "f:kubernetes.io/hostname": {}, "f:type": {}}}}}]
    images = [{"names": ["registry.k8s.io/image-%02d@sha256:%064x" % (k, 0x1234567 * (k + 1)), "registry.k8s.io/image-%02d:v1.%d.0" % (k, k)],
               "sizeBytes": 31000000 + 1234567 * k} for k in range(10)]
    conds = [{"type": c[0], "status": c[1], "lastHeartbeatTime": ts, "lastTransitionTime": "2024-01-01T00:00:00Z", "reason": c[2],
              "message": c[3]} for c in CONDITIONS]
    dumps = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
    head = '{"kind":"Node","apiVersion":"v1","metadata":{"name":"'
    mid1 = ('","resourceVersion":"%d","creationTimestamp":"2024-01-01T00:00:00Z","labels":{"kubernetes.io/hostname":"')
    tail = ('","type":"kwok"},"annotations":{"kwok.x-k8s.io/node":"fake","node.alpha.kubernetes.io/ttl":"0"},"managedFields":' + dumps(managed) +
            '},"spec":{},"status":{"capacity":{"cpu":"32","memory":"256Gi","pods":"110"},"allocatable":{"cpu":"32","memory":"256Gi","pods":"110"},'
            '"phase":"Running","conditions":' + dumps(conds) + ',"addresses":[{"type":"InternalIP","address":"%s"},{"type":"Hostname","address":"%s"}],'
            '"daemonEndpoints":{"kubeletEndpoint":{"Port":0}},"nodeInfo":' + dumps(NODE_INFO) + ',"images":' + dumps(images) + "}}")
    parts = []
    for i in range(n):
        name = "kwok-node-%07d" % i
        ip = "10.%d.%d.%d" % (i >> 16, (i >> 8) & 255, i & 255)
        parts.append((head + name + '","uid":"0a7f2c2e-0000-4000-8000-%012d' % i + mid1 % (1000 + i) + name + tail % (ip, name)).encode())
    lens = np.fromiter((len(p) for p in parts), np.uint32, n)
    offs = np.zeros(n, np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return b"".join(parts), offs, lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=540)
    a = ap.parse_args()
    signal.alarm(a.limit)
    lib = keng.load_engine_lib()
    have_on = hasattr(lib, "kwok_canon_enable")
    arena, offs, lens = node_documents(a.nodes)
    ops = np.full(a.nodes, abi.OP_UPSERT, np.uint8)
    buckets = 1 << max(6, int(np.ceil(np.log2(a.nodes / 24))))
    codec = Codec(manage_all_nodes=False, manage_nodes_with_annotation_selector="kwok.x-k8s.io/node=fake")
    legs = {"off": keng.Engine(keng.make_config(buckets=buckets, node_slots_per_bucket=64, pod_slots_per_bucket=8))}
    if have_on:
        legs["on"] = keng.Engine(keng.make_config(buckets=buckets, node_slots_per_bucket=64, pod_slots_per_bucket=8))
        legs["on"].canon_enable()
    print("canon_probe: %d documents, %.1f MB (%.0f bytes each), legs: %s" % (a.nodes, len(arena) / 1e6, len(arena) / a.nodes, ", ".join(legs)),
          flush=True)
    times = {k: [] for k in legs}
    n_host, answers = {}, {}
    for call in range(a.warmup + a.calls):
        for k, e in legs.items():  # alternating: both legs see the same moments of the shared host
            sys.stderr.write("[probe] leg %s call %d%s\n" % (k, call, " (warm-up)" if call < a.warmup else ""))
            sys.stderr.flush()
            t0 = time.perf_counter()
            hs, st, nh = e.ingest_nodes_json(codec, arena, offs, lens, ops)
            ms = (time.perf_counter() - t0) * 1e3
            if call >= a.warmup:
                times[k].append(ms)
            n_host[k] = nh
            answers[k] = (hs.copy(), st.copy())
            assert not st.any(), "leg %s: %d documents rejected" % (k, int((st != 0).sum()))
    if have_on:
        assert (answers["on"][0] == answers["off"][0]).all() and (answers["on"][1] == answers["off"][1]).all(), "the legs' answers differ"
    out = {"probe": "canon", "nodes": a.nodes, "arena_bytes": len(arena), "calls": a.calls, "warmup": a.warmup,
           "library": os.environ.get("KWOK_ENGINE_LIB") or "in-tree"}
    for k in legs:
        t = times[k]
        out[k] = {"median_ms": round(statistics.median(t), 2), "min_ms": round(min(t), 2), "max_ms": round(max(t), 2), "n_host": n_host[k]}
        print("leg %-3s: median %.2f ms, min %.2f, max %.2f over %d calls; documents the host codec decoded per call: %d" % (
            k, out[k]["median_ms"], out[k]["min_ms"], out[k]["max_ms"], len(t), n_host[k]))
    if have_on:
        out["canon_stats"] = legs["on"].canon_stats()
    print(json.dumps(out))
    for e in legs.values():
        e.close()
    codec.close()


if __name__ == "__main__":
    main()
