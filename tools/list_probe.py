#!/usr/bin/env python3
"""The List body framer at the metric fleet's document shapes: pages
of Running pods (workload's pod document, ~1.5 KB) and of nodes (~1.1 KB), one
body of --big pods and pager-sized bodies of 500 and 10k items.

  * each new kernel group's device time and bytes per second, from the engine's
    own event stamps (KWOK_INGEST_PROF: the "[kwok list]" lines on stderr), and
    the whole call;
  * kwok_frame_watch_gpu's kernels over the same documents wrapped as watch
    lines, in the same run, alternating ("[kwok watch]" lines);
  * the framed ingest of the resident body after the list call;
  * the host framer (kwok_frame_list) on one thread over the 10k-item body.

usage: list_probe.py [--big 1000000] [--reps 3]   (its own time limit: --limit seconds)"""
import argparse
import json
import os
import re
import signal
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["KWOK_INGEST_PROF"] = "1"
import torch  # noqa: E402,F401  (the HIP runtime the engine binds)

from kwok_amd import engine as keng, workload  # noqa: E402
from kwok_amd.codec import Codec, frame_list  # noqa: E402

RUNNING_DOC = workload.DocTemplate(
    workload._META + '"labels":{"app":"fake"}},' + workload._SPEC + '"status":{"phase":"Running","conditions":[' +
    ",".join(workload._COND % t for t in ("Initialized", "Ready", "ContainersReady")).replace("{ct}", "{ct2}") +
    '],"hostIP":"196.168.0.1","podIP":{pip},"podIPs":[{"ip":{pip}}],"startTime":"{ct3}","containerStatuses":[{"name":'
    '"fake-pod","state":{"running":{"startedAt":"{ct4}"}},"lastState":{},"ready":true,"restartCount":0,'
    '"image":"fake","imageID":""}],"qosClass":"BestEffort"}}',
    dict(name=12, uid=36, rv=8, ct=20, ct2=20, ct3=20, ct4=20, node=12, pip=17))
NODE_DOC = workload.DocTemplate(
    '{"kind":"Node","apiVersion":"v1","metadata":{"name":"{name}","uid":"{uid}","resourceVersion":"{rv}",'
    '"creationTimestamp":"2024-01-01T00:00:00Z","annotations":{"kwok.x-k8s.io/node":"fake"}},"spec":{},'
    '"status":{"capacity":{"cpu":"1k","memory":"1Ti","pods":"1M"},"allocatable":{"cpu":"1k","memory":"1Ti","pods":"1M"},'
    '"conditions":[{"type":"Ready","status":"True","lastHeartbeatTime":"2024-01-01T00:00:00Z","lastTransitionTime":'
    '"2024-01-01T00:00:00Z","reason":"KubeletReady","message":"kubelet is posting ready status"}],'
    '"addresses":[{"type":"InternalIP","address":"196.168.0.1"}],"daemonEndpoints":{"kubeletEndpoint":{"Port":0}},'
    '"nodeInfo":{"machineID":"","systemUUID":"","bootID":"","kernelVersion":"","osImage":"","containerRuntimeVersion":"",'
    '"kubeletVersion":"fake","kubeProxyVersion":"fake","operatingSystem":"linux","architecture":"amd64"},"phase":"Running"}}',
    dict(name=12, uid=36, rv=8))
W_HEAD, W_TAIL = b'{"type":"ADDED","object":', b"}\n"


def docs(kind, n):
    """(n, L) uint8: n documents of one length"""
    k = np.arange(n)
    name = np.frombuffer(b"".join(b"%s-%07d" % (b"node" if kind == "nodes" else b"pod0", i) for i in range(n)), np.uint8).reshape(n, 12)
    uid = np.frombuffer(b"".join(b"7d3c0e9a-0000-4000-8000-%012d" % i for i in range(n)), np.uint8).reshape(n, 36)
    vals = dict(name=name, uid=uid, rv=workload._digits(10_000_000 + k, 8))
    if kind == "nodes":
        return NODE_DOC.fill(n, vals)
    ct = workload.rfc3339_rows(np.full(n, workload.S0 - 60))
    node = np.frombuffer(b"".join(b"node-%07d" % (i // workload.PODS_PER_NODE) for i in range(n)), np.uint8).reshape(n, 12)
    vals.update(ct=ct, ct2=ct, ct3=ct, ct4=ct, node=node, pip=workload.quoted_ips((0x0A000001 + k).astype(np.uint32)))
    return RUNNING_DOC.fill(n, vals)


def list_body(kind, rows):
    """the rows as one List body (a comma after every item but the last) in page-locked memory"""
    n, L = rows.shape
    head = b'{"kind":"%s","apiVersion":"v1","metadata":{"resourceVersion":"12345678"},"items":[' % (
        b"NodeList" if kind == "nodes" else b"PodList")
    out = keng.host_array((len(head) + n * (L + 1) + 1,), np.uint8)
    out[:len(head)] = np.frombuffer(head, np.uint8)
    v = out[len(head):len(head) + n * (L + 1)].reshape(n, L + 1)
    v[:, :L] = rows
    v[:, L] = ord(",")
    out[len(head) + n * (L + 1) - 1:] = np.frombuffer(b"]}", np.uint8)
    return out


def watch_stream(rows):
    n, L = rows.shape
    row = len(W_HEAD) + L + len(W_TAIL)
    out = keng.host_array((n * row,), np.uint8)
    v = out.reshape(n, row)
    v[:, :len(W_HEAD)] = np.frombuffer(W_HEAD, np.uint8)
    v[:, len(W_HEAD):len(W_HEAD) + L] = rows
    v[:, len(W_HEAD) + L:] = np.frombuffer(W_TAIL, np.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=540)
    a = ap.parse_args()
    signal.alarm(a.limit)  # the probe's own time limit
    # the engine's stamps go to stderr: kept in a file and read back per call
    log = tempfile.TemporaryFile(mode="w+b")
    saved = os.dup(2)
    os.dup2(log.fileno(), 2)
    try:
        run(a, log)
    finally:
        os.dup2(saved, 2)
        log.seek(0)
        sys.stderr.write(log.read().decode(errors="replace")[-3000:])


def run(a, log):
    e = keng.Engine(keng.make_config(cidr=workload.CIDR, node_ip=workload.NODE_IP, buckets=workload.BUCKETS,
                                     node_slots_per_bucket=64, pod_slots_per_bucket=640, pod_handle_stride=65528,
                                     heartbeat_once=True))
    codec = Codec(manage_all_nodes=True)
    rows_out = []

    def stamps():
        log.flush()
        log.seek(0)
        text = log.read().decode(errors="replace")
        log.seek(0)
        log.truncate()
        return text

    for kind, n in (("pods", 500), ("pods", 10_000), ("pods", a.big), ("nodes", 500), ("nodes", 10_000), ("nodes", 100_000)):
        rows = docs(kind, n)
        body, stream = list_body(kind, rows), watch_stream(rows)
        rec = dict(kind=kind, items=n, body_bytes=int(body.nbytes), stream_bytes=int(stream.nbytes), list=[], watch=[])
        for r in range(a.reps + 1):  # (one untimed round first), alternating
            stamps()
            t0 = time.perf_counter()
            frames, info, nh, sid = e.frame_list(body, cap=n)
            ms = (time.perf_counter() - t0) * 1e3
            assert len(frames) == n and nh == 0
            m = re.search(r"quotes \+ scans ([\d.]+) ms.*?scans ([\d.]+) ms.*?k_list_range ([\d.]+) ms, k_list_parse ([\d.]+) ms", stamps())
            if r:
                rec["list"].append(dict(call_ms=ms, quotes_ms=float(m[1]), count_ms=float(m[2]), emit_ms=float(m[3]),
                                        parse_ms=float(m[4])))
            t0 = time.perf_counter()
            wframes, used, nh, _sid = e.frame_watch(stream, cap=n)
            ms = (time.perf_counter() - t0) * 1e3
            assert len(wframes) == n and used == stream.nbytes and not wframes["status"].any()
            m = re.search(r"k_frame_scan ([\d.]+) ms, k_frame_emit ([\d.]+) ms, k_frame_parse ([\d.]+) ms", stamps())
            if r:
                rec["watch"].append(dict(call_ms=ms, count_ms=float(m[1]), emit_ms=float(m[2]), parse_ms=float(m[3])))
        med = lambda rs, k: float(np.median([x[k] for x in rs]))  # noqa: E731
        L, Wm = rec["list"], rec["watch"]
        split = med(L, "quotes_ms") + med(L, "count_ms") + med(L, "emit_ms")
        wsplit = med(Wm, "count_ms") + med(Wm, "emit_ms")
        rec["median"] = dict(
            list=dict(call_ms=med(L, "call_ms"), quotes_ms=med(L, "quotes_ms"), count_ms=med(L, "count_ms"),
                      emit_ms=med(L, "emit_ms"), parse_ms=med(L, "parse_ms"), split_ms=split,
                      quotes_GBps=body.nbytes / med(L, "quotes_ms") / 1e6, count_GBps=body.nbytes / med(L, "count_ms") / 1e6,
                      emit_GBps=body.nbytes / med(L, "emit_ms") / 1e6, parse_GBps=body.nbytes / med(L, "parse_ms") / 1e6),
            watch=dict(call_ms=med(Wm, "call_ms"), count_ms=med(Wm, "count_ms"), emit_ms=med(Wm, "emit_ms"),
                       parse_ms=med(Wm, "parse_ms"), split_ms=wsplit),
            list_device_over_watch_device=(split + med(L, "parse_ms")) / (wsplit + med(Wm, "parse_ms")),
            list_split_over_watch_split_plus_parse=split / (wsplit + med(Wm, "parse_ms")))
        # the framed ingest of the resident body (the list call again: the watch replaced it)
        frames, info, nh, sid = e.frame_list(body, cap=n)
        t0 = time.perf_counter()
        if kind == "pods":
            hs, st, _rel, nh2 = e.ingest_pods_framed(codec, sid, np.arange(n, dtype=np.uint32), np.full(n, -1, np.int32))
        else:
            hs, st, nh2 = e.ingest_nodes_framed(codec, sid, np.arange(n, dtype=np.uint32))
        rec["framed_ingest"] = dict(ms=(time.perf_counter() - t0) * 1e3, ok=int((st == 0).sum()), host_docs=int(nh2))
        if n == 10_000:  # the host framer, one thread
            b = body.tobytes()
            t0 = time.perf_counter()
            hf, _ = frame_list(b, cap=n)
            dt = time.perf_counter() - t0
            rec["host_framer"] = dict(threads=1, ms=dt * 1e3, items_per_s=len(hf) / dt, GB_per_s=len(b) / dt / 1e9)
        del rec["list"], rec["watch"]
        rows_out.append(rec)
        stamps()
    out = dict(workload="List pages of Running pods / nodes against the same documents as watch ADDED lines", rows=rows_out,
               list_stats=e.list_stats())
    e.close()
    codec.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
