#!/usr/bin/env python3
"""The watch-stream framer at the C4 shape: per step the 2 x N pod
documents of one churn tick (workload.ChurnJson) wrapped as watch frames
({"type":"MODIFIED","object":...}\\n, 30 envelope bytes on ~1.3 KB), on the
metric fleet.

  * the framing kernels' device time (k_frame_count + k_frame_scan,
    k_frame_emit, k_frame_parse) beside k_json_pods' over the same documents in
    the same run: the engine's own stamps (KWOK_INGEST_PROF, the "[kwok watch]"
    and "[kwok json]" lines on stderr; a framed ingest copies nothing, so its
    "decoded" figure is k_json_pods alone);
  * the host framer (kwok_frame_watch) on one thread over one such stream;
  * the framed step - kwok_frame_watch_gpu, the uid -> handle map, then
    kwok_ingest_pods_framed - against the kwok_ingest_pods_json step (the call
    the drop-in makes today, whose code this framer leaves as it was) over the
    same kind of batch on the same engine, in alternating steps.

usage: watch_probe.py [--nodes 1000000] [--steps 6]   (its own time limit: --limit seconds)"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("KWOK_INGEST_PROF", "1")
import torch  # noqa: E402,F401  (the HIP runtime the engine binds)

from kwok_amd import engine as keng, workload  # noqa: E402
from kwok_amd.codec import Codec, frame_watch  # noqa: E402

HEAD, TAIL = b'{"type":"MODIFIED","object":', b"}\n"


def as_stream(arena, lens, out):
    """the batch's documents (two runs of fixed-length rows) each wrapped as one watch line"""
    D = len(lens) // 2
    pos = src = 0
    for L in (int(lens[0]), int(lens[D])):
        row = len(HEAD) + L + len(TAIL)
        v = out[pos:pos + D * row].reshape(D, row)
        v[:, :len(HEAD)] = np.frombuffer(HEAD, np.uint8)
        v[:, len(HEAD):len(HEAD) + L] = arena[src:src + D * L].reshape(D, L)
        v[:, len(HEAD) + L:] = np.frombuffer(TAIL, np.uint8)
        pos += D * row
        src += D * L
    return out[:pos]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--limit", type=int, default=540)
    a = ap.parse_args()
    signal.alarm(a.limit)  # the probe's own time limit
    n = a.nodes
    e, fl, pods = workload.build_engine_fleet(keng.Engine, n, heartbeat_once=True)
    now = workload.S0 + 30
    e.tick(now, read=False)
    n_handles = workload.BUCKETS * fl.cp
    ch = workload.ChurnJson(pods, np.repeat(fl.node_handles, workload.PODS_PER_NODE), 0, n_handles, n, seed=7,
                            alloc=keng.host_array, node_name_of=workload.node_names_by_handle(fl))
    codec = Codec(manage_all_nodes=True)
    dump = lambda: e.dump_pods(0, n_handles)  # noqa: E731
    outs = (keng.host_array((2 * n,), np.int32), keng.host_array((2 * n,), np.int32), keng.host_array((2 * n,), np.uint32))
    sbuf = None
    res = {"json": [], "framed": [], "frame": [], "map": [], "ingest": []}
    host = None
    for k in range(a.steps + 2):  # (two untimed steps first, one of each kind)
        now += 30
        arena, offs, lens, ops, handles = ch.batch_json(dump, now)
        framed = k % 2 == 1
        if framed:
            if sbuf is None:
                sbuf = keng.host_array((int(lens.sum()) + (len(HEAD) + len(TAIL)) * len(lens),), np.uint8)
            stream = as_stream(arena, lens, sbuf)
            if host is None:  # the host framer, one thread (untimed step)
                t0 = time.perf_counter()
                hf, used = frame_watch(stream.tobytes())
                host = (time.perf_counter() - t0, len(hf), int((hf["status"] == 0).sum()), stream.nbytes)
                del hf
        torch.cuda.synchronize()
        print("---- step %d: %s" % (k, "framed" if framed else "ingest_pods_json"), file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        if framed:
            frames, used, nh, sid = e.frame_watch(stream, cap=len(lens))
            t1 = time.perf_counter()
            # the uid -> handle map of the caller: here the generator's (frame i is document i)
            assert len(frames) == len(lens) and used == stream.nbytes and not frames["status"].any()
            idx = np.arange(len(frames), dtype=np.uint32)
            t2 = time.perf_counter()
            hs, st, _rel, nh2 = e.ingest_pods_framed(codec, sid, idx, handles, out=outs)
            t3 = time.perf_counter()
        else:
            hs, st, _rel, nh = e.ingest_pods_json(codec, arena, offs, lens, ops, handles, out=outs)
            t3 = time.perf_counter()
        r = e.tick(now, read=False)
        ch.applied(hs.copy(), st)
        if k >= 2:
            res["framed" if framed else "json"].append((t3 - t0) * 1e3)
            if framed:
                res["frame"].append((t1 - t0) * 1e3)
                res["map"].append((t2 - t1) * 1e3)
                res["ingest"].append((t3 - t2) * 1e3)
    med = lambda v: float(np.median(v)) if v else None  # noqa: E731
    out = {"workload": "C4 as watch frames: %d deletion-marked + %d created pod documents per step" % (n, n),
           "documents_per_step": 2 * n, "stream_bytes": int(host[3]) if host else None,
           "ingest_pods_json_step_ms": res["json"], "framed_step_ms": res["framed"],
           "framed_parts_ms": {"frame_watch_gpu": res["frame"], "map": res["map"], "ingest_pods_framed": res["ingest"]},
           "median_ms": {"ingest_pods_json": med(res["json"]), "framed": med(res["framed"])},
           "framed_over_json": med(res["framed"]) / med(res["json"]) if res["json"] and res["framed"] else None,
           "host_framer": None if host is None else {"threads": 1, "ms": host[0] * 1e3, "frames": host[1], "ok": host[2],
                                                     "frames_per_s": host[1] / host[0], "GB_per_s": host[3] / host[0] / 1e9},
           "watch_stats": e.watch_stats(),
           "note": "device times of the framing kernels and of k_json_pods: the [kwok watch] / [kwok json] lines above"}
    e.close()
    codec.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
