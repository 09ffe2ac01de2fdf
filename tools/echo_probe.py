#!/usr/bin/env python3
"""The echo ledger at the steady shape, on the metric fleet, heartbeat-once
engine.  Per step, alternating between the ledger path and the parent path in one run:

  * the node step: one MODIFIED line per node, every one the echo of a heartbeat patch
    whose (uid, resourceVersion) was noted with kwok_echo_update right before;
  * the pod step, C4-shaped: N lines of pods the engine holds, every one an echo, and N
    creates (workload.ChurnJson's documents as watch lines).

The ledger path: kwok_frame_watch_gpu, then kwok_ingest_*_framed_echo over ALL frames.
The parent path: kwok_frame_watch_gpu, the host filter, then the framed ingest on `keep`
- with the host filter stood in for by a precomputed `keep` (no echo among the nodes'
lines: nothing to ingest; the pods' creates), the lower bound of what any host map costs.
The notes' upload (kwok_echo_update) is timed on its own: the host path notes into its
dictionary at the same place, which is not timed either.

Device times of the echo kernels come from the engine's own event stamps
(KWOK_INGEST_PROF: the "[kwok echo]" lines on stderr, beside "[kwok watch]" with
k_frame_parse's time over the same frames).  The last line on stdout is one JSON object.

usage: echo_probe.py [--nodes 1000000] [--steps 6]   (its own time limit: --limit seconds)"""
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

from kwok_amd import abi, engine as keng, workload  # noqa: E402
from kwok_amd.codec import Codec  # noqa: E402
from uid_probe import UidChurn, bind_fleet  # noqa: E402
from watch_probe import HEAD, TAIL, as_stream  # noqa: E402

NODE_UID = b"0a7f2c2e-0000-4000-8000-"
NODE_LINE = (b'{"type":"MODIFIED","object":{"kind":"Node","apiVersion":"v1","metadata":{"name":"', b'","uid":"',
             b'","resourceVersion":"', b'"},"status":{}}}\n')


def node_stream(names, serial, out):
    """one MODIFIED line per node: name (12 bytes), uid (36), resourceVersion (8 digits of serial) -> (stream, uid / rv rows)"""
    n = len(names)
    uid = np.concatenate([np.broadcast_to(np.frombuffer(NODE_UID, np.uint8), (n, 24)), workload._digits(np.arange(n, dtype=np.int64), 12)],
                         axis=1)
    rv = workload._digits(np.full(n, serial, np.int64), 8)
    parts = [NODE_LINE[0], names, NODE_LINE[1], uid, NODE_LINE[2], rv, NODE_LINE[3]]
    row = sum(len(p) if isinstance(p, bytes) else p.shape[1] for p in parts)
    v = out[:n * row].reshape(n, row)
    pos = 0
    for p in parts:
        w = len(p) if isinstance(p, bytes) else p.shape[1]
        v[:, pos:pos + w] = np.frombuffer(p, np.uint8) if isinstance(p, bytes) else p
        pos += w
    return out[:n * row], uid, rv


def note(e, uid_rows, rv_rows):
    """kwok_echo_update: one note per row -> (wall ms, bytes uploaded)"""
    n = len(uid_rows)
    ul, rl = uid_rows.shape[1], rv_rows.shape[1]
    arena = np.ascontiguousarray(np.concatenate([uid_rows, rv_rows], axis=1)).reshape(-1)
    uo = np.arange(n, dtype=np.uint64) * (ul + rl)
    ro = uo + ul
    uls, rls = np.full(n, ul, np.uint32), np.full(n, rl, np.uint32)
    op = np.full(n, abi.ECHO_NOTE, np.uint8)
    st = np.empty(n, np.int32)
    t0 = time.perf_counter()
    rc = e._lib.kwok_echo_update(e._h, op.ctypes.data, arena.ctypes.data, uo.ctypes.data, uls.ctypes.data, ro.ctypes.data,
                                 rls.ctypes.data, n, st.ctypes.data)
    ms = (time.perf_counter() - t0) * 1e3
    e._check(rc, "echo_update")
    assert rc == 0 and not st.any()
    return ms, arena.nbytes + uo.nbytes + ro.nbytes + uls.nbytes + rls.nbytes + op.nbytes


def rows_of(stream, frames, key, width):
    off = frames[key]["off"].astype(np.int64)
    assert (frames[key]["len"] == width).all()
    return stream[off[:, None] + np.arange(width)]


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
    e.uid_dir_enable()
    e.echo_enable()
    bind_fleet(e, pods)
    n_handles = workload.BUCKETS * fl.cp
    ch = UidChurn(pods, np.repeat(fl.node_handles, workload.PODS_PER_NODE), 0, n_handles, n, seed=7,
                  alloc=keng.host_array, node_name_of=workload.node_names_by_handle(fl))
    ch.start(n_handles)
    codec = Codec(manage_all_nodes=True)
    dump = lambda: e.dump_pods(0, n_handles)  # noqa: E731
    nbuf = keng.host_array((n * 256,), np.uint8)
    sbuf = None
    res = {k: [] for k in ("node_ledger", "node_parent", "pod_ledger", "pod_parent", "node_note", "pod_note", "node_frame",
                           "pod_frame", "node_ingest_echo", "pod_ingest_echo", "pod_ingest_keep")}
    note_bytes = {}
    for k in range(a.steps + 2):  # (two untimed steps first, one of each kind)
        now += 30
        ledger = k % 2 == 1
        print("---- step %d: %s" % (k, "ledger" if ledger else "parent path"), file=sys.stderr, flush=True)
        # ---- nodes: every line an echo ----
        stream, uid, rv = node_stream(fl.names, 10_000_000 + k, nbuf)
        if ledger:
            ms, note_bytes["nodes"] = note(e, uid, rv)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames, used, _nh, sid = e.frame_watch(stream, cap=n)
        t1 = time.perf_counter()
        assert len(frames) == n and used == stream.nbytes and not frames["status"].any()
        if ledger:
            hs, st, _nh2, ne = e.ingest_nodes_framed_echo(codec, sid, np.arange(n, dtype=np.uint32))
            assert ne == n and (st == abi.ECHO).all() and (hs >= 0).all()
        t2 = time.perf_counter()  # (the parent path: keep is empty, nothing follows the framing)
        if k >= 2:
            res["node_ledger" if ledger else "node_parent"].append((t2 - t0) * 1e3)
            res["node_frame"].append((t1 - t0) * 1e3)
            if ledger:
                res["node_note"].append(ms)
                res["node_ingest_echo"].append((t2 - t1) * 1e3)
        # ---- pods: N echoes of pods the engine holds, N creates ----
        arena, offs, lens, ops, handles = ch.batch_json(dump, now)
        if sbuf is None:
            sbuf = keng.host_array((int(lens.sum()) + (len(HEAD) + len(TAIL)) * len(lens),), np.uint8)
        stream = as_stream(arena, lens, sbuf)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames, used, _nh, sid = e.frame_watch(stream, cap=len(lens))
        t1 = time.perf_counter()
        assert len(frames) == 2 * n and used == stream.nbytes
        idx = np.arange(2 * n, dtype=np.uint32)
        if ledger:  # (the notes come from the patches' responses: here from the lines themselves, outside the timed part)
            ms, note_bytes["pods"] = note(e, rows_of(stream, frames[:n], "uid", 36), rows_of(stream, frames[:n], "resource_version", 8))
            torch.cuda.synchronize()
            t1b = time.perf_counter()
            hs, st, _rel, _nh2, runs, ne = e.ingest_pods_framed_echo(codec, sid, idx)
            t2 = time.perf_counter()
            assert ne == n and (st[:n] == abi.ECHO).all() and not st[n:].any() and (hs[:n] == handles[:n]).all()
            new = hs[n:]
        else:
            t1b = time.perf_counter()
            new, st, _rel, _nh2, runs = e.ingest_pods_framed_uid(codec, sid, idx[n:])  # keep: the creates
            t2 = time.perf_counter()
            assert not st.any()
        # outside the timed part: the deletion-marked lines are ingested after all, so that the tick removes those
        # pods and the fleet stays at its size
        h0, s0, _rel, _nh2, _r = e.ingest_pods_framed_uid(codec, sid, idx[:n])
        assert not s0.any() and (h0 == handles[:n]).all()
        e.tick(now, read=False)
        ch.applied(np.concatenate([h0, new]), np.zeros(2 * n, np.int32))
        if k >= 2:
            res["pod_ledger" if ledger else "pod_parent"].append((t1 - t0 + t2 - t1b) * 1e3)
            res["pod_frame"].append((t1 - t0) * 1e3)
            if ledger:
                res["pod_note"].append(ms)
                res["pod_ingest_echo"].append((t2 - t1b) * 1e3)
            else:
                res["pod_ingest_keep"].append((t2 - t1b) * 1e3)
    med = lambda v: float(np.median(v)) if v else None  # noqa: E731
    rng = lambda v: [min(v), max(v)] if v else None  # noqa: E731
    s = e.echo_stats()
    out = {"workload": "%d node MODIFIED lines, all echoes; then %d pod echoes + %d creates, per step" % (n, n, n),
           "steps_ms": res, "median_ms": {k: med(v) for k, v in res.items()}, "range_ms": {k: rng(v) for k, v in res.items()},
           "note_upload_bytes_per_step": note_bytes, "echo_stats": s,
           "ledger_bytes": {"pool": s["table_entries"] * 256, "note": "256 bytes per noted uid; the table adds 4 bytes per entry of its capacity"},
           "note": "device time of the echo kernels and of k_frame_parse: the [kwok echo] / [kwok watch] lines above"}
    e.close()
    codec.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
