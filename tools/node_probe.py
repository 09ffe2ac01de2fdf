#!/usr/bin/env python3
"""The node uid directory on the metric fleet's nodes: two heartbeat-once
engines holding the same 1M nodes (no pods: the node entries read none), engine A with the
uid directory, the echo ledger, the reference directory and the node directory on, engine B
with the first three.  Steps alternate between the two engines in one run, two untimed
steps first; medians with ranges.

  * the node step of §24's probe: one MODIFIED line per node, every one the echo of a
    heartbeat patch whose (uid, resourceVersion) was noted right before (not timed): the
    whole kwok_ingest_nodes_framed_echo call.  With the directory on the dropped records'
    handles come from k_nd_lookup_frames and the call's answers are merged on the device
    (two arrays come back); with it off the handles come from k_echo_node_handles and four
    arrays come back for a host merge.  Device time (KWOK_INGEST_PROF=1, stderr): the echo
    filter's kernels on "[kwok echo]" lines, and with the directory on everything behind the
    filter on "[kwok nodes]" lines;
  * the C5 flap shape: 10,000 Deleted and 10,000 Added typed node records in one
    kwok_ingest_nodes call; on - off is what k_nd_uid_note costs behind the apply pass;
  * the same 20,000 records as watch lines through kwok_ingest_nodes_framed (the note with
    the frames' uids, and the upload of their spans);
  * kwok_node_lookup of every name in one call (both engines: it needs no directory).

The last line on stdout is one JSON object.

usage: node_probe.py [--nodes 1000000] [--steps 6]   (its own time limit: --limit seconds)"""
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
from echo_probe import NODE_LINE, node_stream, note  # noqa: E402


def build(n, node_dir):
    fl = workload.make_fleet(n)
    cfg = keng.make_config(cidr=workload.CIDR, node_ip=workload.NODE_IP, start_time=workload.S0, buckets=workload.BUCKETS,
                           node_slots_per_bucket=fl.cn, pod_slots_per_bucket=fl.cp, heartbeat_once=True)
    e = keng.Engine(cfg)
    e.uid_dir_enable()
    e.echo_enable()
    e.refs_enable()
    if node_dir:
        e.node_dir_enable()
    hs, st = e.ingest_nodes_raw(fl.node_events, fl.arena)
    assert not st.any()
    fl.node_handles = hs
    return e, fl


def lines(names, uid, typ, serial, out):
    """one watch line of type typ per row of names / uid (36 bytes) -> the stream"""
    n = len(names)
    head = NODE_LINE[0].replace(b"MODIFIED", typ)
    rv = workload._digits(np.full(n, serial, np.int64), 8)
    parts = [head, names, NODE_LINE[1], uid, NODE_LINE[2], rv, NODE_LINE[3]]
    row = sum(len(p) if isinstance(p, bytes) else p.shape[1] for p in parts)
    v = out[:n * row].reshape(n, row)
    pos = 0
    for p in parts:
        w = len(p) if isinstance(p, bytes) else p.shape[1]
        v[:, pos:pos + w] = np.frombuffer(p, np.uint8) if isinstance(p, bytes) else p
        pos += w
    return out[:n * row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--flap", type=int, default=10_000)
    ap.add_argument("--limit", type=int, default=540)
    a = ap.parse_args()
    signal.alarm(a.limit)  # the probe's own time limit
    n, k_flap = a.nodes, a.flap
    eng = {}
    for on in (True, False):
        eng[on] = build(n, on)
    fl = eng[True][1]
    assert (eng[True][1].node_handles == eng[False][1].node_handles).all()
    codec = Codec(manage_all_nodes=True)
    nbuf = keng.host_array((n * 256,), np.uint8)
    fbuf = keng.host_array((2 * k_flap * 256,), np.uint8)
    res = {k: [] for k in ("echo_call_on", "echo_call_off", "frame_on", "frame_off", "flap_typed_on", "flap_typed_off",
                           "flap_framed_on", "flap_framed_off", "lookup_on", "lookup_off")}
    rng = np.random.default_rng(5)
    # kwok_node_lookup's inputs for every name, built once (the names are 12 bytes each)
    l_arena = np.ascontiguousarray(fl.names).reshape(-1)
    l_off = np.arange(n, dtype=np.uint64) * fl.names.shape[1]
    l_len = np.full(n, fl.names.shape[1], np.uint32)
    got = np.empty(n, np.int32)
    now = workload.S0 + 30
    for on in (True, False):
        eng[on][0].tick(now, read=False)
    for k in range(2 * a.steps + 2):  # (two untimed steps first, one per engine)
        on = k % 2 == 1
        tag = "on" if on else "off"
        e = eng[on][0]
        timed = k >= 2
        print("---- step %d: node directory %s" % (k, tag), file=sys.stderr, flush=True)
        # ---- every line an echo ----
        stream, uid, rv = node_stream(fl.names, 10_000_000 + k // 2, nbuf)
        note(e, uid, rv)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames, used, _nh, sid = e.frame_watch(stream, cap=n)
        t1 = time.perf_counter()
        hs, st, _nh2, ne = e.ingest_nodes_framed_echo(codec, sid, np.arange(n, dtype=np.uint32))
        t2 = time.perf_counter()
        assert ne == n and (st == abi.ECHO).all() and (hs == eng[on][1].node_handles).all()
        if timed:
            res["frame_" + tag].append((t1 - t0) * 1e3)
            res["echo_call_" + tag].append((t2 - t1) * 1e3)
        # ---- the flap shape, typed: k Deleted then k Added records ----
        pick = np.sort(rng.choice(n, k_flap, replace=False))
        ev = np.concatenate([fl.node_events[pick], fl.node_events[pick]])
        ev["op"][:k_flap] = abi.OP_DELETE
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h2, s2 = e.ingest_nodes_raw(ev, fl.arena)
        t1 = time.perf_counter()
        assert not s2.any()
        if timed:
            res["flap_typed_" + tag].append((t1 - t0) * 1e3)
        # ---- the flap shape as watch lines (uids from the frames) ----
        fstream = np.concatenate([lines(fl.names[pick], uid[pick], b"DELETED", 20_000_000 + k, fbuf[:k_flap * 256]),
                                  lines(fl.names[pick], uid[pick], b"ADDED", 20_000_001 + k, fbuf[k_flap * 256:])])
        torch.cuda.synchronize()
        frames, used, _nh, sid = e.frame_watch(fstream, cap=2 * k_flap)
        assert len(frames) == 2 * k_flap and not frames["status"].any()
        t0 = time.perf_counter()
        h3, s3, _nh3 = e.ingest_nodes_framed(codec, sid, np.arange(2 * k_flap, dtype=np.uint32))
        t1 = time.perf_counter()
        assert not s3.any()
        if timed:
            res["flap_framed_" + tag].append((t1 - t0) * 1e3)
        # ---- every name in one lookup (a flapped node may sit in another slot of its bucket now) ----
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = e._lib.kwok_node_lookup(e._h, l_arena.ctypes.data, l_off.ctypes.data, l_len.ctypes.data, n, got.ctypes.data)
        t1 = time.perf_counter()
        e._check(rc, "node_lookup")
        assert (got >= 0).all()
        eng[on][1].node_handles = got.copy()
        if timed:
            res["lookup_" + tag].append((t1 - t0) * 1e3)
        now += 30
        e.tick(now, read=False)
    # the uids the directory holds after the run: the flapped nodes' from their ADDED frames
    e = eng[True][0]
    some = eng[True][1].node_handles[:4096]
    refs, blob = e.refs_lookup(abi.KIND_NODES, some)
    med = lambda v: float(np.median(v)) if v else None  # noqa: E731
    rngs = lambda v: [min(v), max(v)] if v else None  # noqa: E731
    out = {"workload": "%d nodes; per step %d MODIFIED lines that are all echoes, then %d Deleted + %d Added typed and as lines, "
                       "then one lookup of every name" % (n, n, k_flap, k_flap),
           "steps_ms": res, "median_ms": {k: med(v) for k, v in res.items()}, "range_ms": {k: rngs(v) for k, v in res.items()},
           "bytes_copied_back_per_record": {"on": 8, "off": 4 + 4 + 1 + 4 + 8,
                                            "note": "off: kidx (kept only), kpos, res, hdrop, then handles + statuses; on: handles + "
                                                    "statuses and one 16-byte word per call"},
           "node_dir_stats": e.node_dir_stats(), "uids_held_of_4096": int((refs["uid_len"] > 0).sum()),
           "note": "device time of the echo kernels: the [kwok echo] lines above"}
    for on in (True, False):
        eng[on][0].close()
    codec.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
