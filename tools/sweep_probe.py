#!/usr/bin/env python3
"""Relist with Replace on the metric fleet: 1M nodes x 10M pods on a
heartbeat-once engine, addresses assigned.

  * the mark cost: kwok_ingest_pods_framed of one 1M-pod page of held pods with a
    resync session open against the same call with none (alternating, medians);
  * the sweep at 0 %, 1 % and 10 % of the pods absent (the present ones marked with
    kwok_resync_mark), split by the engine's own stamps (KWOK_INGEST_PROF, the
    "[kwok resync]" line) into count + scan, emit and the apply chain; bytes read
    per pass and GB/s; k_frame_count + k_frame_scan over as many bytes beside it;
  * what a caller does without the sweep, in the same run: the host diff of the
    listed uids against its uid -> handle map (TIMED IN THIS PROBE'S PYTHON: a set
    and a dict of ints) and the same number of deletes as kwok_pod_rec12 DELETE
    records through kwok_ingest_pods_packed12.

usage: sweep_probe.py [--nodes 1000000] [--reps 3]   (its own time limit: --limit seconds)"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ["KWOK_INGEST_PROF"] = "1"
import torch  # noqa: E402,F401  (the HIP runtime the engine binds)

import list_probe as lp  # noqa: E402
from kwok_amd import abi, engine as keng, workload  # noqa: E402
from kwok_amd.codec import Codec  # noqa: E402

PODS = abi.KIND_PODS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=540)
    a = ap.parse_args()
    signal.alarm(a.limit)  # the probe's own time limit
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
    def stamps():
        log.flush()
        log.seek(0)
        text = log.read().decode(errors="replace")
        log.seek(0)
        log.truncate()
        return text

    med = lambda xs: float(np.median(xs))  # noqa: E731
    e, fl, ph = workload.build_engine_fleet(keng.Engine, a.nodes, heartbeat_once=True)
    e.tick(workload.S0 + 30, read=False)
    n_slots = workload.BUCKETS * fl.cp
    used, _phase, _hip, pip = e.dump_pods(0, n_slots)
    live = np.nonzero(used)[0].astype(np.int32)
    rng = np.random.default_rng(1)
    out = dict(workload="relist with Replace, %d nodes x %d pods, heartbeat-once" % (a.nodes, len(live)), pods=int(len(live)))

    # ---- the mark cost
    codec = Codec(manage_all_nodes=True)
    n_page = min(1_000_000, len(live))
    body = lp.list_body("pods", lp.docs("pods", n_page))
    idx, hv = np.arange(n_page, dtype=np.uint32), live[:n_page].copy()
    ms = {True: [], False: []}
    for r in range(a.reps + 1):  # (one untimed round first), alternating
        for sess in (True, False):
            if sess:
                e.resync_begin(PODS)
            _frames, _info, _nh, sid = e.frame_list(body, cap=n_page)
            t0 = time.perf_counter()
            _hs, st, _rel, _nh2 = e.ingest_pods_framed(codec, sid, idx, hv)
            dt = (time.perf_counter() - t0) * 1e3
            assert not st.any()
            if sess:
                e.resync_end(PODS)
            if r:
                ms[sess].append(dt)
    out["mark_cost"] = dict(page_pods=n_page, framed_ingest_ms_session=med(ms[True]), framed_ingest_ms_none=med(ms[False]))
    stamps()

    # ---- the sweep, and the path without it
    out["sweep"] = []
    for frac in (0.0, 0.01, 0.10):
        rec = dict(absent_frac=frac, runs=[])
        for r in range(a.reps):
            k = int(len(live) * frac)
            absent = np.sort(rng.choice(live, k, replace=False)) if k else live[:0]
            present = np.setdiff1d(live, absent)
            e.resync_begin(PODS)
            assert e.resync_mark(PODS, present) == 0
            stamps()
            t0 = time.perf_counter()
            swept, _rel, _nd = e.resync_sweep(PODS, cap=k + 1)
            call = (time.perf_counter() - t0) * 1e3
            assert len(swept) == k
            txt = stamps()
            m = re.search(r"k_sweep_count \+ k_frame_scan ([\d.]+) ms(?:, k_sweep_emit ([\d.]+) ms, apply chain \+ results ([\d.]+) ms)?", txt)
            live = present
            rec["runs"].append(dict(swept=k, call_ms=call, count_scan_ms=float(m[1]), emit_ms=float(m[2] or 0),
                                    apply_chain_ms=float(m[3] or 0)))
        # bytes a pass reads: 2-byte state + 1-byte mark per slot below the fill marks (~ the live pods, rounded up to
        # 8 per bucket); emit also 4 + 2 bytes and writes 28 per swept pod
        nbytes = 3 * (len(live) + int(len(live) * frac))
        R = rec.pop("runs")
        rec.update(swept=R[-1]["swept"], pass_bytes=nbytes, call_ms=med([x["call_ms"] for x in R]),
                   count_scan_ms=med([x["count_scan_ms"] for x in R]), emit_ms=med([x["emit_ms"] for x in R]),
                   apply_chain_ms=med([x["apply_chain_ms"] for x in R]))
        rec["count_scan_GBps"] = nbytes / rec["count_scan_ms"] / 1e6
        if rec["emit_ms"]:
            rec["emit_GBps"] = (nbytes + 34 * rec["swept"]) / rec["emit_ms"] / 1e6
        # k_frame_count + k_frame_scan over as many bytes, in the same run
        stream = np.full(nbytes, 32, np.uint8)
        stream[-1] = 10
        fc = []
        for _ in range(a.reps + 1):
            stamps()
            e.frame_watch(stream, cap=2)
            fm = re.search(r"k_frame_count \+ k_frame_scan ([\d.]+) ms", stamps())
            fc.append(float(fm[1]))
        rec["frame_count_scan_ms"] = med(fc[1:])
        rec["frame_count_scan_GBps"] = nbytes / rec["frame_count_scan_ms"] / 1e6
        if frac:  # the caller's path without the sweep (one round: the host diff takes seconds)
            k = int(len(live) * frac)
            gone = np.sort(rng.choice(live, k, replace=False))
            listed_ids = np.setdiff1d(live, gone).tolist()
            uid_map = dict(zip(live.tolist(), live.tolist()))
            t0 = time.perf_counter()
            listed = set(listed_ids)
            t1 = time.perf_counter()
            diff = [h for u, h in uid_map.items() if u not in listed]
            t2 = time.perf_counter()
            assert len(diff) == k
            recs = np.zeros(k, abi.POD_REC12_DTYPE)
            recs["op"] = abi.OP_DELETE
            recs["target"] = np.array(diff, np.int32)
            recs["value"] = pip[recs["target"]]
            t3 = time.perf_counter()
            _nh, st, _rel = e.ingest_pods_packed12(recs)
            t4 = time.perf_counter()
            assert not st.any()
            live = np.setdiff1d(live, gone)
            del uid_map, listed, listed_ids
            rec["without_sweep"] = dict(deletes=k, python_set_of_listed_uids_ms=(t1 - t0) * 1e3,
                                        python_walk_of_uid_map_ms=(t2 - t1) * 1e3, packed12_deletes_ms=(t4 - t3) * 1e3)
        out["sweep"].append(rec)
    out["resync_stats"] = e.resync_stats()
    e.close()
    codec.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
