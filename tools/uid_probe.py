#!/usr/bin/env python3
"""The pod uid directory at the C4 shape: per step the 2 x N pod
documents of one churn tick as watch frames on the metric fleet, heartbeat-once
engine - N deletion-marked pods the engine holds (their uids bound) and N creates.

In one run, alternating:
  * the host-map step: kwok_frame_watch_gpu, the caller's uid -> handle map, then
    kwok_ingest_pods_framed with the handle array (the step of tools/watch_probe.py;
    the map is the generator's own handle array, i.e. a lower bound of what a caller
    with a real map pays);
  * the by-uid step: kwok_frame_watch_gpu, then kwok_ingest_pods_framed_uid.

Device times of the uid kernels come from the engine's own event stamps
(KWOK_INGEST_PROF: the "[kwok uid]" lines on stderr, beside "[kwok watch]" with
k_frame_parse's time over the same frames).  The last line on stdout is one JSON
object with every step's wall times, the medians and the bytes the by-uid call no
longer moves over the link.

usage: uid_probe.py [--nodes 1000000] [--steps 6]   (its own time limit: --limit seconds)"""
import argparse
import ctypes as C
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
from kwok_amd.codec import Codec  # noqa: E402
from watch_probe import HEAD, TAIL, as_stream  # noqa: E402

UID_HEAD = b"0b7f2c2e-0000-4000-8000-"
OLD = 500_000_000_000  # serials of the fleet's initial pods: OLD + handle (the creates count from 0)


class UidChurn(workload.ChurnJson):
    """ChurnJson whose documents carry each pod's own uid: a deletion-marked pod the uid it was created with"""

    def start(self, n_handles):
        self.serial_of = OLD + np.arange(n_handles, dtype=np.int64)
        self.dead_next = True

    def names(self, n):
        if self.dead_next:
            s = self.serial_of[self.live[:n] - self.first]
        else:
            s = np.arange(self.serial, self.serial + n, dtype=np.int64)
            self.serial += n
            self.new_serials = s
        self.dead_next = not self.dead_next
        name = np.empty((n, 12), np.uint8)
        name[:, :4] = np.frombuffer(b"pod-", np.uint8)
        name[:, 4:] = workload._digits(s % 10 ** 8, 8)
        uid = np.broadcast_to(np.frombuffer(UID_HEAD, np.uint8), (n, 24))
        return name, np.concatenate([uid, workload._digits(s, 12)], axis=1), workload._digits(s % 10 ** 8, 8)

    def applied(self, hs, st):
        D = self._pending[0]
        super().applied(hs, st)
        self.serial_of[hs[D:] - self.first] = self.new_serials


def bind(e, handles, serials):
    """kwok_uid_bind: pod handles[i] gets the uid of serial serials[i]"""
    h = np.ascontiguousarray(handles, np.int32)
    rows = np.concatenate([np.broadcast_to(np.frombuffer(UID_HEAD, np.uint8), (len(h), 24)),
                           workload._digits(np.asarray(serials, np.int64), 12)], axis=1)
    arena = np.ascontiguousarray(rows).reshape(-1)
    offs = np.arange(len(h), dtype=np.uint64) * 36
    lens = np.full(len(h), 36, np.uint32)
    bad = C.c_size_t()
    rc = e._lib.kwok_uid_bind(e._h, h.ctypes.data, arena.ctypes.data, offs.ctypes.data, lens.ctypes.data, len(h), C.byref(bad))
    e._check(rc, "uid_bind")
    assert bad.value == 0, bad.value


def bind_fleet(e, pods):
    """the fleet's pods (created through kwok_pod_rec12: no uid) bound in pieces of 1M"""
    t0 = time.perf_counter()
    for lo in range(0, len(pods), 1 << 20):
        h = pods[lo:lo + (1 << 20)]
        bind(e, h, OLD + np.asarray(h, np.int64))
    return (time.perf_counter() - t0) * 1e3


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
    bind_ms = bind_fleet(e, pods)
    n_handles = workload.BUCKETS * fl.cp
    ch = UidChurn(pods, np.repeat(fl.node_handles, workload.PODS_PER_NODE), 0, n_handles, n, seed=7,
                  alloc=keng.host_array, node_name_of=workload.node_names_by_handle(fl))
    ch.start(n_handles)
    codec = Codec(manage_all_nodes=True)
    dump = lambda: e.dump_pods(0, n_handles)  # noqa: E731
    outs = (keng.host_array((2 * n,), np.int32), keng.host_array((2 * n,), np.int32), keng.host_array((2 * n,), np.uint32))
    sbuf = None
    res = {"map": [], "uid": [], "frame": [], "host_map": [], "ingest_framed": [], "frame_uid": [], "ingest_uid": [], "runs": []}
    for k in range(a.steps + 2):  # (two untimed steps first, one of each kind)
        now += 30
        arena, offs, lens, ops, handles = ch.batch_json(dump, now)
        by_uid = k % 2 == 1
        if sbuf is None:
            sbuf = keng.host_array((int(lens.sum()) + (len(HEAD) + len(TAIL)) * len(lens),), np.uint8)
        stream = as_stream(arena, lens, sbuf)
        torch.cuda.synchronize()
        print("---- step %d: %s" % (k, "by uid" if by_uid else "host map"), file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        frames, used, nh, sid = e.frame_watch(stream, cap=len(lens))
        t1 = time.perf_counter()
        assert len(frames) == len(lens) and used == stream.nbytes
        idx = np.arange(len(frames), dtype=np.uint32)
        if by_uid:
            t2 = t1
            hs, st, _rel, nh2, runs = e.ingest_pods_framed_uid(codec, sid, idx)
            res["runs"].append(runs)
        else:
            # the caller's uid -> handle map: here the generator's (frame i is document i)
            hv = np.ascontiguousarray(handles, np.int32)
            t2 = time.perf_counter()
            hs, st, _rel, nh2 = e.ingest_pods_framed(codec, sid, idx, hv, out=outs)
        t3 = time.perf_counter()
        assert (hs[:n] == handles[:n]).all(), "the deletion-marked pods resolve to their handles"
        e.tick(now, read=False)
        ch.applied(hs.copy(), st)
        if not by_uid:  # the pods the host-map step created have no uid on the device: bound, outside the timed part
            bind(e, hs[len(lens) // 2:], ch.new_serials)
        if k >= 2:
            res["uid" if by_uid else "map"].append((t3 - t0) * 1e3)
            if by_uid:
                res["frame_uid"].append((t1 - t0) * 1e3)
                res["ingest_uid"].append((t3 - t1) * 1e3)
            else:
                res["frame"].append((t1 - t0) * 1e3)
                res["host_map"].append((t2 - t1) * 1e3)
                res["ingest_framed"].append((t3 - t2) * 1e3)
    med = lambda v: float(np.median(v)) if v else None  # noqa: E731
    nrec = 2 * n
    out = {"workload": "C4 as watch frames: %d deletion-marked + %d created pod documents per step" % (n, n),
           "documents_per_step": nrec, "stream_bytes": int(stream.nbytes), "bind_fleet_ms": bind_ms,
           "host_map_step_ms": res["map"], "by_uid_step_ms": res["uid"],
           "host_map_parts_ms": {"frame_watch_gpu": res["frame"], "map": res["host_map"], "ingest_pods_framed": res["ingest_framed"]},
           "by_uid_parts_ms": {"frame_watch_gpu": res["frame_uid"], "ingest_pods_framed_uid": res["ingest_uid"]},
           "median_ms": {"host_map": med(res["map"]), "by_uid": med(res["uid"]),
                         "ingest_pods_framed": med(res["ingest_framed"]), "ingest_pods_framed_uid": med(res["ingest_uid"])},
           "host_map_spread_ms": (max(res["map"]) - min(res["map"])) if res["map"] else None,
           "runs_per_by_uid_step": res["runs"],
           # per record: the host-map call uploads span (8 + 4), op (1), handle (4) and the frame index stays on the host;
           # the by-uid call uploads the frame index (4)
           "link_bytes_per_call": {"ingest_pods_framed_up": nrec * 17, "ingest_pods_framed_uid_up": nrec * 4,
                                   "no_longer_crossing": nrec * 13},
           "uid_stats": e.uid_stats(), "watch_stats": e.watch_stats(),
           "note": "device times of k_uid_resolve / k_uid_claim + k_uid_cut / k_uid_note and of k_frame_parse: the "
                   "[kwok uid] / [kwok watch] lines above"}
    e.close()
    codec.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
