#!/usr/bin/env python3
"""The reference directory on the metric fleet, heartbeat-once engines.

  1. kwok_read_refs over the initial tick's pod-patch (10 per node) and node-init lists, in
     pieces of --piece items, and over a C4 step's delete and pod-patch lists: wall time per
     call; the kernels' own times come from the engine's event stamps (KWOK_INGEST_PROF: the
     "[kwok refs]" lines on stderr);
  2. kwok_ingest_pods_framed_uid over the C4 step's frames (N deletion-marked pods, N creates,
     tools/uid_probe.py's step) on an engine with the directory and on one without, the same
     stream on both in every step, the order alternating;
  3. the device memory the directory holds (kwok_refs_stats).

--pmc: the initial tick's reads alone, for a `rocprofv3 --pmc FETCH_SIZE --kernel-trace` run of
its own; --summarise DIR prints k_refs_gather's counter from such a run against the byte model
(per item: 2 bytes of the length array, the record's 16-byte units in use, the uid's 8-byte
words).  The last line on stdout is one JSON object.

usage: ref_probe.py [--nodes 1000000] [--steps 6] [--piece 1048576] [--pmc] | --summarise DIR"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("KWOK_INGEST_PROF", "1")

NS = b"default"
NAME_LEN, UID_LEN = 12, 36  # "pod-%08d", tools/uid_probe.py's uids


def model_bytes(n_items, ns_len=len(NS), name_len=NAME_LEN, uid_len=UID_LEN):
    units = (ns_len + name_len + 15) // 16
    return n_items * (2 + 16 * units + 8 * ((uid_len + 7) // 8))


def summarise(d):
    rows = {}
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if row["Counter_Name"] == "FETCH_SIZE" and "k_refs_" in row["Kernel_Name"]:
                name = row["Kernel_Name"].split("k_refs_")[1].split("(")[0]
                rows.setdefault("k_refs_" + name, []).append((int(row["Dispatch_Id"]), float(row["Counter_Value"]) * 1024.0,
                                                              int(row.get("Grid_Size", 0) or 0)))
    out = {}
    for k, v in rows.items():
        v.sort()
        out[k] = [{"fetch_size_bytes": b, "grid_threads": g} for _d, b, g in v]
    print(json.dumps(out))


def bind_names(e, handles, serials):
    """kwok_refs_bind: pod handles[i] becomes default/pod-<serial % 10^8>"""
    from kwok_amd import workload
    h = np.ascontiguousarray(handles, np.int32)
    n = len(h)
    rows = np.empty((n, len(NS) + NAME_LEN), np.uint8)
    rows[:, :len(NS)] = np.frombuffer(NS, np.uint8)
    rows[:, len(NS):len(NS) + 4] = np.frombuffer(b"pod-", np.uint8)
    rows[:, len(NS) + 4:] = workload._digits(np.asarray(serials, np.int64) % 10 ** 8, 8)
    arena = np.ascontiguousarray(rows).reshape(-1)
    ns_off = np.arange(n, dtype=np.uint64) * rows.shape[1]
    nm_off = ns_off + len(NS)
    ns_len, nm_len = np.full(n, len(NS), np.uint32), np.full(n, NAME_LEN, np.uint32)
    bad = C.c_size_t()
    rc = e._lib.kwok_refs_bind(e._h, h.ctypes.data, arena.ctypes.data, ns_off.ctypes.data, ns_len.ctypes.data, nm_off.ctypes.data,
                               nm_len.ctypes.data, n, C.byref(bad))
    e._check(rc, "refs_bind")
    assert bad.value == 0, bad.value


class Reader:
    """kwok_read_refs into buffers allocated once (page-locked)"""

    def __init__(self, keng, abi, e, piece):
        self.e, self.abi, self.piece = e, abi, piece
        self.refs = keng.host_array((piece,), abi.REF_DTYPE)
        self.blob = keng.host_array((piece * 96,), np.uint8)

    def read(self, which, total):
        """the whole list in pieces -> (per-call wall ms, items, blob bytes)"""
        ms, nbytes = [], 0
        for lo in range(0, total, self.piece):
            cnt = min(self.piece, total - lo)
            used = C.c_size_t()
            t0 = time.perf_counter()
            rc = self.e._lib.kwok_read_refs(self.e._h, which, lo, cnt, self.refs.ctypes.data, self.blob.ctypes.data, self.blob.nbytes,
                                            C.byref(used))
            ms.append((time.perf_counter() - t0) * 1e3)
            self.e._check(rc, "read_refs")
            nbytes += used.value
            assert (self.refs["status"][:cnt] == 0).all(), "every item of the list has a name"
        return ms, total, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--piece", type=int, default=1 << 20)
    ap.add_argument("--limit", type=int, default=540)
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--summarise", default="")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    signal.alarm(a.limit)  # the probe's own time limit
    import torch  # noqa: F401  (the HIP runtime the engine binds)
    from kwok_amd import abi, engine as keng, workload
    from kwok_amd.codec import Codec
    from uid_probe import OLD, UidChurn, bind_fleet
    from watch_probe import HEAD, TAIL, as_stream

    n = a.nodes
    say = lambda s: print("---- " + s, file=sys.stderr, flush=True)  # noqa: E731
    on, fl, pods = workload.build_engine_fleet(keng.Engine, n, heartbeat_once=True)
    on.refs_enable()
    t0 = time.perf_counter()
    bind_fleet(on, pods)
    for lo in range(0, len(pods), 1 << 20):
        h = pods[lo:lo + (1 << 20)]
        bind_names(on, h, OLD + np.asarray(h, np.int64))
    bind_ms = (time.perf_counter() - t0) * 1e3
    mem = on.refs_stats()["bytes"]
    now = workload.S0 + 30
    res = on.tick(now, read=False)
    rd = Reader(keng, abi, on, a.piece)
    out = {"fleet": "%d nodes x %d pods" % (n, len(pods)), "piece": a.piece, "bind_uids_and_names_ms": bind_ms,
           "refs_bytes_held": mem, "bytes_per_pod_slot": abi.REF_STRIDE + 2}
    say("the initial tick: %d pod patches, %d node inits" % (res.n_pod_patch, res.n_node_init))
    reads = {}
    for rep in range(2):  # (the second pass: buffers grown, the lists warm)
        reads["pod_patch"] = rd.read(abi.REFS_POD_PATCH, res.n_pod_patch)
        reads["node_init"] = rd.read(abi.REFS_NODE_INIT, res.n_node_init)
    items = keng.Engine.ref_items(rd.refs[:2], rd.blob)
    assert items[0][0] == 0 and len(items[0][2]) == fl.names.shape[1], items[0]  # (the last read: node inits)
    out["initial_tick"] = {k: {"items": v[1], "blob_bytes": v[2], "call_ms": v[0], "total_ms": sum(v[0])} for k, v in reads.items()}
    out["model_bytes_per_pod_item"] = model_bytes(1)
    if a.pmc:
        on.close()
        print(json.dumps(out), flush=True)
        return
    # ---- the C4 step on an engine with the directory and on one without ----
    off, fl2, pods2 = workload.build_engine_fleet(keng.Engine, n, heartbeat_once=True)
    assert (pods2 == pods).all()
    off.uid_dir_enable()
    bind_fleet(off, pods2)
    off.tick(now, read=False)
    n_handles = workload.BUCKETS * fl.cp
    ch = UidChurn(pods, np.repeat(fl.node_handles, workload.PODS_PER_NODE), 0, n_handles, n, seed=7, alloc=keng.host_array,
                  node_name_of=workload.node_names_by_handle(fl))
    ch.start(n_handles)
    codec = Codec(manage_all_nodes=True)
    dump = lambda: on.dump_pods(0, n_handles)  # noqa: E731
    sbuf = None
    t = {"ingest_on": [], "ingest_off": [], "read_delete": [], "read_pod_patch": [], "lists": []}
    for k in range(a.steps + 2):  # (two untimed steps first)
        now += 30
        arena, offs, lens, ops, handles = ch.batch_json(dump, now)
        if sbuf is None:
            sbuf = keng.host_array((int(lens.sum()) + (len(HEAD) + len(TAIL)) * len(lens),), np.uint8)
        stream = as_stream(arena, lens, sbuf)
        idx = np.arange(len(lens), dtype=np.uint32)
        got = {}
        order = (("on", on), ("off", off)) if k % 2 == 0 else (("off", off), ("on", on))
        say("step %d: %s first" % (k, order[0][0]))
        for tag, e in order:
            frames, used, _nh, sid = e.frame_watch(stream, cap=len(lens))
            assert len(frames) == len(lens) and used == stream.nbytes
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            hs, st, _rel, _nh2, _runs = e.ingest_pods_framed_uid(codec, sid, idx)
            got[tag] = ((time.perf_counter() - t1) * 1e3, hs, st)
        assert (got["on"][1] == got["off"][1]).all() and (got["on"][2] == got["off"][2]).all() and not got["on"][2].any()
        r_on = on.tick(now, read=False)
        r_off = off.tick(now, read=False)
        assert (r_on.n_delete, r_on.n_pod_patch) == (r_off.n_delete, r_off.n_pod_patch)
        rdl = rd.read(abi.REFS_DELETE, r_on.n_delete)
        rpp = rd.read(abi.REFS_POD_PATCH, r_on.n_pod_patch)
        ch.applied(got["on"][1].copy(), got["on"][2])
        if k >= 2:
            t["ingest_on"].append(got["on"][0])
            t["ingest_off"].append(got["off"][0])
            t["read_delete"].append(sum(rdl[0]))
            t["read_pod_patch"].append(sum(rpp[0]))
            t["lists"].append((r_on.n_delete, r_on.n_pod_patch))
    med = lambda v: float(np.median(v)) if v else None  # noqa: E731
    out["c4_step"] = {"steps_ms": t, "median_ms": {k: med(v) for k, v in t.items() if k != "lists"},
                      "ingest_off_spread_ms": max(t["ingest_off"]) - min(t["ingest_off"]) if t["ingest_off"] else None,
                      "ingest_on_minus_off_ms": med(t["ingest_on"]) - med(t["ingest_off"]) if t["ingest_on"] else None}
    out["refs_stats"] = on.refs_stats()
    out["note"] = "device times of k_refs_size / the scan / k_refs_gather: the [kwok refs] lines above; k_refs_note has no stamp of its own"
    on.close()
    off.close()
    codec.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
