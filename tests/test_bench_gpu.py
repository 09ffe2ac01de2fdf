"""GPU: bench.py's plain run and --dump-outputs on a small fleet.  The plain
run prints one result line with the headline fields and none of the --full
legs; the dumped arrays are float32 / float64, under 64 MB, and equal what the
oracle hands back for the same fleet at the last timed step's clock."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from kwok_amd import workload
from oracle.oracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODES, STEPS, WARMUP = 3000, 3, 2  # more nodes than bench.DUMP_BODIES: the body sample is a real sample


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(tmp_path):
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--nodes-per-rank", str(NODES), "--dump-outputs", d],
                       stdout=subprocess.PIPE, timeout=120)
    assert r.returncode == 0
    lines = r.stdout.decode().strip().splitlines()
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == STEPS and out["warmup"] == WARMUP and out["full"] is False
    assert out["unit"] == "transitions/s" and out["higher_is_better"] is True and out["dtype"] == "u8"
    assert out["ms_per_step"] > 0
    # a steady tick: one heartbeat per node, nothing else
    assert out["value"] == pytest.approx(NODES / (out["ms_per_step"] * 1e-3), rel=1e-9)
    for k in ("roofline", "churn", "flap", "heartbeat_once", "c2", "emulated_ranks", "cpu_baseline",
              "ms_per_step_kwok_tick", "ms_per_step_with_handoff"):
        assert k not in out, k

    got = {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(d, "*.npy"))}
    assert all(x.dtype in (np.float32, np.float64) for x in got.values())
    assert sum(x.nbytes for x in got.values()) <= 64 << 20

    o, _, _ = workload.build_engine_fleet(Oracle, NODES)
    for k in range(1, WARMUP + STEPS + 1):  # the initial tick, the other warmup steps, the timed steps
        res = o.tick(workload.S0 + 30 * k, read=False)
    want = o.read_arrays(res)
    o.close()
    assert list(got["counters"]) == list(res.counters)
    assert list(got["local_counters"]) == list(res.local_counters)
    assert np.array_equal(got["heartbeat_nodes"], want["heartbeat_nodes"]) and len(got["heartbeat_nodes"]) == NODES
    ln, st, off = want["heartbeat_len"], want["heartbeat_stride"], want["heartbeat_off"]
    bodies = np.stack([want["arena"][off + i * st:off + i * st + ln] for i in range(NODES)])
    assert np.array_equal(got["heartbeat_body_sums"], bodies.sum(axis=1, dtype=np.int64))
    rows = got["heartbeat_rows"].astype(np.int64)
    assert len(rows) < NODES and len(set(rows)) == len(rows)
    assert np.array_equal(got["heartbeat_bodies"], bodies[rows])
    # a steady tick has no patches and no deletes: sizes says so, and no empty file stands for them
    assert list(got["sizes"]) == [NODES, ln, 0, 0, 0]
    assert res.n_node_init == res.n_pod_patch == res.n_delete == 0
    assert all(x.size for x in got.values())
    assert sorted(got) == ["counters", "heartbeat_bodies", "heartbeat_body_sums", "heartbeat_nodes", "heartbeat_rows",
                           "local_counters", "sizes"]
