"""GPU: kwok_engine_destroy gives back what an engine took (engine.cpp; engine_impl.h DevArr /
Pinned / DevGroup: the scratch of the ingests, the codec, the framers and the directories
frees itself with the engine).

One small engine with every directory enabled takes 8 records through each framed path,
the directories' typed calls, a List body, a resync session and one tick, and is
destroyed.  The drop in free device memory while the first one is alive is its footprint.
After 20 more such engines in this process, free device memory is not lower than after the
first destroy by more than one footprint: a scratch group leaked per engine adds up past
that, the runtime's own bookkeeping does not.  Free memory is hipMemGetInfo's, read through
the engine library's own HIP runtime."""
import ctypes as C

import numpy as np
import pytest

from kwok_amd import abi
from kwok_amd.codec import Codec
from kwok_amd.engine import Engine, load_engine_lib, make_config
from test_scratch_regrow_gpu import SPEC, T0, node, pod, span, stream_of

pytestmark = pytest.mark.gpu

KW = dict(cidr="10.0.0.1/24", node_ip="196.168.0.1", buckets=8, node_slots_per_bucket=16, pod_slots_per_bucket=16,
          heartbeat_once=True)
N = 8


def free_bytes():
    free, total = C.c_size_t(), C.c_size_t()
    assert load_engine_lib().hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def one_engine(codec):
    """-> free device memory while the engine is alive, after its work"""
    e = Engine(make_config(**KW))
    e.register_pod_spec(*SPEC)
    e.refs_enable()
    e.echo_enable()
    idx = np.arange(N)
    # nodes and pods through every framed entry
    _f, _u, _nh, sid = e.frame_watch(stream_of([node(i) for i in range(N)], "ADDED"))
    hn, st, _nh, ne = e.ingest_nodes_framed_echo(codec, sid, idx)
    assert not st.any() and ne == 0
    assert not e.ingest_nodes_framed(codec, sid, idx)[1].any()
    stream = stream_of([pod(i) for i in range(N)], "ADDED")
    fr, _u, _nh, sid = e.frame_watch(stream)
    hp, st, _rel, _nh, runs = e.ingest_pods_framed_uid(codec, sid, idx)
    assert not st.any() and runs == 1 and len(set(hp)) == N
    assert not e.ingest_pods_framed(codec, sid, idx, hp)[1].any()
    uids = [span(stream, f, "uid") for f in fr]
    rvs = [span(stream, f, "resource_version") for f in fr]
    # the typed calls of the three directories
    assert not e.echo_update([abi.ECHO_NOTE] * N, uids, rvs).any()
    assert list(e.echo_match(uids[:4], rvs[:4], np.zeros(4, np.uint8))) == [1] * 4
    h2, st, _rel, _nh, _runs, ne = e.ingest_pods_framed_echo(codec, sid, idx)
    assert list(st) == [0] * 4 + [abi.ECHO] * 4 and ne == 4 and list(h2) == list(hp)
    assert e.uid_bind(hp, uids) == 0 and list(e.uid_lookup(uids)) == list(hp)
    assert e.refs_bind(hp, [b"ns"] * N, [b"p%d" % i for i in range(N)]) == 0
    assert [x[2] for x in Engine.ref_items(*e.refs_lookup(abi.KIND_PODS, hp))] == [b"p%d" % i for i in range(N)]
    # a List body, a resync session that sweeps half of the pods
    body = b'{"kind":"PodList","apiVersion":"v1","metadata":{"resourceVersion":"7"},"items":[' + b",".join(pod(i) for i in range(N)) + b"]}"
    fl, _info, _nh, sid = e.frame_list(body)
    assert len(fl) == N
    e.resync_begin(abi.KIND_PODS)
    assert e.resync_mark(abi.KIND_PODS, hp[:4]) == 0
    assert list(e.resync_sweep(abi.KIND_PODS)[0]) == sorted(hp[4:])
    e.tick(T0, read=False)
    e.read_outputs(heartbeat_once=True)
    alive = free_bytes()
    e.close()
    return alive


def test_twenty_more_engines_leave_free_memory_where_the_first_left_it():
    codec = Codec(manage_all_nodes=True)
    before = free_bytes()
    footprint = before - one_engine(codec)
    after_first = free_bytes()
    assert footprint > 0
    for _ in range(20):
        one_engine(codec)
    after_last = free_bytes()
    print("footprint %d bytes; free after the 1st destroy %d, after the 21st %d (%+d)" % (
        footprint, after_first, after_last, after_last - after_first))
    assert after_first - after_last <= footprint
    codec.close()
