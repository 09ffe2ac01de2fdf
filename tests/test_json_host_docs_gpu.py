"""GPU: the documents k_json_pods lists for the host (JSON_HOST, JSON_SPEC, JSON_SPEC_X) and json_complete
(kwok_amd/csrc/engine.cpp) completes, through every JSON entry point of the pod ingest, against the host
codec and the CPU oracle - never against a second engine on the same path.

The corpus is tests/host_docs.py (proved sound on the CPU by tests/test_host_docs_cpu.py).  Each scenario
runs once per entry point:
  json    kwok_ingest_pods_json
  framed  kwok_frame_watch_gpu + kwok_ingest_pods_framed, handles from the test's own uid map
  uid     kwok_frame_watch_gpu + kwok_ingest_pods_framed_uid
  echo    kwok_frame_watch_gpu + kwok_ingest_pods_framed_echo with an empty ledger (nothing is dropped)
  list    kwok_frame_list_gpu + kwok_ingest_pods_framed_uid for the create-only batches (the others by uid)
After every call: statuses, handles and released addresses equal the oracle's document for document, and
n_host equals the corpus' stated count - which keeps the test on the host-completion branch.  After every
batch: kwok_register_pod_spec of every spec seen so far answers the first-appearance order of the documents
(the oracle's ids), then a tick compared output by output and on the pod state; two ticks after the last
batch, so the patches of the host-completed creates are compared byte for byte."""
import numpy as np
import pytest

import host_docs as hd
import watch_frames as wf
from gpu_common import compare, compare_state
from kwok_amd import abi
from kwok_amd.codec import Codec
from kwok_amd.engine import Engine, make_config
from oracle.oracle import Oracle
from test_uid_ingest_gpu import KW

pytestmark = pytest.mark.gpu

ENTRIES = ["json", "framed", "uid", "echo", "list"]


def call(e, codec, entry, b, sent):
    """one batch through the entry point -> (handles, statuses, released, n_host)"""
    docs = [l.doc for l in b.lines]
    n = len(docs)
    if entry == "json":
        arena, offs, lens = Engine._docs(docs)
        ops = np.array([abi.OP_DELETE if l.type == "DELETED" else abi.OP_UPSERT for l in b.lines], np.uint8)
        return e.ingest_pods_json(codec, arena, offs, lens, ops, sent)
    if entry == "list" and b.create_only:
        body = b'{"kind":"PodList","apiVersion":"v1","metadata":{"resourceVersion":"7"},"items":[' + b",".join(docs) + b"]}"
        frames, _info, _nh, sid = e.frame_list(body)
    else:
        frames, _used, _nh, sid = e.frame_watch(b"".join(wf.wrap(l.doc, l.type) for l in b.lines))
    assert len(frames) == n and not frames["status"].any()
    idx = np.arange(n)
    if entry == "framed":
        return e.ingest_pods_framed(codec, sid, idx, sent)
    if entry == "echo":
        h, s, r, nh, runs, dropped = e.ingest_pods_framed_echo(codec, sid, idx)
        assert dropped == 0
    else:
        h, s, r, nh, runs = e.ingest_pods_framed_uid(codec, sid, idx)
    assert runs == 1  # (uids are unique within a batch: n_host is that of one decode)
    return h, s, r, nh


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(hd.SCENARIOS))
def test_host_completed_documents(name, entry, monkeypatch):
    assert hd.KW == KW
    sc = hd.SCENARIOS[name]()
    if sc.key_bits:  # (read when a spec is registered and when a decode is launched: set before the engine exists)
        monkeypatch.setenv("KWOK_DEBUG_SPEC_KEY_BITS", str(sc.key_bits))
    ref = hd.Ref(sc)
    e = Engine(make_config(**KW))
    reg = lambda s: e.register_pod_spec([tuple(x) for x in s[0]], [tuple(x) for x in s[1]], list(s[2]))  # noqa: E731
    assert [reg(s) for s in sc.pre_specs] == [ref.spec_id[s] for s in sc.pre_specs]
    h, st = e.ingest_nodes_raw(*hd.node_events())
    assert not st.any() and list(h) == list(ref.node_handles)
    if entry in ("uid", "echo", "list"):
        e.uid_dir_enable()
    if entry == "echo":
        e.echo_enable()
    now = hd.T0

    def tick(where):
        nonlocal now
        compare(e.tick(now), ref.o.tick(now), where)
        compare_state(e, ref.o, ref.n_slots, where)
        now += 30

    for b in sc.batches:
        where = "%s / %s through %s" % (name, b.name, entry)
        sent, want_h, want_st, want_rel, _decoded = ref.expect(b)
        assert list(want_st) == [l.status for l in b.lines], where  # (the corpus' statement, as on the CPU)
        got_h, got_st, got_rel, n_host = call(e, ref.codec, entry, b, sent)
        print("%s: n_host %d (stated %d), statuses other than the oracle's: %d of %d" % (
            where, n_host, b.n_host, int((np.asarray(got_st) != want_st).sum()), len(b.lines)))
        assert list(got_st) == list(want_st), "%s statuses\n%r\n%r" % (where, list(got_st), list(want_st))
        assert list(got_h) == list(want_h), "%s handles\n%r\n%r" % (where, list(got_h), list(want_h))
        assert list(got_rel) == list(want_rel), where + " released"
        assert n_host == b.n_host > 0, "%s: %d documents listed for the host, %d stated" % (where, n_host, b.n_host)
        # spec ids: the first-appearance order of the documents, as the oracle's registration gives
        assert [reg(s) for s in ref.spec_id] == list(ref.spec_id.values()), where + " spec ids"
        tick(where)
    tick(name + " settled")
    tick(name + " steady")
    for s in sc.unseen:  # a spec only a Deleted line's object showed was never registered: it takes the next id
        assert reg(s) == ref.register(s) == len(ref.spec_id) - 1, name
    e.close()
    ref.close()


def test_arena_longer_than_the_scanner_addresses_is_refused():
    """arena_len above KWOK_JSON_ARENA_MAX: KWOK_EINVAL before any byte is read (json.hip scans with 32-bit
    positions), from kwok_ingest_pods_json and kwok_decode_pods_gpu alike; the engine ticks on as the oracle"""
    import ctypes as C
    e = Engine(make_config(**KW))
    o = Oracle(make_config(**KW))
    codec = Codec(manage_all_nodes=True)
    buf = bytes(16)
    nh = C.c_size_t(7)
    too_long = 0xFFFFFFF1
    lib = e._lib
    rc = lib.kwok_ingest_pods_json(e._h, codec._h, buf, too_long, None, None, None, None, 0, None, None, None, C.byref(nh))
    assert rc == abi.EINVAL
    rc = lib.kwok_decode_pods_gpu(e._h, codec._h, buf, too_long, None, None, 0, None, None, None, None, C.byref(nh))
    assert rc == abi.EINVAL
    # (the limit itself passes the guard: with no documents nothing is read)
    assert lib.kwok_ingest_pods_json(e._h, codec._h, buf, 0xFFFFFFF0, None, None, None, None, 0, None, None, None,
                                     C.byref(nh)) == 0
    ev, arena = hd.node_events(["n0"])
    h, st = e.ingest_nodes_raw(ev, arena)
    h2, st2 = o.ingest_nodes_raw(ev, arena)
    assert not st.any() and not st2.any() and list(h) == list(h2)
    for k in range(2):
        compare(e.tick(hd.T0 + 30 * k), o.tick(hd.T0 + 30 * k), "after the refused calls, tick %d" % k)
    codec.close()
    o.close()
    e.close()
