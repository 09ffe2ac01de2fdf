"""The delta heartbeat stream's resident share (KWOK_HB_KEEP, DevState::hb_keep).
A non-temporal delta tick stores hb_keep of every 64 groups of 4 slots with plain
stores (they stay in the Infinity Cache and are overwritten there) and the rest
non-temporally.  The policy changes no byte and no record, so every case here
is the pattern of test_hb_delta_gpu.py: the engine under test runs with
KWOK_HB_NT=1 KWOK_HB_KEEP=k in lockstep with a KWOK_HB_DELTA=0 engine (the full
stream) and the oracle, and after EVERY tick the whole heartbeat region
(n x stride, padding included) is compared with the full-stream engine's byte
for byte, the bodies with the oracle, and handles, counters and sizes with both.

Node counts sit around what the share's index arithmetic can get wrong: a
partial last group (1, 3, 5), one whole group (4), fewer than 64 groups (255
nodes = 64 groups with a partial last one, 256 = exactly 64), 64 groups and a
remainder (257) and more than one streamer share (1027).  Shares: none (0, the
all-non-temporal path), one group of 64, 31, all but one, and all of them.

The CPU test is of the host helper behind the automatic share: the dirty 64-byte
lines per body between two clocks (templates.h hb_dirty_lines_per_body)."""
import ctypes as C

import numpy as np
import pytest

from gpu_common import new_pods
from kwok_amd import engine
from test_hb_delta_gpu import SPECS, T0, Trio

gpu = pytest.mark.gpu
NODES = [1, 3, 4, 5, 255, 256, 257, 1027]
KEEP = [0, 1, 31, 63, 64]
SIZES = ("n_heartbeat", "heartbeat_len", "heartbeat_stride", "n_node_init", "n_pod_patch", "n_delete", "arena_bytes")
YEAR = 366 * 86400
# T0 is 2024-01-01T00:00:30Z.  30 s steps across a minute carry (00:01:00), the same clock
# twice (nothing to write), a step backwards, 30 s steps across an hour carry (00:59:30 ->
# 01:00:00 -> 01:00:30) ... (the sequences below go on from here)
QUIET = [T0, T0 + 30, T0 + 60, T0 + 60, T0 + 30, T0 + 3540, T0 + 3570, T0 + 3600]


class Keep(Trio):
    """test_hb_delta_gpu.Trio with KWOK_HB_NT=1 and KWOK_HB_KEEP=k (e; f is the
    KWOK_HB_DELTA=0 engine, which never reads the share), and a check that also
    compares handles, counters and sizes"""

    def __init__(self, monkeypatch, k, env=None, **kw):
        monkeypatch.setenv("KWOK_HB_KEEP", str(k))
        for name, v in (env or {}).items():
            monkeypatch.setenv(name, str(v))
        super().__init__(monkeypatch, 1, **kw)

    def check(self, now, where):
        E, n, st, ln = super().check(now, where)
        F = self.f.read_arrays()
        assert (E["heartbeat_nodes"] == F["heartbeat_nodes"]).all(), where + " heartbeat handles"
        assert E["counters"] == F["counters"], where + " counters"
        for x in [self.f] + ([self.o] if self.o is not None else []):
            assert list(self.e.last.local_counters) == list(x.last.local_counters), where + " local counters"
        for k in SIZES:
            assert getattr(self.e.last, k) == getattr(self.f.last, k), "%s: %s" % (where, k)
        return E, n, st, ln

    def stat_tick(self, now, where, delta=True):
        """one blocking tick; returns what the engine's path counters moved by"""
        s0 = self.e.stats()
        _, got, _, _ = self.tick(now, where, delta=delta)
        s1 = self.e.stats()
        return got, {k: s1[k] - s0[k] for k in s1}


@gpu
@pytest.mark.parametrize("k", KEEP)
@pytest.mark.parametrize("n", NODES)
def test_blocking_one_slot(n, k, monkeypatch):
    """one slot: k_tick (everything), one counting k_once_stream delta tick, reused k_hb_stream
    delta ticks over QUIET's clocks; then an ingest, whose tick is a k_tick delta tick; the quiet
    ticks after it until the count is reused again; and a jump of a year"""
    t = Keep(monkeypatch, k)
    spec = t.specs()
    nh = t.nodes(["node-%07d" % i for i in range(n)])
    reused = 0
    for i, now in enumerate(QUIET):
        got, d = t.stat_tick(now, "quiet tick %d (n=%d, keep=%d)" % (i, n, k), delta=i > 0)
        assert got == n
        reused += d["ticks_count_reused"]
        if i >= 2:
            assert d["ticks_count_reused"] == 1, "quiet tick %d was not a reused tick" % i
    ev, ar = new_pods(t.rng, nh, 40, spec)
    t.pods(ev, ar)
    now = QUIET[-1] + 30
    got, d = t.stat_tick(now, "tick after an ingest (n=%d, keep=%d)" % (n, k))
    assert got == n and d["ticks_once_stream"] == 0 and d["ticks_hb_delta"] == 1, "not a k_tick delta tick: %r" % d
    for i in range(5):
        now += 30
        got, d = t.stat_tick(now, "settling tick %d (n=%d, keep=%d)" % (i, n, k))
        if d["ticks_count_reused"]:
            break
    assert d["ticks_count_reused"] == 1, "no reused tick within 5 ticks of the ingest"
    got, d = t.stat_tick(now + YEAR, "a year later (n=%d, keep=%d)" % (n, k))
    assert got == n and d["ticks_count_reused"] == 1 and d["ticks_hb_delta"] == 1
    t.close()


@gpu
@pytest.mark.parametrize("k", KEEP)
@pytest.mark.parametrize("n", NODES)
def test_queued_two_slots(n, k, monkeypatch):
    """tick i+1 is submitted before tick i is collected: two slots, each one's previous bodies
    two ticks back.  30 s steps from 00:57:30 across minute carries and the hour carry, then for
    each slot the clock its bodies already have (nothing to write), a step backwards and a jump
    of a year; ticks 0 and 1 write everything, every later one is a delta, and from tick 3 on the
    count is reused (k_hb_stream)"""
    t = Keep(monkeypatch, k)
    t.nodes(["node-%07d" % i for i in range(n)])
    c = [T0 + 3420 + 30 * i for i in range(8)]  # 00:57:30 .. 01:01:00
    clocks = c + [c[6], c[7], c[5], c[7] + YEAR, c[7] + YEAR + 30]
    for x in (t.e, t.f):
        x.tick_submit(clocks[0])
    for i, now in enumerate(clocks):
        for x in (t.e, t.f):
            if i + 1 < len(clocks):
                x.tick_submit(clocks[i + 1])
            x.tick_collect(read=False)
        t.o.tick(now, read=False)
        s = t.e.stats()
        assert t.delta_ticks() == max(0, i - 1), "queued tick %d" % i
        assert s["ticks_count_reused"] == max(0, i - 2), "queued tick %d: %r" % (i, s)
        _, got, _, _ = t.check(now, "queued tick %d (n=%d, keep=%d)" % (i, n, k))
        assert got == n
    t.close()


@gpu
@pytest.mark.parametrize("k", KEEP)
@pytest.mark.parametrize("n", NODES)
def test_k_tick_delta_ticks(n, k, monkeypatch):
    """KWOK_ONCE_STREAM=0: every tick is k_tick's, whose streamers and chain blocks
    (KWOK_TICK_STREAM_SHARE=512: half the stream each) write the delta stream with the share"""
    t = Keep(monkeypatch, k, env={"KWOK_ONCE_STREAM": 0}, share=512)
    t.nodes(["node-%07d" % i for i in range(n)])
    for i, now in enumerate(QUIET + [QUIET[-1] + YEAR]):
        got, d = t.stat_tick(now, "k_tick tick %d (n=%d, keep=%d)" % (i, n, k), delta=i > 0)
        assert got == n and d["ticks_once_stream"] == 0 and d["ticks_count_reused"] == 0
    t.close()


@gpu
@pytest.mark.parametrize("queued", [False, True])
@pytest.mark.parametrize("n", [5, 257])
def test_custom_heartbeat_template(n, queued, monkeypatch):
    """heartbeat_a.tpl: 79 units per slot, not the default 67 (the kernels' GEN_HB
    instantiations); the bodies are the host template compiler's, the oracle renders none"""
    from test_template_cpu import tpl
    htext = tpl("heartbeat_a.tpl")
    t = Keep(monkeypatch, 31, oracle=False, node_heartbeat_template=htext)
    t.body = lambda now: engine.heartbeat_template_patch(htext, 1704067200, "196.168.0.1", now)
    t.nodes(["node-%07d" % i for i in range(n)])
    clocks = QUIET + [QUIET[-1] + YEAR]
    if not queued:
        for i, now in enumerate(clocks):
            _, got, st, ln = t.tick(now, "custom template tick %d" % i, delta=i > 0)
            assert got == n and ln == len(t.body(now)) and st // 16 != 67
    else:
        for x in (t.e, t.f):
            x.tick_submit(clocks[0])
        for i, now in enumerate(clocks):
            for x in (t.e, t.f):
                if i + 1 < len(clocks):
                    x.tick_submit(clocks[i + 1])
                x.tick_collect(read=False)
            assert t.delta_ticks() == max(0, i - 1), "queued tick %d" % i
            _, got, st, _ = t.check(now, "custom template queued tick %d" % i)
            assert got == n and st // 16 != 67
    assert t.e.stats()["ticks_count_reused"] > 0
    t.close()


def dirty_lines(prev, now, slots=(47, 235, 452, 672, 877), units=67):
    lib = engine.load_engine_lib()
    lib.kwok_hb_dirty_lines.restype = C.c_double
    lib.kwok_hb_dirty_lines.argtypes = [C.POINTER(C.c_uint16), C.c_uint32, C.c_uint32, C.c_int64, C.c_int64]
    a = (C.c_uint16 * len(slots))(*slots)
    return lib.kwok_hb_dirty_lines(a, len(slots), units, prev, now)


def test_dirty_lines_per_body():
    """the default template's Now values sit at 47, 235, 452, 672 and 877 of a 1072-byte body;
    a timestamp is YYYY-MM-DDTHH:MM:SSZ (tens of seconds: character 17, minutes: 15)"""
    assert dirty_lines(T0, T0) == 0
    assert dirty_lines(T0, T0 + 10) == 5  # 00:00:30 -> 00:00:40: seconds only, one line per Now value
    assert dirty_lines(T0, T0 + 60) == 5  # 00:00:30 -> 00:01:30: minutes only
    assert dirty_lines(T0 + 60, T0) == 5  # (backwards: the same characters)
    # 2024-01-01T00:00:30Z -> 2025-01-01T00:00:31Z: characters 3 and 18 differ, 15 bytes apart, at
    # o + 3 and o + 18 of every Now value o; body b of a group starts at 1072 b.  By hand, the
    # 64-byte lines (byte / 64) of those 40 bytes:
    #   body 0:   50,65 -> 0,1     238,253 -> 3     455,470 -> 7       675,690 -> 10      880,895 -> 13     : 6 lines
    #   body 1: 1122,1137 -> 17  1310,1325 -> 20  1527,1542 -> 23,24  1747,1762 -> 27    1952,1967 -> 30    : 6
    #   body 2: 2194,2209 -> 34  2382,2397 -> 37  2599,2614 -> 40     2819,2834 -> 44    3024,3039 -> 47    : 5
    #   body 3: 3266,3281 -> 51  3454,3469 -> 53,54  3671,3686 -> 57  3891,3906 -> 60,61  4096,4111 -> 64   : 7
    # 24 lines of the group's 67: four pairs straddle a line boundary
    assert dirty_lines(T0, T0 + YEAR + 1) == 24 / 4
    # no Now value, and a unit count past the kernels' largest: nothing
    assert dirty_lines(T0, T0 + 10, slots=()) == 0
    assert dirty_lines(T0, T0 + 10, units=81) == 0
