"""GPU: the echo ledger itself (include/kwok_watch.h; echo.hip), through
kwok_echo_update and kwok_echo_match.  The yardstick is controller.Echoes driven with the
same sequence under _encode's rule (Mirror below), compared after every call: every
status, the drop mask and every kwok_echo_stats counter the host can state.  The table
is forced to 64 entries (KWOK_ECHO_TAB_LOG2=6) so that probes chain, wrap the table's
end and meet emptied entries.

Not tested: the refusal of kwok_echo_enable on a multi-rank engine (no forced-multi
fixture is at hand in one process)."""
import numpy as np
import pytest

from kwok_amd import abi
from kwok_amd.controller import Echoes
from kwok_amd.engine import Engine, KwokError, make_config

pytestmark = pytest.mark.gpu

KW = dict(cidr="10.0.0.1/16", node_ip="196.168.0.1", buckets=64, node_slots_per_bucket=32, pod_slots_per_bucket=64)
N, F = abi.ECHO_NOTE, abi.ECHO_FORGET
HOST_STATS = ("notes", "forgets", "evictions", "matched", "dropped", "kept_matched", "live_uids")


class Mirror:
    """the host rule: Echoes as Controller._apply / _encode / _ingest_frames use it, and what they would count"""

    def __init__(self):
        self.echo = Echoes()
        self.s = dict.fromkeys(HOST_STATS, 0)

    def update(self, ops, uids, rvs):
        st = []
        for op, u, r in zip(ops, uids, rvs):
            if len(u) > abi.UID_MAX or (op == N and len(r) > abi.RV_MAX):
                st.append(abi.EDOMAIN)
                continue
            st.append(abi.OK)
            if op == N:
                if u and r:
                    self.s["notes"] += 1
                    self.s["evictions"] += len(self.echo.rv.get(u, ())) == Echoes.ECHO_KEEP
                self.echo.note(u, r)
            else:
                self.s["forgets"] += u in self.echo.rv
                self.echo.forget(u)
        self.s["live_uids"] = len(self.echo.rv)
        return st

    def match(self, uids, rvs, deleted):
        seen, drop = set(), []
        for u, r, d in zip(uids, rvs, deleted):
            if d:
                seen.add(u)
                self.s["forgets"] += u in self.echo.rv
                self.echo.forget(u)
                drop.append(0)
                continue
            m = self.echo.is_echo(u, r)
            self.s["matched"] += m
            if m and u not in seen:
                self.s["dropped"] += 1
                drop.append(1)
                continue
            self.s["kept_matched"] += m
            seen.add(u)
            drop.append(0)
        self.s["live_uids"] = len(self.echo.rv)
        return drop


class Rig:
    def __init__(self, monkeypatch, log2=6, enable=True):
        if log2:
            monkeypatch.setenv("KWOK_ECHO_TAB_LOG2", str(log2))
        else:
            monkeypatch.delenv("KWOK_ECHO_TAB_LOG2", raising=False)
        self.e = Engine(make_config(**KW))
        self.m = Mirror()
        if enable:
            self.e.echo_enable()

    def stats(self, where):
        got = self.e.echo_stats()
        assert {k: got[k] for k in HOST_STATS} == self.m.s, where
        assert got["table_entries"] >= got["live_uids"], where
        return got

    def update(self, ops, uids, rvs, where):
        got = self.e.echo_update(ops, uids, rvs)
        assert list(got) == self.m.update(ops, uids, rvs), where
        self.stats(where)
        return got

    def note(self, pairs, where):
        return self.update([N] * len(pairs), [u for u, _r in pairs], [r for _u, r in pairs], where)

    def match(self, recs, where):
        """recs: (uid, rv, deleted)"""
        u, r, d = [x[0] for x in recs], [x[1] for x in recs], [bool(x[2]) for x in recs]
        got = self.e.echo_match(u, r, d)
        want = self.m.match(u, r, d)
        assert list(got) == want, "%s\n%r\n%r" % (where, list(got), want)
        self.stats(where)
        return list(got)


def uids_of(n, seed=0):
    """uids of length 1, 36 and 40, two equal in their first 39 bytes, the rest UUID-shaped"""
    rng = np.random.default_rng(seed)
    out = [b"a", b"b", b"x" * 39 + b"1", b"x" * 39 + b"2", b"y" * 40, b"y" * 39]
    while len(out) < n:
        h = rng.bytes(16).hex()
        out.append(("%s-%s-%s-%s-%s" % (h[:8], h[8:12], h[12:16], h[16:20], h[20:])).encode())
    assert len(set(out)) == len(out)
    return out[:n]


def test_the_rule_on_one_uid(monkeypatch):
    r = Rig(monkeypatch)
    u = b"3f2b8c1e-9d4a-4b6f-8e21-0a1b2c3d4e5f"
    # nine notes: the first no longer matches, the other eight do, each once
    r.note([(u, b"%d" % (100 + k)) for k in range(9)], "nine notes")
    assert r.e.echo_stats()["evictions"] == 1
    assert r.match([(u, b"100", 0)], "the evicted note") == [0]
    for k in range(1, 9):
        assert r.match([(u, b"%d" % (100 + k), 0)], "note %d" % k) == [1]
        assert r.match([(u, b"%d" % (100 + k), 0)], "note %d again" % k) == [0]
    assert r.e.echo_stats()["live_uids"] == 0
    # one rv noted twice matches twice
    r.note([(u, b"7"), (u, b"7")], "twice")
    assert r.match([(u, b"7", 0)], "first") == [1]
    assert r.match([(u, b"7", 0)], "second") == [1]
    assert r.match([(u, b"7", 0)], "third") == [0]
    # ... in one call too: both are dropped (no record of the uid was kept before them), the third is kept
    r.note([(u, b"8"), (u, b"8")], "twice, one call")
    assert r.match([(u, b"8", 0), (u, b"8", 0), (u, b"8", 0)], "both in one call") == [1, 1, 0]
    # a match consumed by a kept record: a real change first, then the echo in the same call
    r.note([(u, b"21"), (u, b"22")], "seen")
    assert r.match([(u, b"20", 0), (u, b"21", 0)], "echo behind a kept record") == [0, 0]
    assert r.match([(u, b"21", 0)], "consumed") == [0]
    assert r.match([(u, b"22", 0), (u, b"23", 0)], "echo before a kept record") == [1, 0]
    s = r.e.echo_stats()
    assert s["kept_matched"] == 1
    # Deleted forgets, is never an echo, and puts the uid into seen
    r.note([(u, b"31"), (u, b"32")], "before the delete")
    assert r.match([(u, b"31", 1), (u, b"32", 0)], "deleted") == [0, 0]
    assert r.e.echo_stats()["live_uids"] == 0
    r.note([(u, b"33"), (u, b"34")], "again")
    assert r.match([(u, b"33", 0), (u, b"33", 1), (u, b"34", 0)], "echo, deleted, forgotten") == [1, 0, 0]
    # forget then note inside one update call (the tick's delete list before the finalizer patch's note), and the reverse
    r.note([(u, b"41")], "stale")
    r.update([F, N], [u, u], [b"", b"42"], "forget then note")
    assert r.match([(u, b"41", 0), (u, b"42", 0)], "only the later note") == [0, 0]  # (41 is kept: 42 follows a kept record)
    r.update([N, F, N, N, F], [u] * 5, [b"51", b"", b"52", b"53", b""], "note, forget, notes, forget")
    assert r.match([(u, b"53", 0)], "all forgotten") == [0]
    r.update([N, F, N], [u] * 3, [b"61", b"", b"62"], "the last note stays")
    assert r.match([(u, b"62", 0)], "62") == [1]
    assert r.match([(u, b"61", 0)], "61") == [0]
    r.e.close()


def test_keys_at_the_domain_edges(monkeypatch):
    r = Rig(monkeypatch)
    us = uids_of(8)
    rv24, rv1 = b"9" * 24, b"5"
    r.note([(u, rv1) for u in us] + [(u, rv24) for u in us] + [(u, rv24[:23]) for u in us], "lengths 1 / 23 / 24")
    # a 41-byte uid and a 25-byte rv: KWOK_EDOMAIN, nothing stored (never truncated); empty uid / rv: ignored
    st = r.update([N, N, N, N, F, F], [b"z" * 41, us[4], b"", us[0], b"z" * 41, b""], [b"1", b"9" * 25, b"1", b"", b"", b""],
                  "outside the domain")
    assert list(st) == [abi.EDOMAIN, abi.EDOMAIN, abi.OK, abi.OK, abi.EDOMAIN, abi.OK]
    n0 = r.e.echo_stats()["notes"]
    assert n0 == 24
    # never an echo: the truncations and extensions of what is stored, an empty uid, an empty rv
    probes = [(b"z" * 40, b"1", 0), (b"z" * 41, b"1", 0), (us[4], b"9" * 25, 0), (us[4][:38], rv1, 0), (us[2][:39], rv1, 0),
              (b"", b"1", 0), (b"", rv1, 0), (us[0], b"", 0), (us[1], b"55", 0), (us[1], b"", 0)]
    assert r.match(probes, "near misses") == [0] * len(probes)
    # the prefix and the full rv are two notes; the uids equal in 39 bytes are two uids
    assert r.match([(us[2], rv24[:23], 0)], "the prefix") == [1]
    assert r.match([(us[3], rv24, 0)], "the whole") == [1]
    assert r.match([(us[2], rv24, 0), (us[3], rv24[:23], 0)], "the others") == [1, 1]
    assert r.match([(u, rv1, 0) for u in us], "length 1") == [1] * 8  # (the near misses consumed nothing)
    r.e.close()


def test_chains_wraps_rebuilds_and_the_full_table(monkeypatch):
    r = Rig(monkeypatch)
    us = uids_of(48, seed=1)
    # 48 uids in 64 entries: probes chain past their home entries and wrap the table's end (the mirror says what is right)
    r.note([(u, b"1") for u in us], "48 uids")
    s = r.e.echo_stats()
    assert s["table_entries"] == 48 and s["live_uids"] == 48 and s["rebuilds"] == 0
    others = uids_of(80, seed=2)[6:]
    assert r.match([(u, b"1", 0) for u in others[:40]], "strangers") == [0] * 40
    assert r.match([(u, b"1", 0) for u in us[:40]], "40 echoes") == [1] * 40
    # note / match cycles: emptied entries pile up until a rebuild compacts them; every answer stays right
    gone = []
    for c in range(8):
        cyc = [b"cycle-%d-%d" % (c, i) for i in range(10)]
        r.note([(u, b"%d" % c) for u in cyc], "cycle %d noted" % c)
        assert r.match([(u, b"1", 0) for u in gone[-10:]] + [(u, b"%d" % c, 0) for u in cyc], "cycle %d" % c) == \
            [0] * len(gone[-10:]) + [1] * 10
        gone += cyc
    s = r.e.echo_stats()
    assert s["rebuilds"] >= 1 and s["live_uids"] == 8 and s["table_entries"] < 64
    assert r.match([(u, b"1", 0) for u in us[40:]], "the 8 that stayed through the rebuilds") == [1] * 8
    # the forced table cannot hold 64 uids: refused before anything is stored
    before = r.e.echo_stats()
    with pytest.raises(KwokError) as ei:
        r.e.echo_update([N] * 64, [b"full-%d" % i for i in range(64)], [b"1"] * 64)
    assert ei.value.code == abi.EFULL
    assert r.e.echo_stats() == before
    assert r.match([(b"full-0", b"1", 0), (b"full-63", b"1", 0)], "after the refusal") == [0, 0]
    r.note([(b"fits-%d" % i, b"1") for i in range(60)], "60 fit")
    assert r.match([(b"fits-%d" % i, b"1", 0) for i in range(60)], "60 echoes") == [1] * 60
    r.e.close()


def test_growth_without_a_forced_table(monkeypatch):
    r = Rig(monkeypatch, log2=0)
    us = uids_of(700, seed=3)
    r.note([(u, b"1") for u in us[:20]], "20")
    assert r.e.echo_stats()["rebuilds"] == 0
    r.note([(u, b"2") for u in us[:300]], "300: past the 64 entries it starts with")
    r.note([(u, b"3") for u in us[100:700]], "700")
    s = r.e.echo_stats()
    assert s["rebuilds"] >= 2 and s["live_uids"] == 700 and s["table_entries"] == 700
    want = [1] * 20 + [0] * 680
    assert r.match([(u, b"1", 0) for u in us], "rv 1") == want
    assert r.match([(u, b"3", 0) for u in us], "rv 3") == [0] * 100 + [1] * 600
    assert r.match([(u, b"2", 0) for u in us], "rv 2") == [1] * 300 + [0] * 400
    assert r.e.echo_stats()["live_uids"] == 0
    r.e.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_block_edges(monkeypatch, n):
    """one thread per record, 256 per block: n distinct uids, then n records of ONE uid"""
    r = Rig(monkeypatch, log2=0)
    us = [b"edge-%d" % i for i in range(n)]
    r.note([(u, b"1") for u in us], "%d notes" % n)
    assert r.match([(u, b"1", 0) for u in us], "%d echoes" % n) == [1] * n
    # n notes on one uid: the last ECHO_KEEP stay.  n records of it in one call, oldest first: past 8 the first
    # record matches nothing and is kept, so the 8 that match behind it are consumed and kept too
    one = b"one-uid"
    r.note([(one, b"%d" % k) for k in range(n)], "%d notes on one uid" % n)
    recs = [(one, b"%d" % k, 0) for k in range(n)]
    got = r.match(recs, "%d records of one uid" % n)
    assert got == ([1] if n == 1 else [0] * n)
    assert r.e.echo_stats()["live_uids"] == 0
    r.note([(one, b"7")] * 3, "three equal notes")
    assert r.match([(one, b"7", 0)] * n, "%d equal records" % n) == ([1] * 3 + [0] * n)[:n]
    r.e.close()


def test_fuzz(monkeypatch):
    """mixed updates and matches over 40 uids and 6 rvs in a 64-entry table, ~60 calls of up to 90 records:
    repeats of a uid inside a call are the rule, every call is compared"""
    r = Rig(monkeypatch)
    rng = np.random.default_rng(5)
    us = uids_of(40, seed=4)
    rvs = [b"1", b"22", b"333", b"9" * 24, b"9" * 23, b""]
    pick = lambda a: a[int(rng.integers(0, len(a)))]  # noqa: E731
    for c in range(60):
        n = int(rng.integers(1, 90))
        hot = us[:int(rng.integers(1, 41))]
        if rng.integers(0, 2):
            ops = [F if rng.integers(0, 5) == 0 else N for _ in range(n)]
            r.update(ops, [pick(hot) for _ in range(n)], [pick(rvs) for _ in range(n)], "fuzz update %d" % c)
        else:
            r.match([(pick(hot), pick(rvs), rng.integers(0, 8) == 0) for _ in range(n)], "fuzz match %d" % c)
    s = r.e.echo_stats()
    assert s["matched"] > 100 and s["dropped"] > 50 and s["kept_matched"] > 10 and s["evictions"] > 10 and s["forgets"] > 10
    r.e.close()


def test_calls_without_the_ledger(monkeypatch):
    r = Rig(monkeypatch, enable=False)
    for call in (lambda: r.e.echo_update([N], [b"u"], [b"1"]), lambda: r.e.echo_match([b"u"], [b"1"], [0])):
        with pytest.raises(KwokError) as ei:
            call()
        assert ei.value.code == abi.EINVAL
    assert r.e.echo_stats() == dict.fromkeys(abi.ECHO_STATS, 0)
    r.e.echo_enable()
    r.e.echo_enable()  # idempotent
    assert list(r.e.echo_match([b"u"], [b"1"], [0])) == [0]
    assert list(r.e.echo_update([], [], [])) == [] and list(r.e.echo_match([], [], [])) == []
    r.e.close()
