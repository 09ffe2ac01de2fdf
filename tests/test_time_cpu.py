"""CPU: time values at the edges of the supported domain (a
time is the 20 bytes YYYY-MM-DDTHH:MM:SSZ naming a real calendar date, and lies
in [0, 2^32) unix seconds; anything else is KWOK_EDOMAIN).

The yardstick is Python's datetime / calendar.timegm, which shares no code with
the engine's civil-date arithmetic (codec.cpp parse_time, json.hip jtime,
kernels.hip format_ts) nor with the oracle's libc gmtime_r.  Every constant is
built from datetime here, and each family asserts the property it was chosen
for.  tests/test_time_gpu.py runs the same documents through the device.

- the host codec (Codec.decode_pods) decodes a creationTimestamp at the probe's
  seconds (0, 1, both sides of 2000-02-29, of 2^31, of 2100-01-01 and of
  2100-03-01, and 2^32 - 1: PROBE), at the first
  and last second of every month of the years around the domain's edges and the
  Gregorian rule's (1970, 1999, 2000, 2023, 2024, 2038, 2099, 2100, 2105), at
  2106-02-07T06:28:15Z (2^32 - 1), at 0001-01-01 and 9999-12-31 (decoded here,
  refused at ingest) and at seeded random seconds, to calendar.timegm's value;
- it refuses with KWOK_EDOMAIN dates no calendar holds (the valid-or-not table is
  datetime() raising ValueError), clock fields out of range and malformed text:
  time.Parse(time.RFC3339), metav1.Time's decoder, refuses them all;
- the oracle renders every timestamp of every patch as datetime does, over the
  same seconds, ticking at now = start_time = 2^32 - 1, and refuses the times
  the engine refuses with the engine's code."""
import calendar
import json
from datetime import datetime, timedelta

import numpy as np
import pytest

from kwok_amd import abi
from kwok_amd.codec import Codec
from kwok_amd.engine import KwokError, make_config
from oracle.oracle import Oracle

EPOCH = datetime(1970, 1, 1)
LAST = 2 ** 32 - 1
YEARS = (1970, 1999, 2000, 2023, 2024, 2038, 2099, 2100, 2105)


def stamp(dt):
    """RFC3339 in UTC, whole seconds (strftime's %Y does not pad the year 1)"""
    return "%04d-%02d-%02dT%02d:%02d:%02dZ" % (dt.year, dt.month, dt.day, dt.hour, dt.minute, dt.second)


def secs(dt):
    return calendar.timegm(dt.timetuple())


def at(t):
    return EPOCH + timedelta(seconds=int(t))


def rfc3339(t):
    return stamp(at(t))


def month_edges():
    """the first and the last second of every month of YEARS"""
    out = []
    for y in YEARS:
        for m in range(1, 13):
            first = datetime(y, m, 1)
            nxt = datetime(y + (m == 12), m % 12 + 1, 1)
            out += [first, nxt - timedelta(seconds=1)]
    return out


def valid_date(y, m, d, hh=0, mi=0, ss=0):
    try:
        datetime(y, m, d, hh, mi, ss)
        return True
    except ValueError:
        return False


# (year, month, day): day 00 and the days 28 to 31 of every month, months 00 and 13, of a
# common year, a leap year, and the century years that are (2000) and are not (2100) one.
# Which of them exist is datetime's word alone: no month length is written out here
CANDIDATES = [c for y in (2000, 2023, 2024, 2100)
              for c in [(y, m, d) for m in range(1, 13) for d in (0, 28, 29, 30, 31)] + [(y, 0, 10), (y, 13, 10)]]
IMPOSSIBLE = [c for c in CANDIDATES if not valid_date(*c)]
BESIDE = [c for c in CANDIDATES if valid_date(*c)]
# the seconds the issue's probe formats: both sides of everything a 32-bit word or a civil
# date can get wrong (the signed word's boundary, 2000's and 2100's 28 February, the
# 2099 -> 2100 year end, the domain's first and last seconds)
PROBE_DATES = [datetime(1970, 1, 1), datetime(1970, 1, 1, 0, 0, 1), datetime(2000, 2, 28, 23, 59, 59), datetime(2000, 2, 29),
               datetime(2038, 1, 19, 3, 14, 7), datetime(2038, 1, 19, 3, 14, 8), datetime(2099, 12, 31, 23, 59, 59),
               datetime(2100, 1, 1), datetime(2100, 2, 28, 23, 59, 59), datetime(2100, 3, 1),
               datetime(2106, 2, 7, 6, 28, 15)]
PROBE = [calendar.timegm(dt.timetuple()) for dt in PROBE_DATES]
# (hour, minute, second) out of range, and the last valid one
BAD_CLOCKS = [(0, 0, 60), (24, 0, 0), (0, 60, 0)]
GOOD_CLOCK = (23, 59, 59)
DIGITS = (0, 1, 2, 3, 5, 6, 8, 9, 11, 12, 14, 15, 17, 18)  # the 14 digit positions of the 20 bytes


def date_text(y, m, d, hh=0, mi=0, ss=0):
    return "%04d-%02d-%02dT%02d:%02d:%02dZ" % (y, m, d, hh, mi, ss)


def accepted():
    """[(text, unix seconds)] inside [0, 2^32): the probe's seconds, the month edges,
    the real dates beside the impossible ones, seeded random seconds"""
    dts = PROBE_DATES + month_edges() + [datetime(*c) for c in BESIDE] + [datetime(2024, 1, 1, *GOOD_CLOCK)]
    rng = np.random.default_rng(2106)
    dts += [at(t) for t in rng.integers(0, 2 ** 32, 300)]
    return [(stamp(dt), secs(dt)) for dt in dict.fromkeys(dts)]  # (each second once)


def far():
    """decoded by the codec, outside [0, 2^32): refused at ingest"""
    return [(stamp(dt), secs(dt)) for dt in (datetime(1, 1, 1), datetime(9999, 12, 31, 23, 59, 59))]


def rejected():
    """[(text, why)]: no calendar date, a clock field out of range, malformed text"""
    out = [(date_text(*c), "no such date") for c in IMPOSSIBLE]
    out += [(date_text(2024, 1, 1, *c), "clock field out of range") for c in BAD_CLOCKS]
    good = date_text(2024, 1, 1)
    out += [(good.replace("T", "t"), "lower-case t"), (good.replace("Z", "z"), "lower-case z"),
            (good[:-1] + "+00:00", "a numeric offset"), (good[:-1], "19 bytes"), (good[1:], "19 bytes"),
            (good + "Z", "21 bytes"), ("0" + good, "21 bytes"), (good.replace("T", " "), "a space for T")]
    for k in DIGITS:
        for ch in "/:":  # the characters next to '0' and '9'
            out.append((good[:k] + ch + good[k + 1:], "a non-digit at %d" % k))
    return out


SPEC = ([("c", "img"), ("d", "img/d:v2")], [("init", "busybox")], ["g.io/x"])


ORDER = ("apiVersion", "kind", "metadata", "spec", "status")


def echoed_status(ts):
    """the status pod.status.tpl renders for SPEC at the text ts, as the apiserver
    echoes it: the codec's no-op test compares its times with the creationTimestamp"""
    conds = [{"lastProbeTime": None, "lastTransitionTime": ts, "status": "True", "type": t}
             for t in ["Initialized", "Ready", "ContainersReady"] + SPEC[2]]
    cs = [{"image": i, "name": n, "ready": True, "restartCount": 0, "state": {"running": {"startedAt": ts}}}
          for n, i in SPEC[0]]
    ics = [{"image": i, "name": n, "ready": True, "restartCount": 0,
            "state": {"terminated": {"exitCode": 0, "finishedAt": ts, "reason": "Completed", "startedAt": ts}}}
           for n, i in SPEC[1]]
    return {"conditions": conds, "containerStatuses": cs, "initContainerStatuses": ics, "startTime": ts,
            "phase": "Running", "hostIP": "196.168.0.1", "podIP": "10.0.0.9", "podIPs": [{"ip": "10.0.0.9"}]}


def pod_document(ts, k, node="node-0", indent=None, order=ORDER, echo=False):
    """a scheduled Pending pod created at the text ts (containers, an init container
    and a readiness gate: every timestamp slot of pod.status.tpl is rendered);
    echo: a Running one whose status is the template's own (KWOK_POD_CONFORMS)"""
    d = {"apiVersion": "v1", "kind": "Pod",
         "metadata": {"name": "pod-%05d" % k, "namespace": "default", "creationTimestamp": ts, "uid": "u-%05d" % k,
                      "labels": {"app": "fake"}},
         "spec": {"nodeName": node, "containers": [{"name": n, "image": i} for n, i in SPEC[0]],
                  "initContainers": [{"name": n, "image": i} for n, i in SPEC[1]],
                  "readinessGates": [{"conditionType": g} for g in SPEC[2]]},
         "status": echoed_status(ts) if echo else {"phase": "Pending", "qosClass": "BestEffort"}}
    return json.dumps({key: d[key] for key in order}, indent=indent).encode()


def patch_times(patch):
    """every timestamp a pod patch renders: (startTime, [the others])"""
    st = json.loads(patch)["status"]
    rest = [c["lastTransitionTime"] for c in st["conditions"]]
    rest += [c["state"]["running"]["startedAt"] for c in st.get("containerStatuses", [])]
    for c in st.get("initContainerStatuses", []):
        rest += [c["state"]["terminated"]["startedAt"], c["state"]["terminated"]["finishedAt"]]
    return st["startTime"], rest


def test_the_constants_are_what_they_are_chosen_for():
    assert rfc3339(0) == "1970-01-01T00:00:00Z" and rfc3339(LAST) == "2106-02-07T06:28:15Z"
    edges = month_edges()
    assert len(edges) == 2 * 12 * len(YEARS)
    for first, last in zip(edges[0::2], edges[1::2]):
        assert (first.day, first.hour, first.minute, first.second) == (1, 0, 0, 0)
        assert (last.hour, last.minute, last.second) == (23, 59, 59) and (last + timedelta(seconds=1)).day == 1
        assert last.month == first.month and last.day == calendar.monthrange(first.year, first.month)[1]
    assert all(0 <= secs(dt) <= LAST for dt in edges)
    assert {dt.day for dt in edges if dt.month == 2 and dt.day > 1} == {28, 29}
    assert datetime(2100, 2, 28, 23, 59, 59) in edges and datetime(2100, 3, 1) in edges
    # the probe's seconds: pairs one second apart across each boundary, all in the set
    assert PROBE == [0, 1, 951782399, 951782400, 2 ** 31 - 1, 2 ** 31, 4102444799, 4102444800, 4107542399, 4107542400, LAST]
    assert [stamp(PROBE_DATES[k]) for k in (3, 9)] == ["2000-02-29T00:00:00Z", "2100-03-01T00:00:00Z"]  # leap, not leap
    assert np.int32(np.uint32(PROBE[5])) < 0 < np.int32(np.uint32(PROBE[4]))  # a signed word changes sign here
    assert [rfc3339(t) for t in PROBE] == [stamp(dt) for dt in PROBE_DATES]
    assert set(PROBE) <= {t for _, t in accepted()}
    # the dates: generated, with the ones the domain's sentence is about among them
    assert not any(valid_date(*c) for c in IMPOSSIBLE) and all(valid_date(*c) for c in BESIDE)
    named = ([(y, 2, d) for y in (2023, 2100) for d in (29, 30, 31)] + [(y, 2, d) for y in (2024, 2000) for d in (30, 31)] +
             [(2023, m, 31) for m in (4, 6, 9, 11)] + [(2024, 1, 0), (2024, 0, 10), (2024, 13, 10)])
    assert set(named) <= set(IMPOSSIBLE) and {(2024, 2, 29), (2000, 2, 29), (2100, 2, 28), (2023, 12, 31)} <= set(BESIDE)
    assert len(IMPOSSIBLE) + len(BESIDE) == len(CANDIDATES) == 4 * (12 * 5 + 2)
    assert not any(valid_date(2024, 1, 1, *c) for c in BAD_CLOCKS) and valid_date(2024, 1, 1, *GOOD_CLOCK)
    acc = accepted()
    assert len({s for s, _ in acc}) == len(acc)
    assert all(len(s) == 20 and 0 <= t <= LAST and rfc3339(t) == s for s, t in acc)
    assert sum(t >= 2 ** 31 for _, t in acc) > 100
    assert [t for _, t in far()] == [-62135596800, 253402300799]
    rej = rejected()
    assert len({s for s, _ in rej}) == len(rej) and not {s for s, _ in rej} & {s for s, _ in acc}
    good = date_text(2024, 1, 1)
    assert [k for k in range(20) if good[k].isdigit()] == list(DIGITS)
    assert sum(why.startswith("a non-digit") for _, why in rej) == 2 * 14
    assert {len(s) for s, why in rej if why.endswith("bytes")} == {19, 21}


def test_host_codec_decodes_the_calendar():
    codec = Codec()
    cases = accepted() + far()
    b = codec.decode_pods([pod_document(s, k, indent=(None, 1)[k % 2]) for k, (s, _) in enumerate(cases)], strict=False)
    bad = [(s, t, st, d.ev.creation_unix) for (s, t), st, d in zip(cases, b.status, b.pods)
           if st != abi.OK or d.ev.creation_unix != t]
    assert not bad, "%d of %d, first %r" % (len(bad), len(cases), bad[0])
    assert not any(d.ev.flags & abi.POD_CONFORMS for d in b.pods)
    # the apiserver's echo of the template's status: its times equal the creationTimestamp's text
    b = codec.decode_pods([pod_document(s, k, echo=True) for k, (s, _) in enumerate(cases)], strict=False)
    assert all(st == abi.OK and d.ev.creation_unix == t and d.ev.flags & abi.POD_CONFORMS
               for (s, t), st, d in zip(cases, b.status, b.pods))


def test_host_codec_rejects_what_no_calendar_holds():
    """KWOK_EDOMAIN, nothing decoded: no creation time, no spec.  (On the parent
    commit the impossible dates decoded with KWOK_OK, 2023-02-30 to the seconds of
    2023-03-02.)"""
    codec = Codec()
    cases = rejected()
    b = codec.decode_pods([pod_document(s, k) for k, (s, _) in enumerate(cases)], strict=False)
    bad = [(s, why, st) for (s, why), st in zip(cases, b.status) if st != abi.EDOMAIN]
    assert not bad, "%d of %d not refused, first %r" % (len(bad), len(cases), bad[0])
    assert all(d.ev.creation_unix == 0 and d.n_containers == 0 for d in b.pods)


KW = dict(cidr="10.0.0.1/16", node_ip="196.168.0.1", buckets=64, node_slots_per_bucket=16, pod_slots_per_bucket=128)


def oracle_fleet(start_time, n_nodes=40):
    o = Oracle(make_config(start_time=start_time, **KW))
    spec = o.register_pod_spec(*SPEC)
    ar = abi.Arena()
    ev = np.zeros(n_nodes, abi.NODE_EVENT_DTYPE)
    ev["op"], ev["managed"], ev["lockable"] = abi.OP_UPSERT, 1, 1
    for i in range(n_nodes):
        ev[i]["name"] = ar.ref("node-%d" % i)
    nh, st = o.ingest_nodes_raw(ev, bytes(ar.buf))
    assert (st == 0).all()
    return o, spec, nh


def creates(times, spec, nh):
    ev = np.zeros(len(times), abi.POD_EVENT_DTYPE)
    ev["op"], ev["handle"], ev["spec_id"] = abi.OP_UPSERT, -1, spec
    ev["node_handle"] = nh[np.arange(len(times)) % len(nh)]
    ev["phase"], ev["flags"] = abi.PHASE_PENDING, abi.POD_STATUS_NONEMPTY
    ev["creation_unix"] = times
    return ev


def test_oracle_renders_the_calendar():
    cases = accepted()
    o, spec, nh = oracle_fleet(LAST)
    hs, st, _ = o.ingest_pods_raw(creates([t for _, t in cases], spec, nh), b"")
    assert (st == 0).all()
    want = {int(h): s for h, (s, _) in zip(hs, cases)}
    out = o.tick(LAST)
    assert len(out.pod_patches) == len(cases) and len(out.heartbeat_nodes) == len(nh)
    for h, patch in out.pod_patches:
        start, rest = patch_times(patch)
        assert start == want[h] and len(rest) == 4 + 2 + 2 and set(rest) == {want[h]}, (h, want[h], patch)
    body = json.loads(out.heartbeat_body(0))
    conds = body["status"]["conditions"]
    assert len(conds) >= 4 and {c["lastHeartbeatTime"] for c in conds} == {rfc3339(LAST)}
    assert {c["lastTransitionTime"] for c in conds} == {rfc3339(LAST)}  # (start_time)
    assert out.heartbeat_body(0).count(b"2106-02-07T06:28:15Z") == 2 * len(conds)
    o.close()


def test_oracle_refuses_times_outside_the_domain():
    """creation times per record, now per tick, start_time at creation: the codes
    the engine returns (tests/test_time_gpu.py pins the engine's)"""
    o, spec, nh = oracle_fleet(0, n_nodes=2)
    hs, st, _ = o.ingest_pods_raw(creates([0, -1, LAST, 2 ** 32, 1], spec, nh), b"")
    assert list(st) == [abi.OK, abi.EDOMAIN, abi.OK, abi.EDOMAIN, abi.OK] and hs[1] == hs[3] == -1
    assert int(o.dump_pods(0, 64 * 128)[0].sum()) == 3
    for now in (-1, 2 ** 32):
        with pytest.raises(KwokError) as ei:
            o.tick(now)
        assert ei.value.code == abi.EDOMAIN, now
    out = o.tick(0)  # (the refused ticks ticked nothing: the three pods are still to patch)
    assert len(out.pod_patches) == 3 and json.loads(out.heartbeat_body(0))["status"]["conditions"][0][
        "lastHeartbeatTime"] == rfc3339(0)
    o.close()
    for start in (-1, 2 ** 32):
        with pytest.raises(KwokError) as ei:
            Oracle(make_config(start_time=start, **KW))
        assert ei.value.code == abi.EDOMAIN, start
