"""The drop-in controller: the reference's Controller API over the engine.

This is the Python restatement of the Go drop-in
(integration/go/pkg/kwok/controllers/gpu_controller.go + engine_cgo.go), call
for call, so that its ingest / tick / apply sequence runs in the tests against
a fake clientset (tests/fake_clientset.py) the way the reference's unit tests
run NodeController / PodController against client-go's fake clientset
(node_controller_test.go:37-155, pod_controller_test.go:37-194).

Reference interface it stands in for (hezhizhen/kwok, pkg/kwok/controllers):
  Config                 controller.go:64-77
  NewController / Start  controller.go:80-164 (the loop replaces KeepNodeHeartbeat
                         node_controller.go:175-204, LockNodes :301-329, LockPods
                         pod_controller.go:234-250, DeletePods :186-202)
  Has / Size             node_controller.go:403-409
  watch routing          node_controller.go:256-270, pod_controller.go:301-343
                         (the host codec, kwok_decode_*, then kwok_ingest_*)
  apply                  PatchStatus node_controller.go:152,345; Patch status
                         pod_controller.go:221; finalizer Patch + Delete :161-174

Per tick (step):
  1. the watch events since the last tick, minus the ECHOES of the engine's own
     patches: an event whose resourceVersion is the one a patch of the engine
     returned for that object is the state the engine already assumed (DESIGN.md
     §1: patches are assumed applied; the heartbeat echo's re-lock,
     node_controller.go:152 -> :256-263, is part of every tick), so it is dropped
     instead of re-ingested.  Echoes that arrive after their patch returned are
     dropped on arrival (not queued, not encoded); those that overtake their
     patch's response are dropped here, when every apply has returned.  An echo
     that follows another event of its object in the same batch is kept: that
     event is a change the engine has not seen, older than the patch, and the
     echo is the newest state, carrying both;
  2. node events -> JSON -> kwok_decode_nodes -> kwok_ingest_nodes;
  3. pod events -> JSON -> kwok_decode_pods -> kwok_ingest_pods, in runs in which
     no new pod appears twice (a pod's second event needs the handle its first
     one created: Added + Modified, Added + Deleted in one interval);
  4. EnableCNI: cni.Setup for the pods the tick will evaluate without a podIP
     (kwok_cni_pending / kwok_cni_assign, pod_controller.go:383-389);
  5. kwok_tick at the fixed clock; the lists (kwok_read_outputs without an arena),
     ONE heartbeat body (the engine is created with KWOK_CFG_HEARTBEAT_ONCE) sent
     to every managed node, node-init and pod patches read in pieces of at most
     READ_CHUNK bytes (kwok_read_arena), deletes; every body applied through the
     clientset, every returned resourceVersion noted as an echo;
  6. the same interval again for pods patched without a podIP (created with an
     empty status: pod.status.tpl renders no IPs then, `{{ with .status }}`):
     in the reference that patch's own Modified event re-enters lockPodChan
     (pod_controller.go:279-319) and the pod gets hostIP / podIP at once.  Here
     the object the patch returned is ingested as that event (its watch echo is
     then dropped like every echo) and the engine ticks again at the same clock;
     that tick's pod patches, node inits and deletes are applied, its heartbeats
     are not (the interval's heartbeats were sent).

The backend is the HIP engine; tests may pass another implementation of the
same ABI (the CPU oracle) as the checker.

feed_list takes one complete page of a List response (the reference's ListNodes /
ListPods at Start): at step each kind's pages are framed on the GPU
(kwok_frame_list_gpu, include/kwok_watch.h) and their items ingested as upserts
from the resident body, before that kind's events; list_cursor[kind] then holds the
page's resourceVersion and continue token.

feed_watch is the same controller fed with the raw bytes of the watch responses
(a rest.Request.Stream read loop instead of the typed watcher): step 1-3 then
run on frames (include/kwok_watch.h) - the stream of each kind is framed on the
GPU (kwok_frame_watch_gpu), echoes are dropped by the frames' uid and
resourceVersion, and the kept frames are ingested from the resident stream
(kwok_ingest_nodes_framed / kwok_ingest_pods_framed, pods in the same runs): no
object is decoded or serialised on the host.

response_bytes=True (with the uid directory and the echo ledger) keeps step 5's
responses bytes too: the clientset's patch_*_raw methods return each patch's response
body, a tick's bodies are framed on the GPU (kwok_frame_responses_gpu), the echo notes
are taken from the frames (kwok_echo_note_framed) and step 6's pods re-enter from the
resident bytes (kwok_ingest_pods_framed_uid): DESIGN.md §27.

node_status_gpu=True lets the device canonicalise the status blobs of the node
documents it decodes (kwok_canon_enable, include/kwok_canon.h): a node kwok has
patched - every node of a relist - is decoded with no host codec call: DESIGN.md §28.
"""
from __future__ import annotations

import ctypes as C
import json
from dataclasses import dataclass, field

import numpy as np

from . import abi
from .codec import Codec, list_text
from .engine import Engine, KwokError, make_config

READ_CHUNK = 64 << 20  # engine_cgo.go readChunk

HEARTBEAT, NODE_INIT, POD_PATCH, DELETE, DELETE_FIN = range(5)  # engine_cgo.go kind*


NOT_SENT = 1  # ingest_pod_runs: a record not sent to the engine (a Deleted event of an unknown pod)


def ingest_pods_wire(eng, recs, arena):
    """engine_cgo.go ingestPods: every record the compact wire forms can carry
    (kwok_pack_pod_events: IPs as integers, a new pod's node by handle) as a
    12-byte kwok_pod_rec12 through kwok_ingest_pods_packed12 when its hostIP is
    empty or the engine's NodeIP (every pod kwok runs) and it is no create
    holding a podIP, else as a 20-byte kwok_pod_rec through
    kwok_ingest_pods_packed, and the rest (a pod naming a node the engine holds
    no handle for) as kwok_pod_event through kwok_ingest_pods; consecutive
    records of one form in one call, in event order (applying the calls in order
    is applying the batch).  Returns (handles, statuses, released, calls)."""
    from .engine import pack_pod_events
    packed, pst = pack_pod_events(recs, arena)
    n = len(recs)
    node_ip = eng.node_ip
    ok = pst == abi.OK
    hip = packed["host_ip"]
    new = (packed["op"] & abi.REC_NEW) != 0
    small = ((hip == 0) | (hip == node_ip)) & ~(new & (packed["pod_ip"] != 0))
    form = np.where(ok, np.where(small, 12, 20), 0)
    hs, st, rel = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.uint32)
    i = calls = 0
    while i < n:
        f = form[i]
        j = i + 1
        while j < n and form[j] == f:
            j += 1
        if f == 12:
            r12 = abi.pack12(packed[i:j], node_ip)
            nh, st[i:j], rel[i:j] = eng.ingest_pods_packed12(r12)
            nw = (r12["op"] & abi.REC_NEW) != 0
            hs[i:j] = r12["target"]  # every other record's handle is its target
            hs[i:j][nw] = nh
        elif f == 20:
            hs[i:j], st[i:j], rel[i:j] = eng.ingest_pods_packed(packed[i:j])
        else:
            hs[i:j], st[i:j], rel[i:j] = eng.ingest_pods_raw(recs[i:j], arena)
        calls += 1
        i = j
    return hs, st, rel, calls


def ingest_pod_runs(eng, pod_by_uid, recs, uids, deleted, arena, sender=None):
    """gpu_controller.go flushPods' ingest, on decoded records: the batch in
    event order, cut into runs in which no new pod appears twice - a pod's first
    event in the batch may create it (handle -1) and its later events need that
    handle, so run k+1 is ingested once run k's handles are known (Added +
    Modified, or Added + Deleted with its podIP release, pod_controller.go:
    329-336, within one interval).  A Deleted event names the pod's handle; one
    for a pod the engine never held (or already deleted) is not sent.  recs:
    POD_EVENT_DTYPE with spec_id / node_handle set for upserts (op and handle are
    set here); uids: hashable per record; pod_by_uid: the caller's uid -> handle
    map, updated.  Returns (handles, statuses, runs): per record, NOT_SENT for
    those not sent.  sender(idx, ops, handles) -> (handles, statuses): another
    ingest of the records idx (the documents on the GPU codec, ingest_doc_runs);
    recs is then only its length."""
    n = len(recs)
    uids = list(uids)
    deleted = np.asarray(deleted, bool)
    hs = np.full(n, -1, np.int32)
    st = np.full(n, NOT_SENT, np.int32)
    runs = 0

    def flush(lo, hi):
        nonlocal runs
        idx = np.arange(lo, hi)
        hv = np.fromiter((pod_by_uid.get(uids[i], -1) for i in range(lo, hi)), np.int64, hi - lo)
        dl = deleted[lo:hi]
        send = ~dl | (hv >= 0)
        idx, hv, dl = idx[send], hv[send], dl[send]
        if not len(idx):
            return
        ops = np.where(dl, abi.OP_DELETE, abi.OP_UPSERT)
        if sender is not None:
            h1, s1 = sender(idx, ops, hv)
        else:
            recs["op"][idx] = ops
            recs["handle"][idx] = hv
            h1, s1, _rel, _calls = ingest_pods_wire(eng, recs[idx], arena)
        runs += 1
        hs[idx], st[idx] = h1, s1
        for k in np.nonzero(s1 == abi.OK)[0].tolist():
            i = int(idx[k])
            if dl[k]:
                pod_by_uid.pop(uids[i], None)
            else:
                pod_by_uid[uids[i]] = int(h1[k])

    lo, created = 0, set()
    for i in range(n):
        u = uids[i]
        if u in created:  # its handle comes from the run before
            flush(lo, i)
            lo = i
            created.clear()
        if not deleted[i] and u not in pod_by_uid:
            created.add(u)
    flush(lo, n)
    return hs, st, runs


def ingest_doc_runs(eng, codec, pod_by_uid, docs, uids, deleted):
    """gpu_controller.go flushPodsJSON: the batch's pod documents decoded on the
    GPU (kwok_ingest_pods_json: k_json_pods, the host codec only for the
    documents the device leaves undecided, specs registered as they appear, the
    records never leaving HBM), in the same runs as ingest_pod_runs.  Returns
    (handles, statuses, runs, documents the host decided)."""
    arena, offs, lens = Engine._docs(docs)
    n_host = [0]

    def send(idx, ops, hv):
        hs, st, _rel, nh = eng.ingest_pods_json(codec, arena, offs[idx], lens[idx], ops.astype(np.uint8),
                                                hv.astype(np.int32))
        n_host[0] += nh
        return hs, st

    hs, st, runs = ingest_pod_runs(eng, pod_by_uid, np.empty(len(docs)), uids, deleted, None, sender=send)
    return hs, st, runs, n_host[0]


class NotFound(Exception):
    """apierrors.IsNotFound: tolerated by LockPod / DeletePod (pod_controller.go:164,174,224)"""


@dataclass
class Config:
    """controller.go:64-77 (Go field names in snake case).  Templates: None =
    templates.Default*.  start_time: the StartTime() value (controller.go:33),
    injected as the reference tests inject their FuncMap."""
    client_set: object
    enable_cni: bool = False
    manage_all_nodes: bool = False
    manage_nodes_with_annotation_selector: str = ""
    manage_nodes_with_label_selector: str = ""
    disregard_status_with_annotation_selector: str = ""
    disregard_status_with_label_selector: str = ""
    cidr: str = "10.0.0.1/24"
    node_ip: str = "196.168.0.1"
    pod_status_template: str | None = None
    node_initialization_template: str | None = None
    node_heartbeat_template: str | None = None
    start_time: int = 1704067200
    cni: object = None  # EnableCNI: .setup(uid, name, namespace) -> [ip, ...]; .remove(uid, name, namespace)


@dataclass
class WatchObj:
    obj: dict
    uid: str
    rv: str
    deleted: bool


class Echoes:
    """gpu_controller.go echoes: the resourceVersions the engine's own patches
    returned, per object.  An object can take several patches in one tick (a
    node's heartbeat and its init patch; a pod's finalizer patch), each with its
    own echo, so every returned version is kept until its echo is seen (the last
    ECHO_KEEP per object: echoes lost to a watch restart do not pile up)."""

    ECHO_KEEP = 8

    def __init__(self):
        self.rv = {}

    def note(self, uid, rv):
        if uid and rv:
            v = self.rv.setdefault(uid, [])
            v.append(rv)
            if len(v) > self.ECHO_KEEP:
                del v[0]

    def is_echo(self, uid, rv):
        v = self.rv.get(uid)
        if v and rv in v:
            v.remove(rv)
            if not v:
                del self.rv[uid]
            return True
        return False

    def forget(self, uid):
        self.rv.pop(uid, None)


@dataclass
class Stats:
    """what the controller did (tests read it; the Go shim logs it)"""
    echoes_on_arrival: int = 0
    echoes_at_flush: int = 0
    reentered: int = 0    # pods patched without a podIP, ingested again in the same interval
    node_records: int = 0
    pod_records: int = 0
    pod_docs_host: int = 0  # pod documents the GPU codec left to the host codec
    node_docs_host: int = 0  # node documents the GPU codec left to the host codec
    node_docs_canon: int = 0  # node_status_gpu: node documents whose status blobs the device canonicalised
    pod_runs: int = 0
    watch_frames: int = 0       # feed_watch: lines framed
    watch_host_frames: int = 0  # ... of them by the host framer (an escaped type or routed key)
    watch_bad_frames: int = 0   # frames whose status is not OK (malformed lines, unknown types): skipped
    watch_skipped: int = 0      # BOOKMARK / ERROR frames: skipped
    list_items: int = 0         # feed_list: items framed
    list_host_items: int = 0    # ... of them by the host framer (an escaped routed key)
    list_bad_bodies: int = 0    # pages that are no valid list: dropped whole
    resync_swept_nodes: int = 0  # feed_list(replace=True): objects the complete list no longer held, removed
    resync_swept_pods: int = 0
    resync_skipped: int = 0     # ... sessions closed without a sweep (a bad page, frame or record: a partial picture)
    bodies: int = 0
    echo_notes_refused: int = 0  # echo_ledger: notes the device ledger refused (a uid / version outside its domain)
    refs_missing: int = 0       # ref_directory: bodies not sent, their object has no name stored (never with typed / framed feeds)
    responses_framed: int = 0   # response_bytes: response bodies framed on the device (one per successful patch)
    responses_host: int = 0     # ... of them decoded on the host for any reason (an escaped routed key, uid or version)
    response_bytes: int = 0     # ... their bytes, uploaded once
    rejected: list = field(default_factory=list)


def _meta(obj):
    return obj.get("metadata") or {}


class Controller:
    """NewController(conf) + Start: the engine-backed controller."""

    # engine_cgo.go newGPUEngine's geometry (tests pass a smaller one for the CPU oracle,
    # which holds every bucket at its full handle stride)
    GEOMETRY = dict(buckets=4096, node_slots_per_bucket=64, pod_slots_per_bucket=640, pod_handle_stride=65528,
                    max_pod_specs=4096)

    def __init__(self, conf: Config, backend=None, codec_threads=1, suppress_echoes=True, geometry=None,
                 gpu_codec=True, uid_directory=False, echo_ledger=False, ref_directory=False, node_directory=False,
                 response_bytes=False, node_status_gpu=False):
        self.conf = conf
        # uid_directory: the engine's pod uid directory (kwok_watch.h) resolves metadata.uid -> handle on
        # the device; pod_by_uid stays empty (a uid the directory cannot key - empty, escaped in the
        # stream, longer than abi.UID_MAX - is rejected with KWOK_EDOMAIN, where the map would take it)
        self.uid_dir = bool(uid_directory)
        if echo_ledger and not uid_directory:
            raise ValueError("echo_ledger needs uid_directory=True")
        self.suppress = suppress_echoes  # False: every echo re-ingested (tests: the A/B that echoes change nothing)
        custom = {}
        if conf.pod_status_template is not None:
            custom["pod_status_template"] = conf.pod_status_template
        if conf.node_initialization_template is not None:
            custom["node_init_template"] = conf.node_initialization_template
        if conf.node_heartbeat_template is not None:
            custom["node_heartbeat_template"] = conf.node_heartbeat_template
        # engine_cgo.go newGPUEngine: the same geometry and KWOK_CFG_HEARTBEAT_ONCE
        geo = dict(self.GEOMETRY, **(geometry or {}))
        cfg = make_config(cidr=conf.cidr, node_ip=conf.node_ip, start_time=conf.start_time,
                          enable_cni=conf.enable_cni, heartbeat_once=True, **geo, **custom)
        self.eng = (backend or Engine)(cfg)
        if self.uid_dir:
            if not hasattr(self.eng, "uid_dir_enable"):
                raise ValueError("uid_directory needs the engine backend (kwok_uid_dir_enable)")
            self.eng.uid_dir_enable()
        # echo_ledger: the engine's echo ledger (kwok_watch.h) holds the notes of the engine's own patches and
        # drops their echoes on the device: raw frames go to the ingest unfiltered, typed events ask
        # kwok_echo_match, every decision is taken at flush (echoes_on_arrival stays 0) and self.echo stays empty
        self.ledger = bool(echo_ledger)
        self.echo_q = []      # (op, uid, rv) queued for the next kwok_echo_update, in call order
        if self.ledger:
            if not hasattr(self.eng, "echo_enable"):
                raise ValueError("echo_ledger needs the engine backend (kwok_echo_enable)")
            self.eng.echo_enable()
        # ref_directory: the engine's reference directory (kwok_watch.h) holds what a patch is addressed to -
        # a pod's namespace, name and uid, a node's name - and hands it back in the order of the tick's lists:
        # pod_ref, pod_uid and node_name stay empty (node_handle and node_uid, the typed pod events' and the
        # ledger's, stay)
        self.refs = bool(ref_directory)
        if self.refs:
            if not (uid_directory and echo_ledger):
                raise ValueError("ref_directory needs uid_directory=True and echo_ledger=True")
            if not hasattr(self.eng, "refs_enable"):
                raise ValueError("ref_directory needs the engine backend (kwok_refs_enable)")
            self.eng.refs_enable()
        # node_directory: the engine's node uid directory (kwok_watch.h) holds a uid per node slot and resolves
        # names to handles in batches: node_handle and node_uid stay empty too
        self.node_dir = bool(node_directory)
        if self.node_dir:
            if not (uid_directory and echo_ledger and ref_directory):
                raise ValueError("node_directory needs uid_directory=True, echo_ledger=True and ref_directory=True")
            if not hasattr(self.eng, "node_dir_enable"):
                raise ValueError("node_directory needs the engine backend (kwok_node_dir_enable)")
            self.eng.node_dir_enable()
        self.hb_refs = []     # ref_directory: the heartbeat list's references of epoch hb_epoch
        # response_bytes: the responses to the engine's own patches stay bytes (kwok_watch.h): the
        # clientset is asked for raw bodies (patch_*_raw), a tick's bodies are framed on the device
        # (kwok_frame_responses_gpu), the ledger's notes are taken from the frames (kwok_echo_note_framed) and
        # the pods patched without a podIP re-enter from the resident bytes: no response is decoded here
        self.resp = bool(response_bytes)
        if self.resp:
            if not (uid_directory and echo_ledger):
                raise ValueError("response_bytes needs uid_directory=True and echo_ledger=True")
            if not hasattr(self.eng, "frame_responses"):
                raise ValueError("response_bytes needs the engine backend (kwok_frame_responses_gpu)")
        self.rq = self._new_responses()
        self.reentered_dev = 0  # response_bytes: pods that re-entered from the resident response bytes (step 6)
        # node_status_gpu: the device canonicalises the status blobs of the node documents it decodes
        # (kwok_canon.h): a node kwok has patched, seen again through a relist, is decoded with no
        # host codec call (stats.node_docs_host counts only the documents outside the device domain)
        self.node_status_gpu = bool(node_status_gpu)
        if self.node_status_gpu:
            if not hasattr(self.eng, "canon_enable"):
                raise ValueError("node_status_gpu needs the engine backend (kwok_canon_enable)")
            self.eng.canon_enable()
        self.codec = Codec(manage_all_nodes=conf.manage_all_nodes,
                           manage_nodes_with_annotation_selector=conf.manage_nodes_with_annotation_selector,
                           manage_nodes_with_label_selector=conf.manage_nodes_with_label_selector,
                           disregard_status_with_annotation_selector=conf.disregard_status_with_annotation_selector,
                           disregard_status_with_label_selector=conf.disregard_status_with_label_selector)
        self.threads = codec_threads
        # node and pod documents decoded on the GPU (kwok_ingest_nodes_json / kwok_ingest_pods_json)
        # when the backend has them (the CPU oracle backend takes the host codec)
        self.gpu_codec = gpu_codec and hasattr(self.eng, "ingest_pods_json")
        self.nodes: list[WatchObj] = []
        self.pods: list[WatchObj] = []
        self.queued = set()  # uids with an event in the current batch
        self.echo = Echoes()
        self.stats = Stats()
        self.node_name = {}   # node handle -> name
        self.node_handle = {}  # name -> node handle
        self.node_uid = {}    # node handle -> uid (a swept node's echoes are forgotten)
        self.pod_by_uid = {}
        self.pod_uid = {}     # pod handle -> uid
        self.pod_ref = {}     # pod handle -> (namespace, name)
        self.hb = None        # heartbeat handle list of epoch hb_epoch
        self.hb_epoch = None
        self.spec_ids = {}
        self.finalizer = None
        self.reenter = []     # objects of pod patches without a podIP (step 6)
        self.raw = {True: bytearray(), False: bytearray()}  # feed_watch: raw watch bytes per kind (nodes: True)
        self.fed = set()      # the kinds fed raw bytes since the last step
        self.pages = {True: [], False: []}  # feed_list: complete List bodies per kind, in feed order
        self.list_cursor = {}  # "nodes" / "pods" -> kind, resource_version, continue_ of the kind's last page (decoded text)
        # feed_list(replace=True): the kind's open resync session (kwok_watch.h), None: none;
        # dirty: a page, frame or record of it failed - the picture is partial, no sweep
        self.resync = {True: None, False: None}

    def close(self):
        self.eng.close()
        self.codec.close()

    @staticmethod
    def _new_responses():
        """response_bytes: the response bodies of one framing call, appended in apply order: the buffer, the
        bodies' spans, and the indices of the pod patches without a podIP (they re-enter)"""
        return {"buf": bytearray(), "off": [], "len": [], "re": []}

    # ---- Start: the watches (node_controller.go:119-143, pod_controller.go:130-153) ----
    def start(self):
        cs = self.conf.client_set
        cs.watch("nodes", lambda typ, obj: self.on_event(True, typ, obj),
                 label_selector=self.conf.manage_nodes_with_label_selector)
        cs.watch("pods", lambda typ, obj: self.on_event(False, typ, obj), field_selector="spec.nodeName!=")

    def feed_watch(self, nodes: bool, data: bytes):
        """raw bytes of the node (nodes=True) or pod watch response, cut anywhere: they
        are framed and ingested at the next step; an unterminated last line waits
        for its rest"""
        if not hasattr(self.eng, "frame_watch"):
            raise ValueError("feed_watch needs the engine backend (kwok_frame_watch_gpu)")
        if self.nodes if nodes else self.pods:
            raise ValueError("feed_watch after on_event for the same kind within one step")
        self.fed.add(bool(nodes))
        self.raw[bool(nodes)] += data

    def feed_list(self, nodes: bool, body: bytes, replace: bool = False):
        """one complete page of the node (nodes=True) or pod List response
        (pod_controller.go:357-368, node_controller.go:282-296): framed and ingested
        at the next step, before the kind's watch bytes and typed events; its items
        are upserts.  After the step list_cursor[kind] holds the page's
        resourceVersion and continue token: the caller requests the next page with
        the token, or opens its watch from the version.

        replace=True (a relist after 410 Gone, client-go's Replace): the page opens
        the kind's resync session when it is flushed, if none is open; the session
        ends with the flushed page whose continue token is empty, and every node or
        pod the engine holds that no page, watch event or typed event of the session
        touched is then removed as a Deleted event would remove it (kwok_resync_sweep),
        before the same step's typed events and watch bytes of the kind.  A session
        with a bad page, a bad frame or a rejected record is closed without a sweep
        (Stats.resync_skipped): the caller lists again."""
        if not hasattr(self.eng, "frame_list"):
            raise ValueError("feed_list needs the engine backend (kwok_frame_list_gpu)")
        self.pages[bool(nodes)].append((bytes(body), bool(replace)))

    def on_event(self, nodes: bool, typ: str, obj: dict):
        if bool(nodes) in self.fed:
            raise ValueError("on_event after feed_watch for the same kind within one step")
        if typ not in ("ADDED", "MODIFIED", "DELETED"):
            return
        md = _meta(obj)
        w = WatchObj(obj, md.get("uid", ""), md.get("resourceVersion", ""), typ == "DELETED")
        # an echo is dropped only while no other event of its object waits in this
        # tick's batch: after one (a change the engine has not seen, older than the
        # engine's patch) the echo is the object's newest state - it carries both
        if (self.suppress and not self.ledger and typ == "MODIFIED" and self.echo.is_echo(w.uid, w.rv)
                and w.uid not in self.queued):
            self.stats.echoes_on_arrival += 1
            return
        self.queued.add(w.uid)
        (self.nodes if nodes else self.pods).append(w)

    # ---- Has / Size (node_controller.go:403-409) ----------------------------------
    def has(self, name: str) -> bool:
        return bool(name) and self.eng.node_has(name)

    def size(self) -> int:
        return self.eng.node_size()

    # ---- one heartbeat interval (the loop's timer body) ---------------------------
    def step(self, now: int) -> int:
        nw, pw = self.nodes, self.pods
        self.nodes, self.pods, self.queued = [], [], set()
        fed, self.fed = self.fed, set()
        nb = self._encode(nw)
        pb = self._encode(pw)
        pages, self.pages = self.pages, {True: [], False: []}
        for body, replace in pages[True]:  # a kind's list pages go first, in feed order: the watch starts at their version
            self._open_resync(True, replace)
            self._flush_list(True, body)
        self._flush_nodes(nb)
        if True in fed:
            self._flush_watch(True)
        for body, replace in pages[False]:
            self._open_resync(False, replace)
            self._flush_list(False, body)
        self._flush_pods(pb)
        if False in fed:
            self._flush_watch(False)
        if self.conf.enable_cni:
            self._setup_cni()
        n = self._tick(now)
        # step 6: pods patched without a podIP re-enter at once (pod_controller.go:279-319)
        for _ in range(4):  # (a re-entered pod's second patch carries its IPs: one round suffices)
            if not self.reenter and not self.reentered_dev:
                break
            objs, self.reenter = self.reenter, []
            self.stats.reentered += len(objs) + self.reentered_dev  # (response_bytes: ingested in _tick, from the bytes)
            self.reentered_dev = 0
            ws = [WatchObj(o, _meta(o).get("uid", ""), _meta(o).get("resourceVersion", ""), False) for o in objs]
            self._flush_pods((ws, [json.dumps(w.obj, separators=(",", ":")).encode() for w in ws]))
            if self.conf.enable_cni:
                self._setup_cni()
            n += self._tick(now, heartbeats=False)
        return n

    # ---- the notes of the engine's own patches: the host Echoes, or queued for the device ledger ----
    def _note(self, uid, rv):
        if self.ledger:
            if uid and rv:
                self.echo_q.append((abi.ECHO_NOTE, uid, rv))
        else:
            self.echo.note(uid, rv)

    def _forget(self, uid):
        if self.ledger:
            if uid:
                self.echo_q.append((abi.ECHO_FORGET, uid, ""))
        else:
            self.echo.forget(uid)

    def _send_echo(self):
        """the queued notes and forgets in one kwok_echo_update (applied in queue order per uid)"""
        q, self.echo_q = self.echo_q, []
        if q:
            st = self.eng.echo_update([x[0] for x in q], [x[1] for x in q], [x[2] for x in q])
            self.stats.echo_notes_refused += int((st != abi.OK).sum())  # (a uid / version outside the ledger's domain)

    def _encode(self, ws):
        if self.ledger and self.suppress and ws:  # the same rule, decided by the device ledger
            drop = self.eng.echo_match([w.uid for w in ws], [w.rv for w in ws], [w.deleted for w in ws])
            self.stats.echoes_at_flush += int(drop.sum())
            keep = [w for w, d in zip(ws, drop) if not d]
            return keep, [json.dumps(w.obj, separators=(",", ":")).encode() for w in keep]
        keep, seen = [], set()
        for w in ws:
            # (the same rule as on arrival: only before any kept event of the object)
            if self.suppress and not w.deleted and self.echo.is_echo(w.uid, w.rv) and w.uid not in seen:
                self.stats.echoes_at_flush += 1
                continue
            seen.add(w.uid)
            keep.append(w)
            if w.deleted:  # the object's last event: echoes still noted for it will not come
                self.echo.forget(w.uid)
        return keep, [json.dumps(w.obj, separators=(",", ":")).encode() for w in keep]

    def _flush_nodes(self, batch):
        """gpu_controller.go flushNodes: on the HIP engine the documents are decoded on
        the GPU (kwok_ingest_nodes_json); a backend without it takes the host codec"""
        ws, docs = batch
        if not ws:
            return
        if self.gpu_codec:
            return self._flush_nodes_gpu(ws, docs)
        b = self.codec.decode_nodes(docs, strict=False, threads=self.threads)
        keep, names = [], []
        for i, w in enumerate(ws):
            if b.status[i] != abi.OK:  # outside the engine's domain: not simulated
                self.stats.rejected.append(("node", _meta(w.obj).get("name"), b.status[i]))
                continue
            r = np.frombuffer(bytes(b.nodes[i]), abi.NODE_EVENT_DTYPE).copy()
            r["op"] = abi.OP_DELETE if w.deleted else abi.OP_UPSERT
            keep.append(r)
            names.append(b.text(b.nodes[i].name))
        if not keep:
            return
        recs = np.concatenate(keep)
        hs, st = self.eng.ingest_nodes_raw(recs, bytes(b.buf))
        self.stats.node_records += len(recs)
        for k in range(len(recs)):
            if st[k] != abi.OK:
                continue
            if recs[k]["op"] == abi.OP_DELETE:
                self._node_pop(int(hs[k]), names[k])
            else:
                self._node_put(int(hs[k]), names[k])

    def _count_node_docs(self, nh):
        """a device node decode: the documents its host codec decoded and, with node_status_gpu, the
        documents canonicalised on the device so far (kwok_canon_stats' docs)"""
        self.stats.node_docs_host += nh
        if self.node_status_gpu:
            self.stats.node_docs_canon = self.eng.canon_stats()["docs"]

    def _flush_nodes_gpu(self, ws, docs):
        """gpu_controller.go flushNodes on the device codec: the documents straight to
        kwok_ingest_nodes_json (a Deleted event's status is not read); names from the
        watch objects"""
        arena, offs, lens = Engine._docs(docs)
        ops = np.array([abi.OP_DELETE if w.deleted else abi.OP_UPSERT for w in ws], np.uint8)
        hs, st, nh = self.eng.ingest_nodes_json(self.codec, arena, offs, lens, ops)
        self._count_node_docs(nh)
        self.stats.node_records += int(np.isin(st, (abi.EDOMAIN, abi.EINVAL), invert=True).sum())
        bound = {}  # node_directory: handle -> the uid of its last upsert (a typed event carries none to the device)
        for k, w in enumerate(ws):
            name = _meta(w.obj).get("name", "")
            if st[k] != abi.OK:
                if st[k] in (abi.EDOMAIN, abi.EINVAL):  # outside the engine's domain: not simulated
                    self.stats.rejected.append(("node", name, int(st[k])))
                continue
            if w.deleted:
                self._node_pop(int(hs[k]), name)
                bound.pop(int(hs[k]), None)
            else:
                self._node_put(int(hs[k]), name, w.uid)
                bound[int(hs[k])] = w.uid
        self._node_bind(bound)

    def _node_bind(self, bound):
        """node_directory: the nodes a typed batch created or updated are bound to their uids on the device
        (where the pod paths call kwok_uid_bind), so that a sweep finds the uid whose notes it forgets"""
        if not self.node_dir:
            return
        ok = [(h, u) for h, u in bound.items() if u and 0 < len(u.encode()) <= abi.UID_MAX]
        if ok:
            self.eng.node_bind([h for h, _u in ok], [u for _h, u in ok])

    def _node_handles(self, names):
        """node_directory: name -> handle of the existing nodes among names, by one kwok_node_lookup"""
        names = list(dict.fromkeys(names))
        hs = self.eng.node_lookup(names) if names else []
        return {n: int(h) for n, h in zip(names, hs) if h >= 0}

    def _node_put(self, h, name, uid=None):
        """a node the engine created or updated: its handle by name (and, ref_directory off, its name by handle);
        node_directory: the device holds all three"""
        if self.node_dir:
            return
        if not self.refs:
            self.node_name[h] = name
        self.node_handle[name] = h
        if uid is not None:
            self.node_uid[h] = uid

    def _node_pop(self, h, name):
        if self.node_dir:
            return
        self.node_name.pop(h, None)
        self.node_handle.pop(name, None)
        self.node_uid.pop(h, None)

    def _pod_put(self, h, uid, ref):
        if not self.refs:  # (ref_directory: the device holds them)
            self.pod_uid[h] = uid
            self.pod_ref[h] = ref

    def _spec_id(self, b, d):
        spec = (tuple((b.text(c.name), b.text(c.image)) for c in d.containers[:d.n_containers]),
                tuple((b.text(c.name), b.text(c.image)) for c in d.init_containers[:d.n_init_containers]),
                tuple(b.text(g) for g in d.readiness_gates[:d.n_readiness_gates]))
        sid = self.spec_ids.get(spec)
        if sid is None:
            sid = self.spec_ids[spec] = self.eng.register_pod_spec(*spec)
        return sid

    def _uid_map(self, uids):
        """the typed paths' uid -> handle map: the controller's own, or (uid_directory) the batch's
        uids resolved by the device (kwok_uid_lookup) - the pods the directory holds"""
        if not self.uid_dir:
            return self.pod_by_uid
        us = list(dict.fromkeys(uids))
        hs = self.eng.uid_lookup(us) if us else []
        return {u: int(h) for u, h in zip(us, hs) if h >= 0}

    def _uid_bind(self, by_uid, uids, names=None):
        """uid_directory: the pods a typed batch created (or touched) are bound on the device, so that
        raw bytes and typed events of one pod can be mixed"""
        if not self.uid_dir:
            return
        us = [u for u in dict.fromkeys(uids) if u in by_uid and 0 < len(u.encode()) <= abi.UID_MAX]
        if us:
            self.eng.uid_bind([by_uid[u] for u in us], us)
        if self.refs and names is not None:  # ... and named (a typed event carries neither to the device)
            last = {u: r for u, r in zip(uids, names) if u in by_uid}
            ok = [(by_uid[u], ns.encode(), nm.encode()) for u, (ns, nm) in last.items()]
            ok = [x for x in ok if 0 < len(x[2]) <= abi.REF_NAME_MAX and len(x[1]) <= abi.REF_NS_MAX]
            if ok:
                self.eng.refs_bind([x[0] for x in ok], [x[1] for x in ok], [x[2] for x in ok])

    def _flush_pods(self, batch):
        """gpu_controller.go flushPods: decode, then ingest in runs (ingest_pod_runs).
        On the HIP engine the documents are decoded on the GPU (ingest_doc_runs);
        a backend without kwok_ingest_pods_json (the CPU oracle) takes the host codec."""
        ws, docs = batch
        if not ws:
            return
        if self.gpu_codec:
            return self._flush_pods_gpu(ws, docs)
        b = self.codec.decode_pods(docs, strict=False, threads=self.threads)
        idx, recs = [], []
        # the node by handle when the engine holds it; otherwise by spec.nodeName (node_directory: the batch's
        # names resolved by one kwok_node_lookup)
        on = self.node_handle if not self.node_dir else self._node_handles(
            b.text(b.pods[i].ev.node_name) for i, w in enumerate(ws) if b.status[i] == abi.OK and not w.deleted)
        for i, w in enumerate(ws):
            if b.status[i] != abi.OK:
                self.stats.rejected.append(("pod", _meta(w.obj).get("name"), b.status[i]))
                continue
            d = b.pods[i]
            r = np.frombuffer(bytes(d.ev), abi.POD_EVENT_DTYPE).copy()
            if w.deleted:
                # EnableCNI: cni.Remove for a pod on a managed node (pod_controller.go:337-342),
                # also when the engine deleted it already (its handle is gone)
                if self.conf.enable_cni and self.conf.cni and self.has(b.text(d.ev.node_name)):
                    self.conf.cni.remove(w.uid, b.text(d.name), b.text(d.namespace_))
            else:
                try:
                    r["spec_id"] = self._spec_id(b, d)
                except Exception as ex:  # KWOK_EDOMAIN: outside the supported domain
                    self.stats.rejected.append(("pod-spec", b.text(d.name), str(ex)))
                    continue
                r["node_handle"] = on.get(b.text(d.ev.node_name), -1)
            idx.append(i)
            recs.append(r)
        if not recs:
            return
        recs = np.concatenate(recs)
        uids = [ws[i].uid for i in idx]
        deleted = [ws[i].deleted for i in idx]
        refs = [(b.text(b.pods[i].namespace_), b.text(b.pods[i].name)) for i in idx]
        by_uid = self._uid_map(uids)
        hs, st, runs = ingest_pod_runs(self.eng, by_uid, recs, uids, deleted, bytes(b.buf))
        self._uid_bind(by_uid, uids, refs)
        self.stats.pod_records += int((st != NOT_SENT).sum())
        self.stats.pod_runs += runs
        for k in range(len(recs)):
            if st[k] != abi.OK:
                continue
            h = int(hs[k])
            if deleted[k]:
                self.pod_uid.pop(h, None)
                self.pod_ref.pop(h, None)
            else:
                self._pod_put(h, uids[k], refs[k])

    def _flush_pods_gpu(self, ws, docs):
        """gpu_controller.go flushPodsJSON: the documents straight to
        kwok_ingest_pods_json in runs; names and nodes from the watch objects"""
        uids = [w.uid for w in ws]
        deleted = [w.deleted for w in ws]
        by_uid = self._uid_map(uids)
        hs, st, runs, n_host = ingest_doc_runs(self.eng, self.codec, by_uid, docs, uids, deleted)
        self._uid_bind(by_uid, uids, [(_meta(w.obj).get("namespace", ""), _meta(w.obj).get("name", "")) for w in ws]
                       if self.refs else None)
        self.stats.pod_records += int((st != NOT_SENT).sum())
        self.stats.pod_runs += runs
        self.stats.pod_docs_host += n_host
        for k, w in enumerate(ws):
            md = _meta(w.obj)
            if st[k] not in (abi.OK, NOT_SENT):
                self.stats.rejected.append(("pod", md.get("name"), int(st[k])))
                continue
            if w.deleted:
                # EnableCNI: cni.Remove for a pod on a managed node (pod_controller.go:337-342),
                # also when the engine deleted it already (its handle is gone)
                if self.conf.enable_cni and self.conf.cni and self.has((w.obj.get("spec") or {}).get("nodeName", "")):
                    self.conf.cni.remove(w.uid, md.get("name", ""), md.get("namespace", ""))
                if st[k] == abi.OK:
                    self.pod_uid.pop(int(hs[k]), None)
                    self.pod_ref.pop(int(hs[k]), None)
            else:
                self._pod_put(int(hs[k]), w.uid, (md.get("namespace", ""), md.get("name", "")))

    def _flush_watch(self, nodes):
        """the raw bytes of one kind's watch: framed on the GPU, then _ingest_frames:
        echoes dropped by the frames' (uid, resourceVersion) under _encode's rule, the
        kept frames ingested from the resident stream; names for the patches from the
        frames' spans.  The unconsumed tail stays buffered."""
        stream = bytes(self.raw[nodes])
        frames, used, n_host, sid = self.eng.frame_watch(stream)
        self.raw[nodes] = bytearray(stream[used:])
        self.stats.watch_frames += len(frames)
        self.stats.watch_host_frames += n_host
        self._ingest_frames(nodes, stream, frames, sid)

    def _open_resync(self, nodes, replace):
        """a page fed with replace=True opens the kind's resync session, if none is open"""
        if replace and self.resync[nodes] is None:
            self.eng.resync_begin(abi.KIND_NODES if nodes else abi.KIND_PODS)
            self.resync[nodes] = {"dirty": False}

    def _flush_list(self, nodes, body):
        """one List page: framed on the GPU, its items taken as upserts by the path
        of the watch frames (an item whose (uid, resourceVersion) is an echo of the
        engine's own patch is dropped; inside a resync session its known handle is
        marked instead); the page's resourceVersion and continue token go to
        list_cursor.  A body that is no valid list is counted and dropped (client-go:
        the List call fails, the caller lists again).  The page that completes a
        list (an empty continue token) ends the kind's open resync session."""
        sess = self.resync[nodes]
        try:
            frames, info, n_host, sid = self.eng.frame_list(body)
        except KwokError as err:
            if err.code != abi.EINVAL:
                raise
            self.stats.list_bad_bodies += 1
            if sess is not None:
                sess["dirty"] = True
            return
        self.stats.list_items += len(frames)
        self.stats.list_host_items += n_host
        self.list_cursor["nodes" if nodes else "pods"] = dict(
            kind=list_text(body, info.kind, info.flags & abi.LIST_ESC_KIND),
            resource_version=list_text(body, info.resource_version, info.flags & abi.LIST_ESC_RV),
            continue_=list_text(body, info.continue_, info.flags & abi.LIST_ESC_CONTINUE))
        self._ingest_frames(nodes, body, frames, sid, sess)
        if sess is not None and not self.list_cursor["nodes" if nodes else "pods"]["continue_"]:
            self._end_resync(nodes)  # the list is complete

    def _end_resync(self, nodes):
        """the kind's resync session ends: the sweep (kwok_resync_sweep) of what the complete
        list did not hold, and the bookkeeping of the swept objects - or, after a bad page,
        frame or rejected record, no sweep at all (a sweep deletes: never on a partial picture)"""
        kind = abi.KIND_NODES if nodes else abi.KIND_PODS
        sess, self.resync[nodes] = self.resync[nodes], None
        if sess["dirty"]:
            self.eng.resync_end(kind)
            self.stats.resync_skipped += 1
            return
        hs, _rel, nd = self.eng.resync_sweep(kind)
        if nodes and self.node_dir:
            # the swept nodes' slots keep their uids (stale) until the next node ingest: no map is inverted
            for _st, _ns, _name, uid in (self.eng.ref_items(*self.eng.refs_lookup(abi.KIND_NODES, hs, abi.REFS_ANY_SLOT))
                                         if len(hs) else []):
                self._forget(uid.decode())
            self.stats.resync_swept_nodes += len(hs)
            self._send_echo()
            return
        if nodes:
            # (ref_directory: a swept node's entry may be gone with its name; node_handle still names it)
            by_handle = {v: k for k, v in self.node_handle.items()} if self.refs and len(hs) else self.node_name
            for h in hs.tolist():
                self.node_handle.pop(by_handle.pop(h, None), None)
                self._forget(self.node_uid.pop(h, None))
            self.stats.resync_swept_nodes += len(hs)
            self._send_echo()
            return
        if self.refs:  # the swept pods' slots keep their bytes until the next pod ingest
            cni = self.conf.enable_cni and self.conf.cni
            pods = self.eng.ref_items(*self.eng.refs_lookup(abi.KIND_PODS, hs, abi.REFS_ANY_SLOT)) if len(hs) else []
            on = self.eng.ref_items(*self.eng.refs_lookup(abi.KIND_NODES, nd)) if cni and len(hs) else []
            for k, (status, ns, name, uid) in enumerate(pods):
                if cni and status == abi.OK and self.has(on[k][2].decode()):
                    self.conf.cni.remove(uid.decode(), name.decode(), ns.decode())
                self._forget(uid.decode())
            self.stats.resync_swept_pods += len(hs)
            self._send_echo()
            return
        for h, n in zip(hs.tolist(), nd.tolist()):
            uid = self.pod_uid.get(h)
            # EnableCNI: cni.Remove for a swept pod on a managed node (pod_controller.go:337-342), before its
            # handle's bookkeeping goes (_flush_pods_gpu's order); its node from the sweep: there is no document
            if self.conf.enable_cni and self.conf.cni and h in self.pod_ref and self.has(self.node_name.get(n, "")):
                ns, name = self.pod_ref[h]
                self.conf.cni.remove(uid, name, ns)
            self.pod_uid.pop(h, None)
            self.pod_ref.pop(h, None)
            self.pod_by_uid.pop(uid, None)
            self._forget(uid)
        self.stats.resync_swept_pods += len(hs)
        self._send_echo()

    def _ingest_frames(self, nodes, stream, frames, sid, sess=None):
        """step 1-3 over the frames of the resident stream (a watch stream's lines or
        a List body's items).  sess: the page's open resync session (_flush_list)"""
        def text(f, key, bit):
            raw = stream[int(f[key]["off"]):int(f[key]["off"]) + int(f[key]["len"])]
            return json.loads(b'"' + raw + b'"') if f["flags"] & bit else raw.decode()

        name = lambda i: text(frames[i], "name", abi.FRAME_ESC_NAME)  # noqa: E731
        ns = lambda i: text(frames[i], "namespace_", abi.FRAME_ESC_NS)  # noqa: E731
        if self.ledger and self.suppress:
            return self._ingest_frames_ledger(nodes, stream, frames, sid, sess, text, name, ns)
        keep, uids, deleted, seen, echoed = [], [], [], set(), []
        for i, f in enumerate(frames):
            if f["status"] != abi.OK:
                self.stats.watch_bad_frames += 1
                if sess is not None:
                    sess["dirty"] = True
                continue
            if f["type"] in (abi.WATCH_BOOKMARK, abi.WATCH_ERROR):
                self.stats.watch_skipped += 1
                continue
            if f["type"] == abi.WATCH_NONE:
                continue
            uid, rv = text(f, "uid", abi.FRAME_ESC_UID), text(f, "resource_version", abi.FRAME_ESC_RV)
            dl = f["type"] == abi.WATCH_DELETED
            if self.suppress and not dl and self.echo.is_echo(uid, rv) and uid not in seen:
                self.stats.echoes_at_flush += 1
                if sess is not None:  # seen in the list, not ingested: marked by its known handle
                    echoed.append(self.node_handle.get(name(i), -1) if nodes else
                                  uid if self.uid_dir else self.pod_by_uid.get(uid, -1))
                continue
            seen.add(uid)
            if dl:
                self.echo.forget(uid)
            keep.append(i)
            uids.append(uid)
            deleted.append(dl)
        if echoed and not nodes and self.uid_dir:  # (the echoes' handles from the device)
            echoed = self.eng.uid_lookup(echoed).tolist()
        echoed = [h for h in echoed if h >= 0]
        if echoed:
            self.eng.resync_mark(abi.KIND_NODES if nodes else abi.KIND_PODS, echoed)
        if not keep:
            return
        keep = np.array(keep, np.uint32)
        partial = (abi.EDOMAIN, abi.EINVAL, abi.EFULL)  # a rejected record: the session's picture is partial
        if nodes:
            hs, st, nh = self.eng.ingest_nodes_framed(self.codec, sid, keep)
            self._count_node_docs(nh)
            self.stats.node_records += int(np.isin(st, (abi.EDOMAIN, abi.EINVAL), invert=True).sum())
            for k, i in enumerate(keep):
                if st[k] != abi.OK:
                    if st[k] in (abi.EDOMAIN, abi.EINVAL):
                        self.stats.rejected.append(("node", name(i), int(st[k])))
                    if sess is not None and st[k] in partial:
                        sess["dirty"] = True
                    continue
                if deleted[k]:
                    self._node_pop(int(hs[k]), name(i))
                else:
                    self._node_put(int(hs[k]), name(i), uids[k])
            return
        n_host = [0]

        def send(idx, ops, hv):
            h1, s1, _rel, nh = self.eng.ingest_pods_framed(self.codec, sid, keep[idx], hv.astype(np.int32))
            n_host[0] += nh
            return h1, s1

        if self.uid_dir:  # one call: uids resolved, runs cut and creates bound on the device
            hs, st, _rel, nh, runs = self.eng.ingest_pods_framed_uid(self.codec, sid, keep)
            n_host[0] = nh
        else:
            hs, st, runs = ingest_pod_runs(self.eng, self.pod_by_uid, np.empty(len(keep)), uids, deleted, None, sender=send)
        self.stats.pod_records += int((st != NOT_SENT).sum())
        self.stats.pod_runs += runs
        self.stats.pod_docs_host += n_host[0]
        for k, i in enumerate(keep):
            if st[k] not in (abi.OK, NOT_SENT):
                self.stats.rejected.append(("pod", name(i), int(st[k])))
                if sess is not None and st[k] in partial:
                    sess["dirty"] = True
                continue
            if deleted[k]:
                # EnableCNI: cni.Remove for a pod on a managed node, before its handle's bookkeeping
                # (_flush_pods_gpu's order); spec.nodeName is not in the frame: the document is read
                if self.conf.enable_cni and self.conf.cni:
                    f = frames[i]
                    obj = json.loads(stream[int(f["doc_off"]):int(f["doc_off"]) + int(f["doc_len"])])
                    if self.has((obj.get("spec") or {}).get("nodeName", "")):
                        self.conf.cni.remove(uids[k], name(i), ns(i))
                if st[k] == abi.OK:
                    self.pod_uid.pop(int(hs[k]), None)
                    self.pod_ref.pop(int(hs[k]), None)
            else:
                self._pod_put(int(hs[k]), uids[k], (ns(i), name(i)))

    def _ingest_frames_ledger(self, nodes, stream, frames, sid, sess, text, name, ns):
        """_ingest_frames with the echo ledger: ALL frames of the batch in one call per kind, the echoes
        dropped on the device; the counters come from the frame array and the statuses, names are decoded
        only for the records the controller book-keeps (creates, deletes, rejected records)"""
        n = len(frames)
        if not n:
            return
        kind = abi.KIND_NODES if nodes else abi.KIND_PODS
        partial = (abi.EDOMAIN, abi.EINVAL, abi.EFULL)
        ty, fl = frames["type"], frames["flags"]
        bad = frames["status"] != abi.OK
        self.stats.watch_bad_frames += int(bad.sum())
        if sess is not None and bad.any():
            sess["dirty"] = True
        self.stats.watch_skipped += int((~bad & np.isin(ty, (abi.WATCH_BOOKMARK, abi.WATCH_ERROR))).sum())
        ing = ~bad & np.isin(ty, (abi.WATCH_ADDED, abi.WATCH_MODIFIED, abi.WATCH_DELETED))
        if not ing.any():
            return
        uid_of = lambda i: text(frames[i], "uid", abi.FRAME_ESC_UID)  # noqa: E731
        runs = 0
        if nodes:
            hs, st, nh, ne = self.eng.ingest_nodes_framed_echo(self.codec, sid, np.arange(n, dtype=np.uint32))
        else:
            hs, st, _rel, nh, runs, ne = self.eng.ingest_pods_framed_echo(self.codec, sid, np.arange(n, dtype=np.uint32))
        self.stats.echoes_at_flush += ne
        # a frame whose uid / resourceVersion holds an escape is not decided on the device (no apiserver sends one):
        # the typed filter on its decoded text, then the plain framed entry - behind the batch's other records
        esc = np.nonzero(ing & ((fl & (abi.FRAME_ESC_UID | abi.FRAME_ESC_RV)) != 0))[0]
        if len(esc):
            drop = self.eng.echo_match([uid_of(i) for i in esc],
                                       [text(frames[i], "resource_version", abi.FRAME_ESC_RV) for i in esc],
                                       ty[esc] == abi.WATCH_DELETED)
            self.stats.echoes_at_flush += int(drop.sum())
            st[esc[drop != 0]] = abi.ECHO
            if nodes and self.node_dir:  # (an echo's handle: the decoded name, resolved by the device)
                dropped = esc[drop != 0]
                if len(dropped):
                    hs[dropped] = self.eng.node_lookup([name(i) for i in dropped])
            elif nodes:  # (an echo's handle: the name the controller knows)
                for i in esc[drop != 0]:
                    hs[i] = self.node_handle.get(name(i), -1)
            late = esc[drop == 0].astype(np.uint32)
            if len(late):
                if nodes:
                    hs[late], st[late], nh2 = self.eng.ingest_nodes_framed(self.codec, sid, late)
                    if self.node_dir:
                        self._bind_escaped_uids(late, hs, st, ty, uid_of)
                else:
                    hs[late], st[late], _rel, nh2, r2 = self.eng.ingest_pods_framed_uid(self.codec, sid, late)
                    runs += r2
                nh += nh2
        if sess is not None:  # seen in the list, not ingested: marked by the handle the device resolved
            marks = hs[ing & (st == abi.ECHO) & (hs >= 0)]
            if len(marks):
                self.eng.resync_mark(kind, marks)
        keep = np.nonzero(ing & (st != abi.ECHO))[0]
        if nodes:
            self._count_node_docs(nh)
            self.stats.node_records += int(np.isin(st[keep], (abi.EDOMAIN, abi.EINVAL), invert=True).sum())
            if self.node_dir:  # the device keeps name, handle and uid of every record: only the rejected ones are looked at
                keep = keep[st[keep] != abi.OK]
            for i in keep.tolist():
                h = int(hs[i])
                if st[i] != abi.OK:
                    if st[i] in (abi.EDOMAIN, abi.EINVAL):
                        self.stats.rejected.append(("node", name(i), int(st[i])))
                    if sess is not None and st[i] in partial:
                        sess["dirty"] = True
                elif ty[i] == abi.WATCH_DELETED:
                    self._node_pop(h, name(i))
                elif h not in (self.node_uid if self.refs else self.node_name):  # a create (a known node keeps its name and uid)
                    self._node_put(h, name(i), uid_of(i))
            return
        self.stats.pod_records += int((st[keep] != NOT_SENT).sum())
        self.stats.pod_runs += runs
        self.stats.pod_docs_host += nh
        if self.refs:
            # the device stored every create's namespace and name from its frame: only rejected records, CNI
            # deletes and creates whose frame holds an escaped name (their decoded text is bound) are looked at
            sent = np.isin(st[keep], (abi.OK, NOT_SENT))
            dels = keep[sent & (ty[keep] == abi.WATCH_DELETED)] if self.conf.enable_cni and self.conf.cni else keep[:0]
            escn = keep[(st[keep] == abi.OK) & (ty[keep] != abi.WATCH_DELETED) &
                        ((fl[keep] & (abi.FRAME_ESC_NAME | abi.FRAME_ESC_NS)) != 0)]
            for i in sorted(keep[~sent].tolist() + dels.tolist()):
                if st[i] not in (abi.OK, NOT_SENT):
                    self.stats.rejected.append(("pod", name(i), int(st[i])))
                    if sess is not None and st[i] in partial:
                        sess["dirty"] = True
                else:
                    f = frames[i]
                    obj = json.loads(stream[int(f["doc_off"]):int(f["doc_off"]) + int(f["doc_len"])])
                    if self.has((obj.get("spec") or {}).get("nodeName", "")):
                        self.conf.cni.remove(uid_of(i), name(i), ns(i))
            if len(escn):
                self.eng.refs_bind(hs[escn], [ns(i).encode() for i in escn], [name(i).encode() for i in escn])
            return
        for i in keep.tolist():
            h = int(hs[i])
            if st[i] not in (abi.OK, NOT_SENT):
                self.stats.rejected.append(("pod", name(i), int(st[i])))
                if sess is not None and st[i] in partial:
                    sess["dirty"] = True
            elif ty[i] == abi.WATCH_DELETED:
                if self.conf.enable_cni and self.conf.cni:  # (_ingest_frames: the document is read for spec.nodeName)
                    f = frames[i]
                    obj = json.loads(stream[int(f["doc_off"]):int(f["doc_off"]) + int(f["doc_len"])])
                    if self.has((obj.get("spec") or {}).get("nodeName", "")):
                        self.conf.cni.remove(uid_of(i), name(i), ns(i))
                if st[i] == abi.OK:
                    self.pod_uid.pop(h, None)
                    self.pod_ref.pop(h, None)
            elif h not in self.pod_ref:  # a create (a known pod keeps its uid and name)
                self.pod_uid[h] = uid_of(i)
                self.pod_ref[h] = (ns(i), name(i))

    def _bind_escaped_uids(self, late, hs, st, ty, uid_of):
        """node_directory: a kept node frame whose uid holds an escape stored no uid on the device (the span is
        the raw text); a node that has none afterwards - a create, as `h not in node_uid` decides it on the host -
        is bound to the decoded text"""
        first = {}  # handle -> its first such frame (the rule keeps a known node's uid)
        for i in late.tolist():
            if st[i] == abi.OK and ty[i] != abi.WATCH_DELETED:
                first.setdefault(int(hs[i]), i)
        if not first:
            return
        refs, _blob = self.eng.refs_lookup(abi.KIND_NODES, list(first))
        self._node_bind({h: uid_of(i) for (h, i), ul in zip(first.items(), refs["uid_len"].tolist()) if ul == 0})

    def _setup_cni(self):
        hs = self.eng.cni_pending()
        if not len(hs):
            return
        keep, ips = [], []
        named = self.eng.ref_items(*self.eng.refs_lookup(abi.KIND_PODS, hs)) if self.refs else None
        for k, h in enumerate(hs):
            if named is not None:
                status, ns, name, uid = named[k]
                if status != abi.OK:
                    self.stats.refs_missing += 1
                    continue
                uid, ns, name = uid.decode(), ns.decode(), name.decode()
            else:
                uid, (ns, name) = self.pod_uid[int(h)], self.pod_ref[int(h)]
            try:
                got = self.conf.cni.setup(uid, name, ns)
            except Exception:  # a failed Setup leaves the pod unpatched this tick
                continue
            ip = abi.ip4(got[0]) if got else 0
            if ip:
                keep.append(int(h))
                ips.append(ip)
        if keep:
            self.eng.cni_assign(keep, ips)

    # ---- tick + apply (engine_cgo.go tick / applyPatches, gpu_controller.go step) -----
    def _tick(self, now, heartbeats=True):
        e = self.eng
        res = e.tick_raw(now)
        new_epoch = self.hb is None or res.heartbeat_epoch != self.hb_epoch
        if new_epoch:
            self.hb = np.empty(res.n_heartbeat, np.int32)
        L = {"ini": np.empty(res.n_node_init, np.int32), "ini_off": np.empty(res.n_node_init, np.uint64),
             "ini_len": np.empty(res.n_node_init, np.uint32),
             "pp": np.empty(res.n_pod_patch, np.int32), "pp_off": np.empty(res.n_pod_patch, np.uint64),
             "pp_len": np.empty(res.n_pod_patch, np.uint32),
             "dl": np.empty(res.n_delete, np.int32), "dlf": np.empty(res.n_delete, np.uint8)}
        p = lambda k: L[k].ctypes.data if L[k].size else None  # noqa: E731
        out = abi.Outputs(self.hb.ctypes.data if (new_epoch and self.hb.size) else None, 0,
                          p("ini"), p("ini_off"), p("ini_len"), p("pp"), p("pp_off"), p("pp_len"),
                          p("dl"), p("dlf"), None, 0, 0)
        e._check(e._fn("read_outputs")(e._h, C.byref(out)), "read_outputs")
        self.hb_epoch = res.heartbeat_epoch
        if self.refs and new_epoch:  # the heartbeat list's references change with the handle list
            self.hb_refs = self._read_refs(abi.REFS_HEARTBEAT, 0, res.n_heartbeat)
        n = 0
        if res.n_heartbeat and heartbeats:
            body = e.read_arena(out.heartbeat_off, res.heartbeat_len).tobytes()
            for k, h in enumerate(self.hb):
                self._apply(HEARTBEAT, int(h), body, self.hb_refs[k] if self.refs else None)
                n += 1
        n += self._apply_patches(NODE_INIT, L["ini"], L["ini_off"], L["ini_len"], abi.REFS_NODE_INIT)
        n += self._apply_patches(POD_PATCH, L["pp"], L["pp_off"], L["pp_len"], abi.REFS_POD_PATCH)
        gone = []
        dl_refs = self._read_refs(abi.REFS_DELETE, 0, res.n_delete) if self.refs else None  # (the tick freed them: their bytes stay)
        if self.resp:  # call 1: the heartbeat, node-init and pod-patch responses, in apply order (every list is read)
            self._flush_responses()
        for k, (h, f) in enumerate(zip(L["dl"], L["dlf"])):  # Patch(removeFinalizers) if finalizers, then Delete(grace 0)
            # the engine freed the handle: the pod's noted echoes go BEFORE the apply, so
            # that the echo of its finalizer patch (noted by the apply) is dropped
            # (gpu_controller.go forgets in the tick callback, ahead of the task)
            ref = dl_refs[k] if self.refs else None
            self._forget(ref[3].decode() if ref else self.pod_uid.get(int(h)))
            self._apply(DELETE_FIN if f else DELETE, int(h), None, ref)
            gone.append(int(h))
            n += 1
        for h in gone:  # the later Deleted watch event finds no handle
            uid = self.pod_uid.pop(h, None)
            self.pod_by_uid.pop(uid, None)
            self.pod_ref.pop(h, None)
        self.stats.bodies += n
        self._send_echo()  # (response_bytes: call 2, the delete list's forgets - behind call 1's notes)
        if self.resp:      # call 3: the finalizer-patch responses.  A uid is in one delete list once: the per-uid
            self._flush_responses()  # order of the three calls is the interleaved order of the queue
            self._send_echo()  # (the notes of responses whose uid / version holds an escape: decoded here)
        return n

    def _response(self, raw, reenter=False):
        """response_bytes: one response body joins the tick's buffer"""
        q = self.rq
        q["off"].append(len(q["buf"]))
        q["len"].append(len(raw))
        q["buf"] += raw
        if reenter:
            q["re"].append(len(q["off"]) - 1)

    def _flush_responses(self):
        """response_bytes: the collected bodies framed on the device, one note per response from its frame, and
        the pod patches without a podIP ingested from the resident bytes by uid (not the echo entry: like the
        host path's re-entry it is not dropped as its own echo; the note stays for the watch echo).  Fallbacks as
        _ingest_frames_ledger's: a response whose uid / resourceVersion holds an escape is decoded here and its
        text noted through kwok_echo_update; a re-entering one with an escaped uid takes the document path."""
        q, self.rq = self.rq, self._new_responses()
        n = len(q["off"])
        if not n:
            return
        buf = bytes(q["buf"])
        frames, n_host, sid = self.eng.frame_responses(buf, q["off"], q["len"])
        self.stats.responses_framed += n
        self.stats.response_bytes += len(buf)
        body = lambda i: buf[q["off"][i]:q["off"][i] + q["len"][i]]  # noqa: E731
        st = self.eng.echo_note_framed(sid, np.arange(n, dtype=np.uint32))
        fl = frames["flags"]
        host = set()
        esc = np.nonzero((st == abi.EDOMAIN) & ((fl & (abi.FRAME_ESC_UID | abi.FRAME_ESC_RV)) != 0))[0].tolist()
        for i in esc:
            md = _meta(json.loads(body(i)))
            self._note(md.get("uid"), md.get("resourceVersion"))
            host.add(i)
        self.stats.echo_notes_refused += int((st != abi.OK).sum()) - len(esc)
        if q["re"]:
            idx = np.array(q["re"], np.uint32)
            _hs, s2, _rel, nh, runs = self.eng.ingest_pods_framed_uid(self.codec, sid, idx)
            self.stats.pod_records += len(idx)
            self.stats.pod_runs += runs
            self.stats.pod_docs_host += nh
            for k, i in enumerate(idx.tolist()):
                if s2[k] == abi.EDOMAIN and fl[i] & abi.FRAME_ESC_UID:
                    self.reenter.append(json.loads(body(i)))  # (step 6 sends it through the document path)
                    host.add(i)
                    continue
                self.reentered_dev += 1
                if s2[k] not in (abi.OK, NOT_SENT):
                    f = frames[i]
                    self.stats.rejected.append(("pod", buf[int(f["name"]["off"]):int(f["name"]["off"]) + int(f["name"]["len"])]
                                                .decode(errors="replace"), int(s2[k])))
        self.stats.responses_host += n_host + len(host)

    REFS_PIECE = 1 << 16  # ref_directory: references read per kwok_read_refs call at most

    def _read_refs(self, which, first, count):
        """items [first, first + count) of a list of the collected tick: [(status, namespace, name, uid)]"""
        out = []
        for lo in range(first, first + count, self.REFS_PIECE):
            out += self.eng.ref_items(*self.eng.read_refs(which, lo, min(self.REFS_PIECE, first + count - lo)))
        return out

    def _apply_patches(self, kind, hs, offs, lens, which=None):
        i = n = 0
        ends = offs.astype(np.int64) + lens
        while i < len(hs):
            lo = int(offs[i])
            j = max(i + 1, int(np.searchsorted(ends, lo + READ_CHUNK, side="right")))
            buf = self.eng.read_arena(lo, int(ends[j - 1]) - lo).tobytes()
            refs = self._read_refs(which, i, j - i) if self.refs else None  # (the piece's references beside its bytes)
            for k in range(i, j):
                o = int(offs[k]) - lo
                self._apply(kind, int(hs[k]), buf[o:o + int(lens[k])], refs[k - i] if refs else None)
                n += 1
            i = j
        return n

    def _apply(self, kind, h, body, ref=None):
        """ref (ref_directory): the object's (status, namespace, name, uid) from the device, else the maps'"""
        cs = self.conf.client_set
        if ref is not None and ref[0] != abi.OK:  # no name stored: the body cannot be addressed
            self.stats.refs_missing += 1
            return
        if kind in (HEARTBEAT, NODE_INIT):  # configureHeartbeatNode / configureNode bodies
            try:
                obj = (cs.patch_node_status_raw if self.resp else cs.patch_node_status)(
                    ref[2].decode() if ref else self.node_name[h], body)
            except NotFound:
                return
            if self.resp:
                return self._response(obj)
            self._note(_meta(obj).get("uid"), _meta(obj).get("resourceVersion"))
        elif kind == POD_PATCH:  # LockPod (pod_controller.go:205-231)
            ns, name = (ref[1].decode(), ref[2].decode()) if ref else self.pod_ref[h]
            try:
                obj = (cs.patch_pod_status_raw if self.resp else cs.patch_pod_status)(ns, name, body)
            except NotFound:
                return
            if self.resp:  # (an empty status: its frame re-enters from the resident bytes)
                return self._response(obj, b'"podIP"' not in body)
            self._note(_meta(obj).get("uid"), _meta(obj).get("resourceVersion"))
            if b'"podIP"' not in body:  # an empty status: its echo re-enters (step 6)
                self.reenter.append(obj)
        else:  # DeletePod (pod_controller.go:155-183)
            ns, name = (ref[1].decode(), ref[2].decode()) if ref else self.pod_ref[h]
            if kind == DELETE_FIN:
                if self.finalizer is None:
                    from .engine import finalizer_patch
                    self.finalizer = finalizer_patch()
                try:
                    obj = (cs.patch_pod_raw if self.resp else cs.patch_pod)(ns, name, self.finalizer)
                except NotFound:
                    return
                if self.resp:
                    self._response(obj)
                else:
                    self._note(_meta(obj).get("uid"), _meta(obj).get("resourceVersion"))
            try:
                cs.delete_pod(ns, name)
            except NotFound:
                pass


def new_controller(conf: Config, backend=None) -> Controller:
    """NewController (controller.go:80): the engine-backed controller"""
    return Controller(conf, backend)
