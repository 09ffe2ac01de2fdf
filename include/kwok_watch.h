/* kwok_watch.h - framing raw Kubernetes watch streams.
 *
 * A watch response is a byte stream of newline-terminated frames,
 * {"type":"MODIFIED","object":{...}}\n.  The framer finds, per line, the event
 * type, the byte span of the "object" value and the spans of the object's
 * metadata.uid / resourceVersion / name / namespace - what a controller needs
 * between the socket and the engine (pod_controller.go:272-343,
 * node_controller.go:225-279) - without building a DOM.  The GPU framer keeps
 * the stream resident, and the framed ingests decode documents straight from
 * it: no document byte crosses the link a second time.
 *
 * Framing rules (the same on host and device, frame for frame):
 *   - a frame is a line; *consumed is the offset just past the last newline
 *     (no newline: n_frames = 0, consumed = 0); the caller prepends the
 *     unconsumed tail to its next chunk;
 *   - every line yields a frame; a line of only whitespace (\r included) is
 *     KWOK_WATCH_NONE with status KWOK_OK;
 *   - a line is one JSON object in the codec's grammar (depth <= 64, lenient
 *     numbers, surrogate pairs); the first occurrence of a key wins;
 *   - "type" is one of the five words, "object" a JSON object; anything else,
 *     or malformed JSON, gives status KWOK_EINVAL for that frame only;
 *   - metadata.uid / resourceVersion / name / namespace of the object: the span
 *     inside the quotes (offsets into the stream); a non-string value gives an
 *     empty span; a string holding an escape sets its KWOK_FRAME_ESC_* bit and
 *     the span is the raw text.
 */
#ifndef KWOK_WATCH_H
#define KWOK_WATCH_H

#include "kwok_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    KWOK_WATCH_NONE = 0, /* blank line */
    KWOK_WATCH_ADDED,
    KWOK_WATCH_MODIFIED,
    KWOK_WATCH_DELETED,
    KWOK_WATCH_BOOKMARK,
    KWOK_WATCH_ERROR
};
enum { KWOK_FRAME_ESC_UID = 1, KWOK_FRAME_ESC_RV = 2, KWOK_FRAME_ESC_NAME = 4, KWOK_FRAME_ESC_NS = 8 };

typedef struct kwok_watch_frame {
    uint32_t line_off;         /* first byte of the line */
    uint32_t doc_off, doc_len; /* the "object" value, braces included (0, 0 unless status is KWOK_OK) */
    uint8_t type;              /* KWOK_WATCH_* */
    uint8_t flags;             /* KWOK_FRAME_ESC_* */
    int8_t status;             /* KWOK_OK / KWOK_EINVAL */
    uint8_t reserved0;
    kwok_str uid, resource_version, name, namespace_; /* inside the quotes; offsets into the stream */
} kwok_watch_frame;

/* the bytes of the stream one block of the line split covers, and the tiles one
 * step of the scan over the tile counts covers (stated for the tests) */
#define KWOK_WATCH_TILE_BYTES 16384
#define KWOK_WATCH_SCAN_TILES 1024

/* Host framer.  frames[cap]; *n_frames = the number of lines, *consumed = the
 * offset past the last newline.  KWOK_EINVAL (n_frames set) when cap is smaller
 * than the line count, and - before any byte is read - when len > 0xFFFFFFF0
 * (offsets are 32-bit).  Otherwise returns the number of frames whose status is
 * not KWOK_OK. */
int kwok_frame_watch(const char* stream, size_t len, kwok_watch_frame* frames, size_t cap, size_t* n_frames,
                     size_t* consumed);

/* GPU framer: uploads the stream once into a device buffer of its own, frames
 * it there and copies the frames back; the stream and its frames stay resident
 * under *stream_id (never 0) until the next framing call.  Lines the device
 * does not decide (an escape inside the type string or inside a key the scan
 * routes on: type, object, metadata, uid, resourceVersion, name, namespace) are
 * framed by the host framer from the caller's bytes and counted in *n_host.
 * The host buffer must stay valid and unchanged until the next framing call or
 * kwok_engine_destroy: the host codec completes undecided documents from it.
 * Return value and errors as kwok_frame_watch (a failed call leaves no stream
 * resident). */
int kwok_frame_watch_gpu(kwok_engine* e, const char* stream, size_t len, kwok_watch_frame* frames, size_t cap,
                         size_t* n_frames, size_t* consumed, size_t* n_host, uint64_t* stream_id);

/* kwok_ingest_pods_json / kwok_ingest_nodes_json over frames of the resident
 * stream: record i is frame frame_idx[i]; its op comes from the frame type
 * (ADDED / MODIFIED: KWOK_OP_UPSERT, DELETED: KWOK_OP_DELETE).  A frame index
 * out of range, a frame whose status is not KWOK_OK or whose type is NONE /
 * BOOKMARK / ERROR gives KWOK_EINVAL for that record and changes nothing.  A
 * stream_id that is not the resident one: KWOK_EINVAL for the call.  Several
 * calls, of both kinds, may follow one framing.  No document byte is uploaded. */
int kwok_ingest_pods_framed(kwok_engine* e, const kwok_codec* c, uint64_t stream_id, const uint32_t* frame_idx,
                            const int32_t* handle, size_t n, int32_t* out_handles, int32_t* out_status,
                            uint32_t* out_released, size_t* n_host);
int kwok_ingest_nodes_framed(kwok_engine* e, const kwok_codec* c, uint64_t stream_id, const uint32_t* frame_idx,
                             size_t n, int32_t* out_handles, int32_t* out_status, size_t* n_host);

enum {
    KWOK_WATCH_STAT_FRAMES = 0,   /* frames framed by kwok_frame_watch_gpu */
    KWOK_WATCH_STAT_HOST_FRAMES,  /* ... of them decided by the host framer */
    KWOK_WATCH_STAT_BYTES,        /* stream bytes uploaded */
    KWOK_WATCH_STAT_INGESTS,      /* framed ingest calls */
    KWOK_WATCH_STAT_COUNT
};
int kwok_watch_stats(kwok_engine* e, uint64_t out[KWOK_WATCH_STAT_COUNT]);

/* ---- List responses ---------------------------------------------
 *
 * A List body is one JSON value,
 *   {"kind":"PodList","apiVersion":"v1","metadata":{"resourceVersion":"..","continue":".."},"items":[{..},{..}]}
 * with no newline between its items.  The list framer gives one kwok_watch_frame
 * per item (type KWOK_WATCH_ADDED, doc_off / doc_len the item's span with its
 * braces, line_off == doc_off, the four metadata spans and KWOK_FRAME_ESC_* flags
 * exactly as the watch framer fills them for an `object`) and the envelope's
 * kwok_list_info.
 *
 * Rules (the same on host and device, frame for frame):
 *   - grammar: the body is one JSON object in the codec's grammar (depth <= 64
 *     counted from the root, lenient numbers, surrogate pairs), whitespace around it
 *     allowed; the first occurrence of a key wins at every level;
 *   - validity: a List decodes or it does not.  A body that is not a complete,
 *     valid JSON object - a truncated one included - or whose `items` is present and
 *     neither null nor an array of objects: KWOK_EINVAL for the call, *n_frames = 0,
 *     no frame written, no stream left resident.  Nothing is consumed in part;
 *   - `items` absent, null or []: zero frames, KWOK_OK.  `kind` is reported, not
 *     judged: sending a PodList to the pod ingest is the caller's decision;
 *   - guards: cap below the item count: KWOK_EINVAL with *n_frames set;
 *     len > 0xFFFFFFF0: KWOK_EINVAL before any byte is read;
 *   - an item without `metadata`, or with non-string members: empty spans, status OK;
 *   - escapes: a routed key (the root's items / metadata / kind, the root
 *     metadata's resourceVersion / continue, an item's metadata and its uid /
 *     resourceVersion / name / namespace) holding an escape is compared as decoded
 *     text, never guessed.  The device lists such an item for the host (*n_host),
 *     which frames it from the caller's bytes; a body whose envelope the device does
 *     not decide (no single array directly under the root that the envelope
 *     confirms as the first `items`) is framed whole by the host framer
 *     (KWOK_LIST_STAT_HOST_BODIES).
 *   - info: the spans of the root's kind, metadata.resourceVersion and
 *     metadata.continue, inside their quotes (empty when the value is absent, empty
 *     or not a string; KWOK_LIST_ESC_* set when the raw text holds an escape), and
 *     the span of the `items` array, brackets included (empty unless an array). */
enum { KWOK_LIST_ESC_KIND = 1, KWOK_LIST_ESC_RV = 2, KWOK_LIST_ESC_CONTINUE = 4 };

typedef struct kwok_list_info {
    kwok_str kind, resource_version, continue_; /* inside the quotes; offsets into the body */
    kwok_str items;                             /* the items array, brackets included */
    uint32_t flags;                             /* KWOK_LIST_ESC_* */
    uint32_t reserved0;
} kwok_list_info;

/* Host framer, the yardstick.  frames[cap]; *n_frames = the item count.  Returns
 * KWOK_OK or KWOK_EINVAL (rules above). */
int kwok_frame_list(const char* body, size_t len, kwok_watch_frame* frames, size_t cap, size_t* n_frames,
                    kwok_list_info* info);

/* GPU framer: uploads the body once, frames it there and copies the frames back.
 * The body stays resident as THE stream under *stream_id (it replaces a watch
 * stream, as every framing call does); kwok_ingest_pods_framed /
 * kwok_ingest_nodes_framed then run on it unchanged (ADDED: KWOK_OP_UPSERT).
 * *n_host: the items the host framed.  The caller's buffer must stay valid and
 * unchanged until the next framing call or kwok_engine_destroy.  Return value and
 * errors as kwok_frame_list; a failed call leaves no stream resident. */
int kwok_frame_list_gpu(kwok_engine* e, const char* body, size_t len, kwok_watch_frame* frames, size_t cap,
                        size_t* n_frames, kwok_list_info* info, size_t* n_host, uint64_t* stream_id);

enum {
    KWOK_LIST_STAT_BODIES = 0,   /* bodies given to kwok_frame_list_gpu (past its argument checks) */
    KWOK_LIST_STAT_ITEMS,        /* items framed */
    KWOK_LIST_STAT_HOST_ITEMS,   /* ... of them framed by the host (an escaped routed key) */
    KWOK_LIST_STAT_HOST_BODIES,  /* bodies handed whole to the host framer */
    KWOK_LIST_STAT_BYTES,        /* body bytes uploaded */
    KWOK_LIST_STAT_COUNT
};
int kwok_list_stats(kwok_engine* e, uint64_t out[KWOK_LIST_STAT_COUNT]);

/* ---- Relist with Replace ---------------------------------------
 *
 * A watch that fell behind is closed with 410 Gone; the reference opens a fresh one
 * (pod_controller.go:280-290, node_controller.go:235-245) and never sees the Deleted
 * events of the gap.  A resync session closes that gap the way client-go's reflector
 * does: list again, then remove what the list did not hold.  A session is per kind
 * (nodes, pods); it collects one `seen` mark per slot and is closed by a sweep.
 *
 * Rules:
 *   - begin: opens the kind's session with every mark cleared; a second begin
 *     restarts it, marks cleared again.  Marks exist only inside a session;
 *   - marks: while the kind's session is open, every KWOK_OP_UPSERT record of that
 *     kind whose final per-record status is KWOK_OK marks the slot of the handle it
 *     returned - through every ingest entry (kwok_ingest_nodes, kwok_ingest_pods,
 *     _packed, _packed12, _packed12_tick, kwok_ingest_pods_json,
 *     kwok_ingest_nodes_json, kwok_ingest_pods_framed, kwok_ingest_nodes_framed),
 *     records the host completed included (a kwok_pod_rec12 update: its target).
 *     A DELETE marks nothing, a rejected record marks nothing;
 *   - kwok_resync_mark: marks objects the caller saw in the list and did not ingest
 *     (an item it dropped as the echo of the engine's own patch).  A handle out of
 *     range, in a bucket this rank does not own, or whose slot is not in use is
 *     counted in *n_bad and marks nothing;
 *   - sweep: closes the session.  Every live object of the kind without a mark is
 *     removed in canonical order (ascending handle) with the effect of a Deleted
 *     watch event for it.  Pods (pod_controller.go:320-343): live is a used slot, a
 *     delete-pending pod included; the event's status.podIP is the address the slot
 *     holds, so Put(ip) runs if the node is managed and the address is in the CIDR
 *     (:329-336; nothing with EnableCNI, :337-342: the caller runs cni.Remove for
 *     out_node's managed nodes), the slot is freed, a zombie node entry nothing
 *     references any more goes, and the foreign-IP flag is not raised.  Nodes
 *     (node_controller.go:265-269): nodesSets.Delete; the entry lives on as a zombie
 *     while pods reference it.  The removals are DELETE records built on the device
 *     and run through the ingest's own event switch, so every side effect (heartbeat
 *     handle bases, the handle-list epoch, quiet-tick state) is a Deleted event's;
 *   - the sweep drains submitted ticks first, as every ingest does; it is refused
 *     with KWOK_EINVAL on a multi-rank engine and with the poisoned code on a
 *     poisoned one.  cap below the number of unmarked objects: KWOK_EINVAL with
 *     *n_swept set, nothing removed, the session stays open (retry with larger
 *     arrays);
 *   - end: closes the session without sweeping.  A sweep or a mark without an open
 *     session: KWOK_EINVAL, nothing changes. */
enum { KWOK_KIND_NODES = 0, KWOK_KIND_PODS = 1 };
int kwok_resync_begin(kwok_engine* e, int kind);
int kwok_resync_mark(kwok_engine* e, int kind, const int32_t* handles, size_t n, size_t* n_bad);
/* out_handles[cap]: the swept handles, ascending; *n_swept their number.  Pods,
 * optional: out_released[i] the address put back for swept pod i (0: none),
 * out_node[i] its node's handle.  Returns KWOK_OK or an error. */
int kwok_resync_sweep(kwok_engine* e, int kind, int32_t* out_handles, size_t cap, size_t* n_swept,
                      uint32_t* out_released, int32_t* out_node);
int kwok_resync_end(kwok_engine* e, int kind);
enum {
    KWOK_RESYNC_STAT_SESSIONS = 0, /* begins */
    KWOK_RESYNC_STAT_MARKED,       /* marks stored: ingested records + explicit marks */
    KWOK_RESYNC_STAT_SWEPT_NODES,
    KWOK_RESYNC_STAT_SWEPT_PODS,
    KWOK_RESYNC_STAT_RELEASED,     /* addresses the swept pods put back */
    KWOK_RESYNC_STAT_COUNT
};
int kwok_resync_stats(kwok_engine* e, uint64_t out[KWOK_RESYNC_STAT_COUNT]);

/* ---- Pod uid directory ------------------------------------------
 *
 * metadata.uid -> pod handle, kept on the device.  With it enabled a framed pod
 * batch needs no handle[] from the caller: kwok_ingest_pods_framed_uid resolves
 * every frame's uid, cuts the batch into runs and binds the pods it creates, all on
 * the device.  The yardstick is the host path, record for record: the batch cut into
 * runs in which no new pod appears twice, each run through kwok_ingest_pods_framed
 * with handles from a uid -> handle map of the caller (controller.ingest_pod_runs).
 *
 * Rules:
 *   - a run resolves every record of its range before any of them is applied: a
 *     Deleted and an Added of one known uid in one run both carry its handle;
 *   - cuts are positional.  In the current range [lo, n), `created` is the set of
 *     uids the directory does not hold that appear in a non-DELETED record; the run
 *     ends before the first record whose uid an earlier record put into `created`,
 *     and everything from there on (records of other pods included) waits for the
 *     next run, which resolves again.  *n_runs counts the runs that sent a record;
 *   - a DELETED frame of a uid that resolves to nothing (a pod the tick or a sweep
 *     already removed included): KWOK_NOT_SENT, handle -1, nothing changes;
 *   - a non-DELETED record that ended KWOK_OK binds its uid to the handle it
 *     returned; any other status binds nothing (a failed create's uid is new again);
 *   - a frame with KWOK_FRAME_ESC_UID, or whose uid is empty or longer than
 *     KWOK_UID_MAX: KWOK_EDOMAIN, handle -1, nothing changes (never guessed or
 *     truncated);
 *   - a frame out of range, not KWOK_OK or of type NONE / BOOKMARK / ERROR:
 *     KWOK_EINVAL, as kwok_ingest_pods_framed;
 *   - a binding ends with its pod: whatever frees the slot (a Deleted event, the
 *     engine's tick, a sweep) unbinds the uid.  A pod created through an entry that
 *     carries no uid (typed events, records, kwok_ingest_pods_framed) has none
 *     until kwok_uid_bind names it;
 *   - single-rank engines only (a rank does not see other ranks' pods): enable is
 *     refused with KWOK_EINVAL on a multi-rank engine. */
#define KWOK_UID_MAX 40  /* a Kubernetes uid is a 36-byte UUID */
#define KWOK_NOT_SENT 1  /* per-record status: a Deleted event of a pod the engine does not hold */
/* Allocates the directory (idempotent).  Pods that exist have no uid until bound. */
int kwok_uid_dir_enable(kwok_engine* e);
/* uid i = arena[off[i], +len[i]) becomes the uid of live pod handles[i] (rebinding replaces it).
 * Counted in *n_bad, binding nothing: a handle out of range, in a bucket this rank does not
 * own or on an unused slot, a uid that is empty or longer than KWOK_UID_MAX.  One handle
 * named twice in a call keeps either uid. */
int kwok_uid_bind(kwok_engine* e, const int32_t* handles, const char* arena, const uint64_t* off, const uint32_t* len,
                  size_t n, size_t* n_bad);
/* out_handles[i]: the live pod bound to uid i, or -1.  Drains submitted ticks first. */
int kwok_uid_lookup(kwok_engine* e, const char* arena, const uint64_t* off, const uint32_t* len, size_t n,
                    int32_t* out_handles);
/* kwok_ingest_pods_framed without handle[] (rules above).  *n_host: documents the host
 * codec decided; *n_runs: the runs.  KWOK_EINVAL for the call when the directory is not
 * enabled or stream_id is not the resident stream.  Returns the number of records whose
 * status is neither KWOK_OK nor KWOK_NOT_SENT, or an error. */
int kwok_ingest_pods_framed_uid(kwok_engine* e, const kwok_codec* c, uint64_t stream_id, const uint32_t* frame_idx,
                                size_t n, int32_t* out_handles, int32_t* out_status, uint32_t* out_released,
                                size_t* n_host, size_t* n_runs);
enum {
    KWOK_UID_STAT_LOOKUPS = 0,   /* keyable uids probed (framed records and kwok_uid_lookup) */
    KWOK_UID_STAT_HITS,          /* ... that resolved to a live pod */
    KWOK_UID_STAT_BINDS,         /* creates noted plus explicit binds */
    KWOK_UID_STAT_UNBOUND,       /* creates through entries that carry no uid */
    KWOK_UID_STAT_RUNS,          /* runs that sent a record */
    KWOK_UID_STAT_CUTS,          /* run cuts */
    KWOK_UID_STAT_REBUILDS,      /* table rebuilds */
    KWOK_UID_STAT_TABLE_ENTRIES, /* entries the table holds, stale ones included */
    KWOK_UID_STAT_COUNT
};
int kwok_uid_stats(kwok_engine* e, uint64_t out[KWOK_UID_STAT_COUNT]);

/* ---- Echo ledger ------------------------------------------------
 *
 * The engine's own patches come back on the watch; a controller drops those echoes
 * by (uid, resourceVersion).  With the ledger enabled that filter runs on the device:
 * the framed ingests below take ALL frames of a batch, decide the echoes under the
 * rule of controller.Echoes as _encode / _ingest_frames apply it, and ingest the rest.
 *
 * The ledger maps a uid to an ordered list of at most KWOK_ECHO_KEEP resourceVersions
 * (opaque bytes, compared byte for byte):
 *   - note(uid, rv) appends; an empty uid or rv is ignored; a ninth note drops the
 *     oldest; one rv noted twice is held twice;
 *   - forget(uid) removes every note of the uid;
 *   - filter, over the records of one call in record order (`seen` empty per call):
 *       a non-ingestible frame touches neither the ledger nor `seen`;
 *       DELETED: never an echo; kept, the uid joins `seen` and is forgotten;
 *       ADDED / MODIFIED: m = the uid's list holds rv; if m its first occurrence is
 *       removed (dropped or not); the record is dropped iff m and the uid is not in
 *       `seen`; a record that is not dropped is kept and its uid joins `seen`.
 * Single-rank engines only. */
#define KWOK_RV_MAX 24
#define KWOK_ECHO_KEEP 8
#define KWOK_ECHO 2 /* per-record status: a frame dropped as the echo of an own patch */
enum { KWOK_ECHO_NOTE = 0, KWOK_ECHO_FORGET = 1 };
/* Allocates the ledger (idempotent).  KWOK_EINVAL on a multi-rank engine. */
int kwok_echo_enable(kwok_engine* e);
/* op[i] (KWOK_ECHO_NOTE / KWOK_ECHO_FORGET) on uid i = arena[uid_off[i], +uid_len[i]) with
 * rv i = arena[rv_off[i], +rv_len[i]) (a forget reads no rv), applied in array order per
 * uid.  out_status[i] (optional): KWOK_OK applied, or an ignored empty uid / rv;
 * KWOK_EDOMAIN a uid longer than KWOK_UID_MAX or a noted rv longer than KWOK_RV_MAX
 * (nothing stored); KWOK_EINVAL an unknown op.  A uid need not belong to a live object.
 * KWOK_EFULL for the call, nothing stored, when a table forced by KWOK_ECHO_TAB_LOG2
 * cannot take the call's notes.  Returns the number of ops not KWOK_OK, or an error. */
int kwok_echo_update(kwok_engine* e, const uint8_t* op, const char* arena, const uint64_t* uid_off,
                     const uint32_t* uid_len, const uint64_t* rv_off, const uint32_t* rv_len, size_t n,
                     int32_t* out_status);
/* The filter over typed events: deleted[i] != 0 is a Deleted event.  out_drop[i] = 1: a
 * dropped echo.  An empty uid or one longer than KWOK_UID_MAX is never an echo; an rv that
 * is empty or longer than KWOK_RV_MAX matches nothing. */
int kwok_echo_match(kwok_engine* e, const char* arena, const uint64_t* uid_off, const uint32_t* uid_len,
                    const uint64_t* rv_off, const uint32_t* rv_len, const uint8_t* deleted, size_t n,
                    uint8_t* out_drop);
/* All frames of a batch: the filter first, then the kept records through exactly what
 * kwok_ingest_pods_framed_uid / kwok_ingest_nodes_framed do with that subset.  A dropped
 * record: KWOK_ECHO with the handle its uid (pods) or name (nodes) resolves to before the
 * ingest, or -1.  A frame with KWOK_FRAME_ESC_UID or KWOK_FRAME_ESC_RV: KWOK_EDOMAIN,
 * handle -1, nothing changes, the ledger untouched.  A non-ingestible frame: KWOK_EINVAL.
 * An empty uid or one longer than KWOK_UID_MAX is never an echo and follows the
 * underlying entry.  *n_echoes: the dropped records.  The pod entry needs the uid
 * directory; both need the ledger (KWOK_EINVAL otherwise).  Returns the number of
 * records whose status is none of KWOK_OK / KWOK_NOT_SENT / KWOK_ECHO, or an error. */
int kwok_ingest_pods_framed_echo(kwok_engine* e, const kwok_codec* c, uint64_t stream_id, const uint32_t* frame_idx,
                                 size_t n, int32_t* out_handles, int32_t* out_status, uint32_t* out_released,
                                 size_t* n_host, size_t* n_runs, size_t* n_echoes);
int kwok_ingest_nodes_framed_echo(kwok_engine* e, const kwok_codec* c, uint64_t stream_id, const uint32_t* frame_idx,
                                  size_t n, int32_t* out_handles, int32_t* out_status, size_t* n_host,
                                  size_t* n_echoes);
enum {
    KWOK_ECHO_STAT_NOTES = 0,     /* notes stored */
    KWOK_ECHO_STAT_FORGETS,       /* forgets (ops and Deleted records) that removed a note */
    KWOK_ECHO_STAT_EVICTIONS,     /* ninth notes */
    KWOK_ECHO_STAT_MATCHED,       /* records whose (uid, rv) was noted */
    KWOK_ECHO_STAT_DROPPED,       /* ... dropped as echoes */
    KWOK_ECHO_STAT_KEPT_MATCHED,  /* ... kept: an earlier record of the uid in the call */
    KWOK_ECHO_STAT_REBUILDS,
    KWOK_ECHO_STAT_LIVE_UIDS,     /* uids holding a note */
    KWOK_ECHO_STAT_TABLE_ENTRIES, /* entries of the table, emptied ones included */
    KWOK_ECHO_STAT_COUNT
};
int kwok_echo_stats(kwok_engine* e, uint64_t out[KWOK_ECHO_STAT_COUNT]);

/* ---- Pod and node reference directory ---------------------------
 *
 * What a patch is addressed to - a pod's namespace, name and uid, a node's name - kept
 * on the device and handed back in the order of the tick's output lists, so a caller
 * keeps no per-object map for addressing.
 *
 * Rules:
 *   - per pod slot the namespace and the name (opaque bytes: namespace <= 63, name
 *     1..253) are stored; the uid is the uid directory's; a node's name is the node
 *     directory's (nodes carry no namespace and no uid here);
 *   - while the directory is on, every pod create (an UPSERT without a handle whose
 *     final status is KWOK_OK) through a by-uid entry (kwok_ingest_pods_framed_uid,
 *     kwok_ingest_pods_framed_echo) stores its frame's namespace and name from the
 *     resident stream; a frame with KWOK_FRAME_ESC_NAME / _NS, an empty name, a name
 *     over 253 bytes or a namespace over 63 stores none (never truncated or guessed).
 *     A create through any other entry stores none: a reused slot never keeps its
 *     previous pod's name.  An upsert of a known pod stores nothing;
 *   - kwok_refs_bind names the pods that have none (typed events, records, escaped
 *     frames whose decoded text the caller holds);
 *   - whatever frees a slot (a Deleted event, the tick, a sweep) leaves its bytes:
 *     KWOK_REFS_DELETE and KWOK_REFS_ANY_SLOT answer from them until the slot is
 *     created into again;
 *   - stale guard: every call that can create an object of a kind (its ingest entries,
 *     kwok_refs_bind for pods) moves that kind's counter; kwok_read_refs refuses a
 *     list of a kind whose counter moved since the collected tick's submit
 *     (KWOK_EINVAL; kwok_last_error says so).  Flush, tick, apply never trips it;
 *   - single-rank engines only.
 *
 * Output: refs[i] describes item i; its bytes are namespace, name, uid, concatenated
 * at blob + refs[i].off.  Every off is a multiple of 16, items lie in list order and
 * an item's tail is zero up to the next multiple of 16; *blob_used is the total.
 * blob_cap below the total: KWOK_EINVAL, *blob_used set to the need, nothing
 * written. */
#define KWOK_REF_NS_MAX 63
#define KWOK_REF_NAME_MAX 253
#define KWOK_REF_STRIDE 320 /* bytes per pod slot: 63 + 253 rounded up to 16-byte units */
#define KWOK_REF_NONE 3     /* kwok_ref.status: a live pod with no name stored */
#define KWOK_REFS_ANY_SLOT 1 /* kwok_refs_lookup flag: what the slot last stored, live or not */
typedef struct kwok_ref {
    uint64_t off;                     /* into blob, a multiple of 16 */
    uint8_t ns_len, name_len, uid_len;
    int8_t status;                    /* KWOK_OK / KWOK_ENOTFOUND / KWOK_REF_NONE (lengths 0, the uid given if known) */
    uint32_t reserved0;
} kwok_ref;
enum { KWOK_REFS_HEARTBEAT = 0, KWOK_REFS_NODE_INIT, KWOK_REFS_POD_PATCH, KWOK_REFS_DELETE, KWOK_REFS_LIST_COUNT };
/* Allocates the directory and enables the uid directory (idempotent).  Pods that exist
 * have no name until bound.  KWOK_EINVAL on a multi-rank engine. */
int kwok_refs_enable(kwok_engine* e);
/* namespace i = arena[ns_off[i], +ns_len[i]) and name i = arena[name_off[i], +name_len[i])
 * become those of live pod handles[i] (rebinding replaces them).  Counted in *n_bad,
 * storing nothing: a handle out of range or on an unused slot, an empty name, a name over
 * KWOK_REF_NAME_MAX, a namespace over KWOK_REF_NS_MAX.  One handle named twice in a call is the caller's error
 * (its record then holds 16-byte units of either).  Drains submitted ticks first. */
int kwok_refs_bind(kwok_engine* e, const int32_t* handles, const char* arena, const uint64_t* ns_off,
                   const uint32_t* ns_len, const uint64_t* name_off, const uint32_t* name_len, size_t n, size_t* n_bad);
/* The references of handles[0, n) of `kind` (KWOK_KIND_PODS / KWOK_KIND_NODES) in the
 * caller's order.  A handle out of range or not live: KWOK_ENOTFOUND, all lengths 0;
 * with KWOK_REFS_ANY_SLOT a handle in range answers what its slot last stored (ask
 * before the next ingest of that kind).  Drains submitted ticks first. */
int kwok_refs_lookup(kwok_engine* e, int kind, const int32_t* handles, size_t n, uint32_t flags, kwok_ref* refs,
                     char* blob, size_t blob_cap, size_t* blob_used);
/* Items [first, first + count) of output list `which` (KWOK_REFS_*) of the last collected
 * tick, read on the device (no handle is uploaded).  A range outside the list, no
 * collected tick, or a moved counter (the stale guard): KWOK_EINVAL. */
int kwok_read_refs(kwok_engine* e, int which, size_t first, size_t count, kwok_ref* refs, char* blob, size_t blob_cap,
                   size_t* blob_used);
enum {
    KWOK_REFS_STAT_BINDS = 0, /* names stored by kwok_refs_bind */
    KWOK_REFS_STAT_NOTES,     /* names stored by ingests (creates through a by-uid entry) */
    KWOK_REFS_STAT_UNNAMED,   /* creates stored without a name */
    KWOK_REFS_STAT_READS,     /* references read (kwok_refs_lookup and kwok_read_refs items) */
    KWOK_REFS_STAT_NOT_FOUND, /* ... of them KWOK_ENOTFOUND */
    KWOK_REFS_STAT_BYTES,     /* device memory the directory holds (the uid directory's not included) */
    KWOK_REFS_STAT_COUNT
};
int kwok_refs_stats(kwok_engine* e, uint64_t out[KWOK_REFS_STAT_COUNT]);

/* ---- Node uid directory and batched name lookup -------------------
 *
 * A node's uid kept per node slot on the device, and the node directory's
 * name -> handle lookup for a whole batch, so a caller keeps no per-node map.
 *
 * The uid rule, applied behind every node batch while the directory is on, per
 * bucket in event order (controller.py's _node_put / _node_pop):
 *   - a DELETE record that ended KWOK_OK marks the slot's uid stale and leaves its
 *     bytes (a swept node's uid stays answerable under KWOK_REFS_ANY_SLOT);
 *   - any other record that ended KWOK_OK on a slot with no uid or a stale one
 *     stores the record's uid and clears stale; on a slot with a live uid it stores
 *     nothing (a known node keeps its uid);
 *   - the record's uid: through kwok_ingest_nodes_framed / _framed_echo the frame's
 *     uid span in the resident stream, if the frame has no KWOK_FRAME_ESC_UID and the
 *     uid is 1..KWOK_UID_MAX bytes; otherwise, and through every other entry
 *     (kwok_ingest_nodes, kwok_ingest_nodes_json, a sweep's DELETE records), none:
 *     length 0 is stored, so a reused slot never answers its previous node's uid.
 *     Nothing is truncated or guessed.
 * With the directory on, the reference directory's node answers carry the uid behind
 * the name: a node whose uid is not stale answers it, else uid_len 0;
 * KWOK_REFS_ANY_SLOT (and kwok_read_refs) answers what the slot last stored, stale
 * or not, and a slot whose entry is gone but whose uid remains answers KWOK_REF_NONE
 * with that uid.  With it off every node answer is what it was.
 * Single-rank engines only (kwok_node_lookup excepted). */
/* Allocates the directory (idempotent): KWOK_UID_MAX + 9 bytes per node slot (the uid, its length byte and
 * the key of the entry it was stored for: a placeholder made in a freed slot never answers another node's uid).  Nodes that
 * exist have no uid until bound.  KWOK_EINVAL on a multi-rank engine. */
int kwok_node_dir_enable(kwok_engine* e);
/* out_handles[i]: the existing node named arena[off[i], +len[i]), or -1 (an empty name, one
 * over KWOK_REF_NAME_MAX bytes, one in a bucket this rank does not own, a deleted node that
 * pods still reference, a placeholder).  kwok_node_has for a batch, answering handles.
 * Needs no directory enabled; drains submitted ticks first. */
int kwok_node_lookup(kwok_engine* e, const char* arena, const uint64_t* off, const uint32_t* len, size_t n,
                     int32_t* out_handles);
/* uid i = arena[off[i], +len[i]) becomes the uid of existing node handles[i] (replacing a
 * stored one, clearing stale).  Counted in *n_bad, storing nothing: a handle out of range or
 * of no existing node, a uid that is empty or longer than KWOK_UID_MAX. */
int kwok_node_bind(kwok_engine* e, const int32_t* handles, const char* arena, const uint64_t* off,
                       const uint32_t* len, size_t n, size_t* n_bad);
enum {
    KWOK_NODE_DIR_STAT_LOOKUPS = 0, /* names probed (kwok_node_lookup and the echo entry's dropped records) */
    KWOK_NODE_DIR_STAT_HITS,        /* ... that resolved to an existing node */
    KWOK_NODE_DIR_STAT_NOTES,       /* uids stored by ingests */
    KWOK_NODE_DIR_STAT_BINDS,       /* uids stored by kwok_node_bind */
    KWOK_NODE_DIR_STAT_UNBOUND,     /* creates stored without a uid (an entry or a frame that carries none) */
    KWOK_NODE_DIR_STAT_BYTES,       /* device memory the directory holds */
    KWOK_NODE_DIR_STAT_COUNT
};
/* All zero while the directory is off. */
int kwok_node_dir_stats(kwok_engine* e, uint64_t out[KWOK_NODE_DIR_STAT_COUNT]);

/* ---- Patch responses ----------------------------------------------
 *
 * The response to one of the engine's own patches is the patched object itself,
 *   {"kind":"Pod","metadata":{..},..}
 * without a {"type":..,"object":..} envelope.  Bodies arrive with a known length and may
 * hold newlines (?pretty), so the caller concatenates them and gives their spans: no
 * line split.  The response framer gives one kwok_watch_frame per body; the notes of the
 * echo ledger (kwok_response.h) and the re-entry of pods patched without a podIP are then
 * taken from the resident bytes.
 *
 * Rules (the same on host and device, frame for frame):
 *   - document i is buf[off[i], +dlen[i]); a span that does not lie inside [0, len):
 *     KWOK_EINVAL for that frame only; len > 0xFFFFFFF0: KWOK_EINVAL for the call before
 *     any byte is read;
 *   - whitespace before and after the value is skipped (the apiserver's trailing \n); an
 *     empty or all-whitespace span: KWOK_WATCH_NONE with status KWOK_OK;
 *   - the value is one JSON object in the codec's grammar (depth <= 64 counted from the
 *     body's root, the first occurrence of a key wins); anything else, or bytes behind
 *     the value: KWOK_EINVAL;
 *   - an OK frame: type KWOK_WATCH_MODIFIED, line_off = off[i], doc_off / doc_len the
 *     object with its braces, the four metadata spans and KWOK_FRAME_ESC_* flags exactly
 *     as the watch framer fills them for the same object.  Only the root's own `metadata`
 *     is read (spec.template.metadata is not);
 *   - an escape in a routed key (metadata, uid, resourceVersion, name, namespace) sends
 *     the document to the host framer (*n_host). */
/* Host framer.  frames[n].  Returns the number of frames whose status is not KWOK_OK, or
 * KWOK_EINVAL. */
int kwok_frame_responses(const char* buf, size_t len, const uint64_t* off, const uint32_t* dlen, size_t n,
                         kwok_watch_frame* frames);
/* GPU framer: uploads buf once, frames the documents there (k_resp_parse) and copies the
 * frames back.  The buffer and its frames become THE resident stream under *stream_id
 * (never 0), replacing whatever was resident, as kwok_frame_watch_gpu does: every framed
 * entry that takes a stream_id then works on response frames unchanged (MODIFIED:
 * KWOK_OP_UPSERT).  The caller's buffer must stay valid and unchanged until the next
 * framing call or kwok_engine_destroy.  Return value as kwok_frame_responses; a failed
 * call leaves no stream resident. */
int kwok_frame_responses_gpu(kwok_engine* e, const char* buf, size_t len, const uint64_t* off, const uint32_t* dlen,
                             size_t n, kwok_watch_frame* frames, size_t* n_host, uint64_t* stream_id);
enum {
    KWOK_RESP_STAT_FRAMES = 0,   /* frames framed by kwok_frame_responses_gpu */
    KWOK_RESP_STAT_HOST_FRAMES,  /* ... of them decided by the host framer */
    KWOK_RESP_STAT_BYTES,        /* buffer bytes uploaded */
    KWOK_RESP_STAT_NOTE_CALLS,   /* note calls over response frames (kwok_response.h), past their checks */
    KWOK_RESP_STAT_NOTES,        /* records they keyed as notes (stored ones count under KWOK_ECHO_STAT_NOTES too) */
    KWOK_RESP_STAT_COUNT
};
int kwok_response_stats(kwok_engine* e, uint64_t out[KWOK_RESP_STAT_COUNT]);

#ifdef __cplusplus
}
#endif
#endif
