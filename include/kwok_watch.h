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

#ifdef __cplusplus
}
#endif
#endif
