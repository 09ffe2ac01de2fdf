/* kwok_canon.h - node status blobs canonicalised on the GPU.
 *
 * The node document codec on the device (kwok_decode_nodes_gpu, kwok_ingest_nodes_json,
 * kwok_ingest_nodes_framed, kwok_ingest_nodes_framed_echo) hands a document with a
 * non-empty status.addresses / allocatable / capacity to the host codec, which writes
 * the three values canonically (keys sorted bytewise, compact, Go string escaping).
 * With the switch below on, the device writes that form itself for every document
 * whose blobs are inside its domain, into a buffer of its own: the documents - and a
 * resident watch, List or response stream - are never written.  Every output is byte
 * for byte what the host codec path gives; only the count of documents the host codec
 * decoded (*n_host) falls.  The entries live in a header of their own because every
 * function kwok_engine.h declares has a twin in the oracle, and the older ABI tests
 * pick kwok_watch.h's entries by name.
 */
#ifndef KWOK_CANON_H
#define KWOK_CANON_H

#include "kwok_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    KWOK_CANON_STAT_DOCS = 0,   /* documents whose blobs the device canonicalised */
    KWOK_CANON_STAT_BLOBS,      /* their non-empty blobs */
    KWOK_CANON_STAT_BYTES_IN,   /* the raw bytes of those blobs */
    KWOK_CANON_STAT_BYTES_OUT,  /* their canonical bytes */
    KWOK_CANON_STAT_DOCS_HOST,  /* documents sent to the host codec because a blob was outside the device domain */
    KWOK_CANON_STAT_CALLS,      /* decode calls that launched the canon kernels */
    KWOK_CANON_STAT_COUNT
};

/* Switch the device canonicaliser on (on != 0) or off for the engine's node decodes.
 * Idempotent; off by default, and while it is off nothing is allocated or launched for
 * it.  Under a custom node template every record still goes through the host's
 * completion; the decode itself changes as elsewhere.  KWOK_EINVAL: a null engine. */
int kwok_canon_enable(kwok_engine* e, int on);

/* The counters since the engine was created (all zero while the switch was never on). */
int kwok_canon_stats(const kwok_engine* e, uint64_t out[KWOK_CANON_STAT_COUNT]);

#ifdef __cplusplus
}
#endif
#endif
