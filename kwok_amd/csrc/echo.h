// echo.h - the echo ledger (echo.hip, kwok_watch.h): layouts shared by
// the host runtime and the kernels.  Kept out of DevState and kernels.h: no kernel
// outside echo.hip sees the ledger.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kwok_watch.h"
#include "kernels.h"

namespace kwok {

// one noted uid: its bytes and up to KWOK_ECHO_KEEP resourceVersions, oldest first
struct EchoEntry {  // 256 bytes
    uint64_t hash;  // FNV-1a-64 of the uid
    uint8_t uid[KWOK_UID_MAX];
    uint8_t ulen, cnt;  // cnt 0: emptied (the uid may note again; no other uid takes the entry)
    uint8_t rlen[KWOK_ECHO_KEEP];
    uint8_t pad[6];
    uint8_t rv[KWOK_ECHO_KEEP][KWOK_RV_MAX];
};
static_assert(sizeof(EchoEntry) == 256, "a ledger entry is 256 bytes");

struct EchoCounters {  // device memory, read back by the host
    unsigned long long notes, forgets, evictions, matched, dropped, kept_matched;
    unsigned long long live;  // entries with cnt > 0
    uint32_t used;            // pool entries handed out since the last rebuild
    uint32_t err;             // a probe wrapped the whole table, or the pool ran out
};
struct EchoCall {  // per call, reset by the host, read back once
    uint32_t n_rep;      // records that are not the first of their uid
    uint32_t list_used;  // the repeat lists handed out
    uint32_t n_keep;     // framed: records that go on to the ingest
    uint32_t n_drop;     // dropped echoes
    uint32_t n_bad;      // update: ops whose status is not KWOK_OK
    uint32_t err;        // the scratch tables wrapped or ran over
    uint32_t n_new;      // update: uids with a note and no entry that holds one (each may take a pool entry)
    uint32_t n_note;     // note_framed: records keyed as notes
};

// tab: [mask + 1] pool index + 1 (0: empty) at the low bits of the uid's hash, linear probing
struct EchoLedger {
    uint32_t* tab;
    uint32_t mask;
    EchoEntry* pool;
    uint32_t pool_cap;
    EchoCounters* ctr;
};

// what a record asks of the ledger
enum : uint8_t { EK_SKIP = 0, EK_UPSERT, EK_DELETE, EK_NOTE, EK_FORGET };
// a framed record's answer
enum : uint8_t { ER_KEEP = 0, ER_DROP, ER_EINVAL, ER_EDOMAIN };

struct EchoBatch {
    const uint8_t* base;  // the resident stream, or the call's arena
    uint64_t base_len;
    uint32_t n;
    uint32_t* uoff;  // [n] keyed records: the uid span, the rv span (rlen 0: matches nothing), the hash
    uint32_t* roff;
    uint8_t* ulen;
    uint8_t* rlen;
    uint64_t* hash;
    uint8_t* kind;  // [n] EK_*
    uint8_t* res;   // [n] ER_* (update: 1 = the uid needs an entry)
    uint32_t* claim;  // [claim_mask + 1] >= 2n record indices, ~0: empty
    uint32_t claim_mask;
    uint32_t* own;    // [n] the first record of the record's uid
    uint32_t* cnt;    // [n] an owner's repeats (zeroed per call)
    uint32_t* fill;   // [n] (zeroed per call)
    uint32_t* lbase;  // [n] an owner's list in list[]
    uint32_t* list;   // [n]
    EchoCall* call;
};

// the typed front end's inputs (update: op; match: deleted) on the device
struct EchoSpans {
    const uint64_t *uid_off, *rv_off;
    const uint32_t *uid_len, *rv_len;
    const uint8_t* op;
};
// the framed front end's
struct EchoFrames {
    const kwok_watch_frame* frames;
    uint32_t n_frames;
    const uint32_t* frame_idx;  // [n]
};
// the framed back end: the kept records' frame indices in record order, each record's place among them
struct EchoKeep {
    uint32_t* bsum;   // [blocks + 1]
    uint32_t* kidx;   // [n] kept frame indices
    uint32_t* kpos;   // [n]
    uint64_t* q_off;  // [n] k_uid_lookup's inputs: a dropped record's uid (len 0 otherwise)
    uint32_t* q_len;
};

void launch_echo_key_update(const EchoBatch& B, const EchoSpans& P, int32_t* status, hipStream_t st);
void launch_echo_key_typed(const EchoBatch& B, const EchoSpans& P, hipStream_t st);
void launch_echo_key_frames(const EchoBatch& B, const EchoFrames& F, hipStream_t st);
// k_echo_key_note_frames: every ingestible frame a note of its (uid, rv); status[i] as kwok_echo_note_framed states it
void launch_echo_key_note_frames(const EchoBatch& B, const EchoFrames& F, int32_t* status, hipStream_t st);
// k_echo_claim, k_echo_group, k_echo_alloc, k_echo_scatter
void launch_echo_group(const EchoBatch& B, hipStream_t st);
// k_echo_need: the call's n_new, before anything is stored
void launch_echo_need(const EchoLedger& L, const EchoBatch& B, hipStream_t st);
// k_echo_apply (uids the ledger holds), k_echo_insert (the others)
void launch_echo_update(const EchoLedger& L, const EchoBatch& B, hipStream_t st);
void launch_echo_decide(const EchoLedger& L, const EchoBatch& B, hipStream_t st);
// k_echo_count, k_echo_scan, k_echo_keep
void launch_echo_keep(const EchoBatch& B, const EchoFrames& F, const EchoKeep& K, hipStream_t st);
// a dropped node frame's handle: its name in the device node directory
void launch_echo_node_handles(const DevState& S, const EchoBatch& B, const EchoFrames& F, int32_t* hdrop, hipStream_t st);
// the call's results: kept records take the ingest's (at kpos), withheld ones their answer
void launch_echo_fix(const EchoBatch& B, const EchoKeep& K, const int32_t* hdrop, const int32_t* h, const int32_t* status,
                     const uint32_t* rel, int32_t* out_h, int32_t* out_status, uint32_t* out_rel, hipStream_t st);
// every entry that holds a note into a fresh pool and table
void launch_echo_rebuild(const EchoLedger& from, const EchoLedger& to, uint32_t used, hipStream_t st);

}  // namespace kwok
