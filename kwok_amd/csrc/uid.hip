// uid.hip - the pod uid directory (kwok_watch.h): metadata.uid ->
// pod handle on the device, and the run cuts of a by-uid framed batch.
//
// Per pod slot: its uid (pod_uid[slot], pod_uid_len[slot]; 0: none known).  The
// table is a hint: 64-bit entries (tag << 32) | (handle + 1), 0 empty, at the low
// bits of FNV-1a-64 over the uid bytes, linear probing.  A probe accepts an entry
// only when the tag matches, the handle's slot is PS_USED and the slot's uid equals
// the key byte for byte: a freed slot fails the check, so deletions need no hook,
// and stale entries are never reused (the host rebuilds the table).
//
//   k_uid_resolve   one thread per record of the range [lo, n): the frame's uid span
//                   -> class (hit / new / not sent / domain / invalid), the handle
//                   and the decode's inputs (span, op, handle) on the device; a record
//                   that must not reach the apply gets a span outside the stream
//   k_uid_claim     every new (non-DELETED, unknown) uid claims itself in the call's
//                   scratch table with atomicMin of its record index
//   k_uid_cut       every unknown uid claimed by a smaller index: atomicMin(first_cut)
//   k_uid_note      behind the apply pass of every pod batch: a create's slot takes its
//                   uid (and a table entry), or no uid (an entry that carries none)
//   k_uid_fix       the final results of a run, the withheld records answered
//   k_uid_bind / k_uid_lookup / k_uid_rebuild
//
// Every probe loop is bounded by the table's capacity (a full wrap sets the error
// word); no block waits on another; a kernel that inserts never probes for equality:
// inserts become visible at kernel boundaries on the engine stream.
#include <hip/hip_runtime.h>

#include "../../include/kwok_engine.h"
#include "../../include/kwok_watch.h"
#include "device.h"
#include "kernels.h"

namespace kwok {
namespace {

__device__ __forceinline__ uint32_t lane() { return threadIdx.x & 63u; }
__device__ __forceinline__ void wave_add(bool c, unsigned long long* ctr) {
    const uint64_t m = __ballot(c);
    if (lane() == 0 && m) atomicAdd(ctr, (unsigned long long)__popcll(m));
}
__device__ __forceinline__ uint64_t fnv1a64(const uint8_t* p, uint32_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint32_t k = 0; k < n; k++) h = (h ^ p[k]) * 0x100000001b3ull;
    return h;
}
__device__ __forceinline__ bool bytes_eq(const uint8_t* a, const uint8_t* b, uint32_t n) {
    for (uint32_t k = 0; k < n; k++)
        if (a[k] != b[k]) return false;
    return true;
}
// pod handle -> local slot of an owned bucket (the inverse of pod_handle_of), or false
__device__ __forceinline__ bool pod_slot_of(const DevState& S, int32_t h, size_t* slot) {
    if (h < 0) return false;
    const uint32_t b = (uint32_t)h / S.pod_stride, idx = (uint32_t)h - b * S.pod_stride;
    if (b < S.b_lo || b >= S.b_lo + S.nb || idx >= S.cp) return false;
    *slot = (size_t)(b - S.b_lo) * S.cp + idx;
    return true;
}
// the live pod bound to the key, or -1
__device__ int32_t uid_find(const DevState& S, const UidDir& D, const uint8_t* key, uint32_t len, uint64_t hash) {
    const uint32_t tag = (uint32_t)(hash >> 32);
    uint32_t p = (uint32_t)hash & D.mask;
    for (uint32_t k = 0; k <= D.mask; k++, p = (p + 1) & D.mask) {
        const unsigned long long en = D.tab[p];
        if (!en) return -1;
        if ((uint32_t)(en >> 32) != tag) continue;
        const int32_t h = (int32_t)((uint32_t)en - 1u);
        size_t slot;
        if (!pod_slot_of(S, h, &slot) || !(S.pod_state[slot] & PS_USED) || D.pod_uid_len[slot] != len) continue;
        if (bytes_eq(D.pod_uid + slot * KWOK_UID_MAX, key, len)) return h;
    }
    atomicOr(&D.ctr->err, 1u);  // a full wrap: the table holds no empty entry
    return -1;
}
__device__ void uid_insert(const UidDir& D, uint64_t hash, int32_t h) {
    const unsigned long long en = ((unsigned long long)(hash >> 32) << 32) | (uint32_t)(h + 1);
    uint32_t p = (uint32_t)hash & D.mask;
    for (uint32_t k = 0; k <= D.mask; k++, p = (p + 1) & D.mask)
        if (D.tab[p] == 0 && atomicCAS(&D.tab[p], 0ull, en) == 0ull) return;
    atomicOr(&D.ctr->err, 1u);
}
__device__ __forceinline__ void uid_store(const UidDir& D, size_t slot, const uint8_t* key, uint32_t len) {
    uint8_t* dst = D.pod_uid + slot * KWOK_UID_MAX;
    for (uint32_t k = 0; k < len; k++) dst[k] = key[k];
    D.pod_uid_len[slot] = (uint8_t)len;
}

__global__ __launch_bounds__(256) void k_uid_resolve(DevState S, UidDir D, UidBatch B) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;  // run-local
    const uint32_t i = B.lo + r;
    bool keyed = false, hit = false, sent = false;
    if (i < B.n) {
        const uint32_t fi = B.frame_idx[i];
        uint8_t cls = UID_INVALID, op = KWOK_OP_UPSERT, ulen = 0;
        uint64_t off = ~0ull, hash = 0;
        uint32_t len = 0, uoff = 0;
        int32_t h = -1;
        if (fi < B.n_frames) {
            const kwok_watch_frame f = B.frames[fi];
            const bool ok = f.status == KWOK_OK &&
                            (f.type == KWOK_WATCH_ADDED || f.type == KWOK_WATCH_MODIFIED || f.type == KWOK_WATCH_DELETED);
            if (ok) {
                const bool del = f.type == KWOK_WATCH_DELETED;
                if ((f.flags & KWOK_FRAME_ESC_UID) || !f.uid.len || f.uid.len > KWOK_UID_MAX ||
                    (uint64_t)f.uid.off + f.uid.len > B.stream_len) {
                    cls = UID_DOMAIN;
                } else {
                    keyed = true;
                    uoff = f.uid.off, ulen = (uint8_t)f.uid.len;
                    hash = fnv1a64(B.stream + uoff, ulen);
                    h = uid_find(S, D, B.stream + uoff, ulen, hash);
                    hit = h >= 0;
                    cls = hit ? UID_HIT : del ? UID_NOT_SENT : UID_NEW;
                    if (cls != UID_NOT_SENT) off = f.doc_off, len = f.doc_len, op = del ? KWOK_OP_DELETE : KWOK_OP_UPSERT;
                }
            }
        }
        sent = cls == UID_HIT || cls == UID_NEW;
        B.cls[i] = cls;
        B.uoff[i] = uoff;
        B.ulen[i] = ulen;
        B.hash[i] = hash;
        B.doc_off[r] = off;
        B.doc_len[r] = len;
        B.op[r] = op;
        B.handle[r] = h;
    }
    wave_add(keyed, &D.ctr->lookups);
    wave_add(hit, &D.ctr->hits);
    const uint64_t m = __ballot(sent), mn = __ballot(sent && !hit);
    if (lane() == 0 && m) atomicAdd(&B.run->n_sent, (uint32_t)__popcll(m));
    if (lane() == 0 && mn) atomicAdd(&B.run->n_new, (uint32_t)__popcll(mn));
}

// the scratch table holds record indices (~0: empty); an entry's uid is its record's span of the stream
__global__ __launch_bounds__(256) void k_uid_claim(UidBatch B) {
    const uint32_t i = B.lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.n || B.cls[i] != UID_NEW) return;
    const uint32_t len = B.ulen[i];
    const uint8_t* key = B.stream + B.uoff[i];
    uint32_t p = (uint32_t)B.hash[i] & B.claim_mask;
    for (uint32_t k = 0; k <= B.claim_mask; k++, p = (p + 1) & B.claim_mask) {
        uint32_t cur = B.claim[p];
        if (cur == ~0u) {
            cur = atomicCAS(&B.claim[p], ~0u, i);
            if (cur == ~0u) return;
        }
        // (cur: a record of the range; atomicMin only ever replaces it by a record of the same uid)
        if (cur < B.n && B.ulen[cur] == len && bytes_eq(B.stream + B.uoff[cur], key, len)) {
            atomicMin(&B.claim[p], i);
            return;
        }
    }
    atomicOr(B.err, 1u);
}
__global__ __launch_bounds__(256) void k_uid_cut(UidBatch B) {
    const uint32_t i = B.lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.n) return;
    const uint8_t cls = B.cls[i];
    if (cls != UID_NEW && cls != UID_NOT_SENT) return;
    const uint32_t len = B.ulen[i];
    const uint8_t* key = B.stream + B.uoff[i];
    uint32_t p = (uint32_t)B.hash[i] & B.claim_mask;
    for (uint32_t k = 0; k <= B.claim_mask; k++, p = (p + 1) & B.claim_mask) {
        const uint32_t cur = B.claim[p];
        if (cur == ~0u) return;
        if (cur < B.n && B.ulen[cur] == len && bytes_eq(B.stream + B.uoff[cur], key, len)) {
            if (cur < i) atomicMin(&B.run->first_cut, i);
            return;
        }
    }
    atomicOr(B.err, 1u);
}

__global__ __launch_bounds__(256) void k_uid_note(DevState S, IngestBatch I, UidDir D, UidNote N) {
    // a speculative apply pass that returned for growth wrote no result: the redo notes
    if (I.spec && (I.sum->need > S.cp || *I.abort)) return;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool bound = false, unbound = false;
    if (i < I.n) {
        const PodRec r = I.rec[i];
        size_t slot = 0;
        const bool create = r.op == KWOK_OP_UPSERT && !(r.chk & REC_EXISTING) && I.out_status[i] == KWOK_OK &&
                            pod_slot_of(S, I.out_handle[i], &slot);
        if (create) {
            if (N.cls && N.cls[i] == UID_NEW) {
                uid_store(D, slot, N.stream + N.uoff[i], N.ulen[i]);
                uid_insert(D, N.hash[i], I.out_handle[i]);
                bound = true;
            } else {
                D.pod_uid_len[slot] = 0;  // (a reused slot would keep its previous pod's uid)
                unbound = true;
            }
        }
    }
    wave_add(bound, &D.ctr->binds);
    wave_add(bound, &D.ctr->entries);
    wave_add(unbound, &D.ctr->unbound);
}

__global__ __launch_bounds__(256) void k_uid_fix(UidBatch B, uint32_t m, const int32_t* h, const int32_t* st, const uint32_t* rel,
                                                 int32_t* out_h, int32_t* out_st, uint32_t* out_rel) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    const uint32_t i = B.lo + r;
    const uint8_t cls = B.cls[i];
    const bool held = cls == UID_NOT_SENT || cls == UID_DOMAIN || cls == UID_INVALID;
    out_h[i] = held ? -1 : h[r];
    out_st[i] = cls == UID_NOT_SENT ? KWOK_NOT_SENT : cls == UID_DOMAIN ? KWOK_EDOMAIN : cls == UID_INVALID ? KWOK_EINVAL : st[r];
    out_rel[i] = held ? 0u : rel[r];
}

__global__ __launch_bounds__(256) void k_uid_bind(DevState S, UidDir D, const int32_t* handles, const uint8_t* arena,
                                                  uint64_t arena_len, const uint64_t* off, const uint32_t* len, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    if (i < n) {
        size_t slot = 0;
        const uint32_t l = len[i];
        ok = l && l <= KWOK_UID_MAX && off[i] <= arena_len && off[i] + l <= arena_len && pod_slot_of(S, handles[i], &slot) &&
             (S.pod_state[slot] & PS_USED);
        if (ok) {
            const uint8_t* key = arena + off[i];
            uid_store(D, slot, key, l);
            uid_insert(D, fnv1a64(key, l), handles[i]);
        }
    }
    wave_add(ok, &D.ctr->binds);
    wave_add(ok, &D.ctr->entries);
    wave_add(i < n && !ok, &D.ctr->bad);
}
__global__ __launch_bounds__(256) void k_uid_lookup(DevState S, UidDir D, const uint8_t* arena, uint64_t arena_len,
                                                    const uint64_t* off, const uint32_t* len, uint32_t n, int32_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool keyed = false, hit = false;
    if (i < n) {
        const uint32_t l = len[i];
        int32_t h = -1;
        keyed = l && l <= KWOK_UID_MAX && off[i] <= arena_len && off[i] + l <= arena_len;
        if (keyed) h = uid_find(S, D, arena + off[i], l, fnv1a64(arena + off[i], l));
        hit = h >= 0;
        out[i] = h;
    }
    wave_add(keyed, &D.ctr->lookups);
    wave_add(hit, &D.ctr->hits);
}
// one thread per pod slot below its bucket's fill mark: every live slot with a uid back into the cleared table
__global__ __launch_bounds__(256) void k_uid_rebuild(DevState S, UidDir D) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    bool live = false;
    if (g < S.n_pod_slots) {
        const uint32_t b = g / S.cp, s = g - b * S.cp;
        const uint32_t l = D.pod_uid_len[g];
        live = s < S.pod_fill[b] && (S.pod_state[g] & PS_USED) && l && l <= KWOK_UID_MAX;
        if (live) uid_insert(D, fnv1a64(D.pod_uid + (size_t)g * KWOK_UID_MAX, l), pod_handle_of(S, g));
    }
    wave_add(live, &D.ctr->entries);
}

inline uint32_t cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

}  // namespace

void launch_uid_resolve(const DevState& S, const UidDir& D, const UidBatch& B, hipStream_t st) {
    if (B.n > B.lo) hipLaunchKernelGGL(k_uid_resolve, dim3(cdiv(B.n - B.lo, 256)), dim3(256), 0, st, S, D, B);
}
void launch_uid_cut(const UidBatch& B, hipStream_t st) {
    if (B.n <= B.lo) return;
    hipLaunchKernelGGL(k_uid_claim, dim3(cdiv(B.n - B.lo, 256)), dim3(256), 0, st, B);
    hipLaunchKernelGGL(k_uid_cut, dim3(cdiv(B.n - B.lo, 256)), dim3(256), 0, st, B);
}
void launch_uid_note(const DevState& S, const IngestBatch& I, const UidDir& D, const UidNote& N, hipStream_t st) {
    if (I.n) hipLaunchKernelGGL(k_uid_note, dim3(cdiv(I.n, 256)), dim3(256), 0, st, S, I, D, N);
}
void launch_uid_fix(const UidBatch& B, uint32_t m, const int32_t* h, const int32_t* status, const uint32_t* rel, int32_t* out_h,
                    int32_t* out_status, uint32_t* out_rel, hipStream_t st) {
    if (m) hipLaunchKernelGGL(k_uid_fix, dim3(cdiv(m, 256)), dim3(256), 0, st, B, m, h, status, rel, out_h, out_status, out_rel);
}
void launch_uid_bind(const DevState& S, const UidDir& D, const int32_t* handles, const uint8_t* arena, uint64_t arena_len,
                     const uint64_t* off, const uint32_t* len, uint32_t n, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_uid_bind, dim3(cdiv(n, 256)), dim3(256), 0, st, S, D, handles, arena, arena_len, off, len, n);
}
void launch_uid_lookup(const DevState& S, const UidDir& D, const uint8_t* arena, uint64_t arena_len, const uint64_t* off,
                       const uint32_t* len, uint32_t n, int32_t* out, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_uid_lookup, dim3(cdiv(n, 256)), dim3(256), 0, st, S, D, arena, arena_len, off, len, n, out);
}
void launch_uid_rebuild(const DevState& S, const UidDir& D, hipStream_t st) {
    if (S.n_pod_slots) hipLaunchKernelGGL(k_uid_rebuild, dim3(cdiv(S.n_pod_slots, 256)), dim3(256), 0, st, S, D);
}

}  // namespace kwok
