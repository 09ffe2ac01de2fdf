// echo.hip - the echo ledger (kwok_watch.h): the resourceVersions the
// engine's own patches returned, per uid, kept in HBM; framed batches and typed events
// are filtered against it on the device under the rule of controller.Echoes.
//
// The ledger is a pool of 256-byte entries (one per noted uid) behind an open-addressing
// table of pool indices at the low bits of FNV-1a-64 over the uid bytes.  A probe accepts
// an entry only after comparing the stored uid bytes.  An emptied entry stays its uid's
// (a rebuild compacts them away).
//
// A call's records are grouped by uid so that ONE thread owns one uid's records, in
// record order - the rule is sequential per uid and independent between uids:
//   k_echo_key_*    one thread per record: the record's class, uid / rv spans and hash
//   k_echo_claim    every keyed record claims its uid in the call's scratch table with
//                   atomicMin of its record index (k_uid_claim's scheme)
//   k_echo_group    every keyed record reads its uid's first record (its owner); a repeat
//                   counts itself there.  A call without repeats ends the grouping here:
//   k_echo_alloc    (repeats only) an owner takes room for its repeats in list[]
//   k_echo_scatter  (repeats only) a repeat writes its index there; the owner sorts the list
//                   (heap sort: n log n, a batch of one uid is not quadratic)
//   k_echo_need     an update's room, counted before anything is stored (the host grows or refuses)
//   k_echo_apply / k_echo_insert   notes and forgets: first the uids the ledger holds, then
//                   (next launch) the uids that need a new entry - a launch that inserts
//                   never probes for equality, and one thread owns a uid: no two insert it
//   k_echo_decide   the filter; it mutates entries, it never inserts
//   k_echo_count / k_echo_scan / k_echo_keep   the kept records' frame indices, in order
//   k_echo_node_handles, k_echo_fix, k_echo_rebuild
//
// Every probe loop is bounded by the capacity (a full wrap sets the error word); no
// block waits on another.
#include <hip/hip_runtime.h>

#include "../../include/kwok_engine.h"
#include "../../include/kwok_watch.h"
#include "device.h"
#include "echo.h"
#include "kernels.h"

namespace kwok {
namespace {

__device__ __forceinline__ uint32_t lane() { return threadIdx.x & 63u; }
// the wave's sum of v onto *ctr (every lane of the wave calls it)
__device__ __forceinline__ void wave_sum(uint32_t v, unsigned long long* ctr) {
    for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    if (lane() == 0 && v) atomicAdd(ctr, (unsigned long long)v);
}
__device__ __forceinline__ void wave_sum32(uint32_t v, uint32_t* ctr) {
    for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    if (lane() == 0 && v) atomicAdd(ctr, v);
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
__device__ __forceinline__ bool span_ok(uint64_t off, uint32_t len, uint64_t total) { return off <= total && off + len <= total; }

// ---- the ledger ----
// the uid's pool entry, or null
__device__ EchoEntry* echo_find(const EchoLedger& L, const uint8_t* key, uint32_t len, uint64_t hash) {
    uint32_t p = (uint32_t)hash & L.mask;
    for (uint32_t k = 0; k <= L.mask; k++, p = (p + 1) & L.mask) {
        const uint32_t en = L.tab[p];
        if (!en) return nullptr;
        if (en > L.pool_cap) break;
        EchoEntry* x = L.pool + (en - 1);
        if (x->hash == hash && x->ulen == len && bytes_eq(x->uid, key, len)) return x;
    }
    atomicOr(&L.ctr->err, 1u);  // a full wrap: the table holds no empty entry
    return nullptr;
}
// pool entry idx into the table (no probe for equality: the uid is not in it)
__device__ void echo_link(const EchoLedger& L, uint64_t hash, uint32_t idx) {
    uint32_t p = (uint32_t)hash & L.mask;
    for (uint32_t k = 0; k <= L.mask; k++, p = (p + 1) & L.mask)
        if (L.tab[p] == 0 && atomicCAS(&L.tab[p], 0u, idx + 1) == 0u) return;
    atomicOr(&L.ctr->err, 1u);
}
__device__ __forceinline__ void entry_shift(EchoEntry* x, uint32_t at) {  // the list without its element `at`
    for (uint32_t k = at; k + 1 < x->cnt; k++) {
        x->rlen[k] = x->rlen[k + 1];
        for (uint32_t b = 0; b < KWOK_RV_MAX; b++) x->rv[k][b] = x->rv[k + 1][b];
    }
    x->cnt--;
}
// true: the ninth note dropped the oldest
__device__ bool entry_note(EchoEntry* x, const uint8_t* rv, uint32_t len) {
    bool ev = false;
    if (x->cnt >= KWOK_ECHO_KEEP) {
        entry_shift(x, 0);
        ev = true;
    }
    const uint32_t k = x->cnt;
    for (uint32_t b = 0; b < KWOK_RV_MAX; b++) x->rv[k][b] = b < len ? rv[b] : 0;
    x->rlen[k] = (uint8_t)len;
    x->cnt = (uint8_t)(k + 1);
    return ev;
}
// is_echo: the first occurrence of rv is removed
__device__ bool entry_take(EchoEntry* x, const uint8_t* rv, uint32_t len) {
    const uint32_t c = x->cnt <= KWOK_ECHO_KEEP ? x->cnt : KWOK_ECHO_KEEP;
    for (uint32_t k = 0; k < c; k++)
        if (x->rlen[k] == len && bytes_eq(x->rv[k], rv, len)) {
            entry_shift(x, k);
            return true;
        }
    return false;
}

// ---- the front ends ----
__device__ __forceinline__ void key_store(const EchoBatch& B, uint32_t i, uint8_t kind, uint32_t uoff, uint32_t ulen, uint32_t roff,
                                          uint32_t rlen) {
    B.kind[i] = kind;
    B.uoff[i] = uoff, B.ulen[i] = (uint8_t)ulen, B.roff[i] = roff, B.rlen[i] = (uint8_t)rlen;
    B.hash[i] = kind != EK_SKIP ? fnv1a64(B.base + uoff, ulen) : 0;
    B.own[i] = ~0u;
}
__global__ __launch_bounds__(256) void k_echo_key_update(EchoBatch B, EchoSpans P, int32_t* status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < B.n) {
        const uint8_t op = P.op[i];
        const uint32_t ul = P.uid_len[i], rl = op == KWOK_ECHO_NOTE ? P.rv_len[i] : 0;
        int32_t s = KWOK_OK;
        uint8_t kind = EK_SKIP;
        if (op != KWOK_ECHO_NOTE && op != KWOK_ECHO_FORGET) s = KWOK_EINVAL;
        else if (ul > KWOK_UID_MAX || rl > KWOK_RV_MAX) s = KWOK_EDOMAIN;
        else if (!ul || (op == KWOK_ECHO_NOTE && !rl)) s = KWOK_OK;  // ignored
        else if (!span_ok(P.uid_off[i], ul, B.base_len) || (rl && !span_ok(P.rv_off[i], rl, B.base_len))) s = KWOK_EINVAL;
        else kind = op == KWOK_ECHO_NOTE ? EK_NOTE : EK_FORGET;
        key_store(B, i, kind, kind ? (uint32_t)P.uid_off[i] : 0, kind ? ul : 0, kind == EK_NOTE ? (uint32_t)P.rv_off[i] : 0,
                  kind == EK_NOTE ? rl : 0);
        B.res[i] = 0;
        status[i] = s;
        bad = s != KWOK_OK;
    }
    wave_sum32(bad, &B.call->n_bad);
}
__global__ __launch_bounds__(256) void k_echo_key_typed(EchoBatch B, EchoSpans P) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.n) return;
    const uint32_t ul = P.uid_len[i];
    uint32_t rl = P.rv_len[i];
    const bool keyed = ul && ul <= KWOK_UID_MAX && span_ok(P.uid_off[i], ul, B.base_len);
    if (!rl || rl > KWOK_RV_MAX || !span_ok(P.rv_off[i], rl, B.base_len)) rl = 0;
    const uint8_t kind = !keyed ? EK_SKIP : P.op[i] ? EK_DELETE : EK_UPSERT;
    key_store(B, i, kind, keyed ? (uint32_t)P.uid_off[i] : 0, keyed ? ul : 0, keyed && rl ? (uint32_t)P.rv_off[i] : 0, keyed ? rl : 0);
    B.res[i] = ER_KEEP;
}
__global__ __launch_bounds__(256) void k_echo_key_frames(EchoBatch B, EchoFrames F) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.n) return;
    const uint32_t fi = F.frame_idx[i];
    uint8_t res = ER_EINVAL, kind = EK_SKIP;
    uint32_t uoff = 0, ulen = 0, roff = 0, rlen = 0;
    if (fi < F.n_frames) {
        const kwok_watch_frame f = F.frames[fi];
        if (f.status == KWOK_OK && (f.type == KWOK_WATCH_ADDED || f.type == KWOK_WATCH_MODIFIED || f.type == KWOK_WATCH_DELETED)) {
            if (f.flags & (KWOK_FRAME_ESC_UID | KWOK_FRAME_ESC_RV)) {
                res = ER_EDOMAIN;
            } else {
                res = ER_KEEP;
                if (f.uid.len && f.uid.len <= KWOK_UID_MAX && span_ok(f.uid.off, f.uid.len, B.base_len)) {
                    kind = f.type == KWOK_WATCH_DELETED ? EK_DELETE : EK_UPSERT;
                    uoff = f.uid.off, ulen = f.uid.len;
                    const kwok_str r = f.resource_version;
                    if (r.len && r.len <= KWOK_RV_MAX && span_ok(r.off, r.len, B.base_len)) roff = r.off, rlen = r.len;
                }
            }
        }
    }
    key_store(B, i, kind, uoff, ulen, roff, rlen);
    B.res[i] = res;
}
// k_echo_key_frames for notes (kwok_echo_note_framed): every ingestible frame is a note of its (uid, rv),
// under k_echo_key_update's rules for a KWOK_ECHO_NOTE with the same pair
__global__ __launch_bounds__(256) void k_echo_key_note_frames(EchoBatch B, EchoFrames F, int32_t* status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false, note = false;
    if (i < B.n) {
        const uint32_t fi = F.frame_idx[i];
        int32_t s = KWOK_EINVAL;
        uint8_t kind = EK_SKIP;
        uint32_t uoff = 0, ulen = 0, roff = 0, rlen = 0;
        if (fi < F.n_frames) {
            const kwok_watch_frame f = F.frames[fi];
            if (f.status == KWOK_OK && (f.type == KWOK_WATCH_ADDED || f.type == KWOK_WATCH_MODIFIED || f.type == KWOK_WATCH_DELETED)) {
                const kwok_str u = f.uid, r = f.resource_version;
                if ((f.flags & (KWOK_FRAME_ESC_UID | KWOK_FRAME_ESC_RV)) || u.len > KWOK_UID_MAX || r.len > KWOK_RV_MAX) {
                    s = KWOK_EDOMAIN;
                } else if (!u.len || !r.len) {
                    s = KWOK_OK;  // ignored
                } else if (span_ok(u.off, u.len, B.base_len) && span_ok(r.off, r.len, B.base_len)) {
                    s = KWOK_OK;
                    kind = EK_NOTE;
                    uoff = u.off, ulen = u.len, roff = r.off, rlen = r.len;
                }
            }
        }
        key_store(B, i, kind, uoff, ulen, roff, rlen);
        B.res[i] = 0;
        status[i] = s;
        bad = s != KWOK_OK;
        note = kind == EK_NOTE;
    }
    wave_sum32(bad, &B.call->n_bad);
    wave_sum32(note, &B.call->n_note);
}

// ---- grouping by uid ----
__device__ __forceinline__ bool same_uid(const EchoBatch& B, uint32_t a, const uint8_t* key, uint32_t len) {
    return a < B.n && B.ulen[a] == len && bytes_eq(B.base + B.uoff[a], key, len);
}
__global__ __launch_bounds__(256) void k_echo_claim(EchoBatch B) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.n || B.kind[i] == EK_SKIP) return;
    const uint32_t len = B.ulen[i];
    const uint8_t* key = B.base + B.uoff[i];
    uint32_t p = (uint32_t)B.hash[i] & B.claim_mask;
    for (uint32_t k = 0; k <= B.claim_mask; k++, p = (p + 1) & B.claim_mask) {
        uint32_t cur = B.claim[p];
        if (cur == ~0u) {
            cur = atomicCAS(&B.claim[p], ~0u, i);
            if (cur == ~0u) return;
        }
        // (cur: a record of the call; atomicMin only ever replaces it by a record of the same uid)
        if (same_uid(B, cur, key, len)) {
            atomicMin(&B.claim[p], i);
            return;
        }
    }
    atomicOr(&B.call->err, 1u);
}
__global__ __launch_bounds__(256) void k_echo_group(EchoBatch B) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool rep = false;
    if (i < B.n && B.kind[i] != EK_SKIP) {
        const uint32_t len = B.ulen[i];
        const uint8_t* key = B.base + B.uoff[i];
        uint32_t p = (uint32_t)B.hash[i] & B.claim_mask, own = ~0u;
        for (uint32_t k = 0; k <= B.claim_mask; k++, p = (p + 1) & B.claim_mask) {
            const uint32_t cur = B.claim[p];
            if (cur == ~0u) break;
            if (same_uid(B, cur, key, len)) {
                own = cur;
                break;
            }
        }
        if (own == ~0u) atomicOr(&B.call->err, 1u);  // (every keyed record claimed its uid)
        else {
            B.own[i] = own;
            rep = own != i;
            if (rep) atomicAdd(&B.cnt[own], 1u);
        }
    }
    wave_sum32(rep, &B.call->n_rep);
}
__global__ __launch_bounds__(256) void k_echo_alloc(EchoBatch B) {
    if (!B.call->n_rep) return;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.n || B.own[i] != i || !B.cnt[i]) return;
    B.lbase[i] = atomicAdd(&B.call->list_used, B.cnt[i]);
}
__global__ __launch_bounds__(256) void k_echo_scatter(EchoBatch B) {
    if (!B.call->n_rep) return;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.n) return;
    const uint32_t own = B.own[i];
    if (own == ~0u || own == i || own >= B.n) return;
    const uint32_t at = B.lbase[own] + atomicAdd(&B.fill[own], 1u);
    if (at < B.n) B.list[at] = i;
    else atomicOr(&B.call->err, 1u);
}
// ascending, in place (one thread)
__device__ void sift(uint32_t* a, uint32_t s, uint32_t e) {
    const uint32_t v = a[s];
    for (;;) {
        uint32_t c = 2 * s + 1;
        if (c >= e) break;
        if (c + 1 < e && a[c + 1] > a[c]) c++;
        if (a[c] <= v) break;
        a[s] = a[c];
        s = c;
    }
    a[s] = v;
}
__device__ void heap_sort(uint32_t* a, uint32_t n) {
    for (uint32_t s = n / 2; s-- > 0;) sift(a, s, n);
    for (uint32_t e = n - 1; e > 0; e--) {
        const uint32_t t = a[0];
        a[0] = a[e];
        a[e] = t;
        sift(a, 0, e);
    }
}
// the owner's records in record order: itself, then its sorted repeats
struct Group {
    uint32_t self, n;
    const uint32_t* rep;
    __device__ uint32_t at(uint32_t j) const { return j ? rep[j - 1] : self; }
};
__device__ bool group_of(const EchoBatch& B, uint32_t i, Group* g) {
    if (i >= B.n || B.kind[i] == EK_SKIP || B.own[i] != i) return false;
    uint32_t c = B.cnt[i];
    g->self = i, g->n = 1, g->rep = nullptr;
    if (c) {
        const uint32_t lb = B.lbase[i];
        if ((uint64_t)lb + c > B.n) {
            atomicOr(&B.call->err, 1u);
            return false;
        }
        if (c > 1) heap_sort(B.list + lb, c);
        g->rep = B.list + lb, g->n = 1 + c;
    }
    return true;
}

// ---- notes and forgets ----
struct Tally {
    uint32_t notes, forgets, evictions;
    int32_t live;
};
__device__ void run_ops(const EchoBatch& B, const Group& g, EchoEntry* x, Tally* t) {
    const bool was = x->cnt > 0;
    for (uint32_t j = 0; j < g.n; j++) {
        const uint32_t r = g.at(j);
        if (B.kind[r] == EK_NOTE) {
            t->evictions += entry_note(x, B.base + B.roff[r], B.rlen[r]);
            t->notes++;
        } else if (B.kind[r] == EK_FORGET) {
            t->forgets += x->cnt > 0;
            x->cnt = 0;
        }
    }
    t->live += (int32_t)(x->cnt > 0) - (int32_t)was;
}
__device__ __forceinline__ void tally_out(const EchoLedger& L, const Tally& t) {
    wave_sum(t.notes, &L.ctr->notes);
    wave_sum(t.forgets, &L.ctr->forgets);
    wave_sum(t.evictions, &L.ctr->evictions);
    wave_sum(t.live > 0 ? (uint32_t)t.live : 0u, &L.ctr->live);
    uint32_t down = t.live < 0 ? (uint32_t)-t.live : 0u;
    for (int o = 32; o; o >>= 1) down += (uint32_t)__shfl_xor((int)down, o);
    if (lane() == 0 && down) atomicAdd(&L.ctr->live, 0ull - (unsigned long long)down);
}
// before anything is stored: the uids the call notes that have no entry holding a note (the room the call needs)
__global__ __launch_bounds__(256) void k_echo_need(EchoLedger L, EchoBatch B) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool need = false;
    Group g;
    if (group_of(B, i, &g)) {
        for (uint32_t j = 0; j < g.n && !need; j++) need = B.kind[g.at(j)] == EK_NOTE;
        if (need) {
            const EchoEntry* x = echo_find(L, B.base + B.uoff[i], B.ulen[i], B.hash[i]);
            need = !x || !x->cnt;
        }
    }
    wave_sum32(need, &B.call->n_new);
}
__global__ __launch_bounds__(256) void k_echo_apply(EchoLedger L, EchoBatch B) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    Tally t{};
    Group g;
    if (group_of(B, i, &g)) {
        EchoEntry* x = echo_find(L, B.base + B.uoff[i], B.ulen[i], B.hash[i]);
        if (x) run_ops(B, g, x, &t);
        else {  // (forgets of a uid the ledger does not hold do nothing)
            bool note = false;
            for (uint32_t j = 0; j < g.n && !note; j++) note = B.kind[g.at(j)] == EK_NOTE;
            B.res[i] = note;
        }
    }
    tally_out(L, t);
}
__global__ __launch_bounds__(256) void k_echo_insert(EchoLedger L, EchoBatch B) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    Tally t{};
    if (i < B.n && B.kind[i] != EK_SKIP && B.own[i] == i && B.res[i]) {
        Group g{i, 1 + B.cnt[i], B.cnt[i] ? B.list + B.lbase[i] : nullptr};  // (k_echo_apply checked and sorted the list)
        const uint32_t idx = atomicAdd(&L.ctr->used, 1u);
        if (idx >= L.pool_cap) atomicOr(&L.ctr->err, 2u);
        else {
            EchoEntry* x = L.pool + idx;  // (a fresh pool entry is zero: no note)
            const uint32_t len = B.ulen[i];
            x->hash = B.hash[i];
            for (uint32_t k = 0; k < len; k++) x->uid[k] = B.base[B.uoff[i] + k];
            x->ulen = (uint8_t)len;
            x->cnt = 0;
            run_ops(B, g, x, &t);
            echo_link(L, B.hash[i], idx);
        }
    }
    tally_out(L, t);
}

// ---- the filter ----
__global__ __launch_bounds__(256) void k_echo_decide(EchoLedger L, EchoBatch B) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t matched = 0, dropped = 0, forgets = 0, down = 0;
    Group g;
    if (group_of(B, i, &g)) {
        EchoEntry* x = echo_find(L, B.base + B.uoff[i], B.ulen[i], B.hash[i]);
        if (x && x->cnt) {
            bool seen = false;
            for (uint32_t j = 0; j < g.n && x->cnt; j++) {
                const uint32_t r = g.at(j);
                if (B.kind[r] == EK_DELETE) {
                    forgets++;
                    x->cnt = 0;
                    seen = true;
                    continue;
                }
                const bool m = B.rlen[r] && entry_take(x, B.base + B.roff[r], B.rlen[r]);
                matched += m;
                if (m && !seen) {
                    B.res[r] = ER_DROP;
                    dropped++;
                } else {
                    seen = true;
                }
            }
            down = x->cnt == 0;
        }
    }
    wave_sum(matched, &L.ctr->matched);
    wave_sum(dropped, &L.ctr->dropped);
    wave_sum(matched - dropped, &L.ctr->kept_matched);
    wave_sum(forgets, &L.ctr->forgets);
    wave_sum32(dropped, &B.call->n_drop);
    for (int o = 32; o; o >>= 1) down += (uint32_t)__shfl_xor((int)down, o);
    if (lane() == 0 && down) atomicAdd(&L.ctr->live, 0ull - (unsigned long long)down);
}

// ---- the kept records, compacted in record order ----
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* total) {  // exclusive, 256 threads
    __shared__ uint32_t ws[4];
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)inc, o);
        if (lane() >= (uint32_t)o) inc += u;
    }
    if (lane() == 63) ws[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) base += ws[w];
    *total = ws[0] + ws[1] + ws[2] + ws[3];
    __syncthreads();
    return base + inc - v;
}
__global__ __launch_bounds__(256) void k_echo_count(EchoBatch B, EchoKeep K) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t total;
    (void)block_scan(i < B.n && B.res[i] == ER_KEEP, &total);
    if (threadIdx.x == 0) K.bsum[blockIdx.x] = total;
}
// one block: bsum[0 .. nb) -> exclusive prefix in place, the total to bsum[nb] and n_keep
__global__ __launch_bounds__(256) void k_echo_scan(EchoBatch B, EchoKeep K, uint32_t nb) {
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += 256) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < nb ? K.bsum[b] : 0;
        uint32_t total;
        const uint32_t ex = block_scan(v, &total);
        if (b < nb) K.bsum[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) K.bsum[nb] = carry, B.call->n_keep = carry;
}
__global__ __launch_bounds__(256) void k_echo_keep(EchoBatch B, EchoFrames F, EchoKeep K) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const bool in = i < B.n;
    const uint8_t res = in ? B.res[i] : (uint8_t)ER_EINVAL;
    uint32_t total;
    const uint32_t pos = K.bsum[blockIdx.x] + block_scan(res == ER_KEEP, &total);
    if (!in) return;
    K.kpos[i] = pos;
    if (res == ER_KEEP && pos < B.n) K.kidx[pos] = F.frame_idx[i];
    K.q_off[i] = B.uoff[i];
    K.q_len[i] = res == ER_DROP ? B.ulen[i] : 0u;
}

// a dropped node frame's handle: the existing node its name resolves to (one thread per record)
__global__ __launch_bounds__(256) void k_echo_node_handles(DevState S, EchoBatch B, EchoFrames F, int32_t* hdrop) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.n) return;
    int32_t h = -1;
    const uint32_t fi = F.frame_idx[i];
    if (B.res[i] == ER_DROP && fi < F.n_frames) {
        const kwok_watch_frame f = F.frames[fi];
        const uint32_t len = f.name.len;
        if (!(f.flags & KWOK_FRAME_ESC_NAME) && len && len <= NODE_NAME_MAX && span_ok(f.name.off, len, B.base_len)) {
            const uint8_t* nm = B.base + f.name.off;
            uint32_t hs = 0x811C9DC5u;
            for (uint32_t k = 0; k < len; k++) hs = (hs ^ nm[k]) * 0x01000193u;
            const uint32_t b = hs & (S.buckets - 1);
            if (b >= S.b_lo && b < S.b_lo + S.nb) {
                const uint64_t key = (uint64_t)hs | ((uint64_t)len << 32);
                const size_t nbase = (size_t)(b - S.b_lo) * S.cn;
                for (uint32_t j = 0; j < S.cn && h < 0; j++)
                    if (S.node_key[nbase + j] == key && (S.node_state[nbase + j] & NS_EXISTS) &&
                        bytes_eq(S.node_name + (nbase + j) * NAME_STRIDE, nm, len))
                        h = (int32_t)(b * S.cn + j);
            }
        }
    }
    hdrop[i] = h;
}

__global__ __launch_bounds__(256) void k_echo_fix(EchoBatch B, EchoKeep K, const int32_t* hdrop, const int32_t* h, const int32_t* st,
                                                  const uint32_t* rel, int32_t* out_h, int32_t* out_st, uint32_t* out_rel) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.n) return;
    const uint8_t res = B.res[i];
    const uint32_t p = K.kpos[i];
    const bool kept = res == ER_KEEP && p < B.n;
    out_h[i] = kept ? h[p] : res == ER_DROP ? hdrop[i] : -1;
    out_st[i] = kept ? st[p] : res == ER_DROP ? KWOK_ECHO : res == ER_EDOMAIN ? KWOK_EDOMAIN : KWOK_EINVAL;
    out_rel[i] = kept ? rel[p] : 0u;
}

// one thread per pool entry handed out: the ones that hold a note move to the fresh ledger
__global__ __launch_bounds__(256) void k_echo_rebuild(EchoLedger from, EchoLedger to, uint32_t used) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= used || g >= from.pool_cap) return;
    const EchoEntry* s = from.pool + g;
    if (!s->cnt) return;
    const uint32_t idx = atomicAdd(&to.ctr->used, 1u);
    if (idx >= to.pool_cap) {
        atomicOr(&to.ctr->err, 2u);
        return;
    }
    const uint4* sp = reinterpret_cast<const uint4*>(s);
    uint4* dp = reinterpret_cast<uint4*>(to.pool + idx);
    for (uint32_t k = 0; k < sizeof(EchoEntry) / 16; k++) dp[k] = sp[k];
    echo_link(to, s->hash, idx);
}

inline uint32_t cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

}  // namespace

void launch_echo_key_update(const EchoBatch& B, const EchoSpans& P, int32_t* status, hipStream_t st) {
    if (B.n) hipLaunchKernelGGL(k_echo_key_update, dim3(cdiv(B.n, 256)), dim3(256), 0, st, B, P, status);
}
void launch_echo_key_typed(const EchoBatch& B, const EchoSpans& P, hipStream_t st) {
    if (B.n) hipLaunchKernelGGL(k_echo_key_typed, dim3(cdiv(B.n, 256)), dim3(256), 0, st, B, P);
}
void launch_echo_key_frames(const EchoBatch& B, const EchoFrames& F, hipStream_t st) {
    if (B.n) hipLaunchKernelGGL(k_echo_key_frames, dim3(cdiv(B.n, 256)), dim3(256), 0, st, B, F);
}
void launch_echo_key_note_frames(const EchoBatch& B, const EchoFrames& F, int32_t* status, hipStream_t st) {
    if (B.n) hipLaunchKernelGGL(k_echo_key_note_frames, dim3(cdiv(B.n, 256)), dim3(256), 0, st, B, F, status);
}
void launch_echo_group(const EchoBatch& B, hipStream_t st) {
    if (!B.n) return;
    const dim3 g(cdiv(B.n, 256)), b(256);
    hipLaunchKernelGGL(k_echo_claim, g, b, 0, st, B);
    hipLaunchKernelGGL(k_echo_group, g, b, 0, st, B);
    hipLaunchKernelGGL(k_echo_alloc, g, b, 0, st, B);
    hipLaunchKernelGGL(k_echo_scatter, g, b, 0, st, B);
}
void launch_echo_need(const EchoLedger& L, const EchoBatch& B, hipStream_t st) {
    if (B.n) hipLaunchKernelGGL(k_echo_need, dim3(cdiv(B.n, 256)), dim3(256), 0, st, L, B);
}
void launch_echo_update(const EchoLedger& L, const EchoBatch& B, hipStream_t st) {
    if (!B.n) return;
    hipLaunchKernelGGL(k_echo_apply, dim3(cdiv(B.n, 256)), dim3(256), 0, st, L, B);
    hipLaunchKernelGGL(k_echo_insert, dim3(cdiv(B.n, 256)), dim3(256), 0, st, L, B);
}
void launch_echo_decide(const EchoLedger& L, const EchoBatch& B, hipStream_t st) {
    if (B.n) hipLaunchKernelGGL(k_echo_decide, dim3(cdiv(B.n, 256)), dim3(256), 0, st, L, B);
}
void launch_echo_keep(const EchoBatch& B, const EchoFrames& F, const EchoKeep& K, hipStream_t st) {
    if (!B.n) return;
    const uint32_t nb = cdiv(B.n, 256);
    hipLaunchKernelGGL(k_echo_count, dim3(nb), dim3(256), 0, st, B, K);
    hipLaunchKernelGGL(k_echo_scan, dim3(1), dim3(256), 0, st, B, K, nb);
    hipLaunchKernelGGL(k_echo_keep, dim3(nb), dim3(256), 0, st, B, F, K);
}
void launch_echo_node_handles(const DevState& S, const EchoBatch& B, const EchoFrames& F, int32_t* hdrop, hipStream_t st) {
    if (B.n) hipLaunchKernelGGL(k_echo_node_handles, dim3(cdiv(B.n, 256)), dim3(256), 0, st, S, B, F, hdrop);
}
void launch_echo_fix(const EchoBatch& B, const EchoKeep& K, const int32_t* hdrop, const int32_t* h, const int32_t* status,
                     const uint32_t* rel, int32_t* out_h, int32_t* out_status, uint32_t* out_rel, hipStream_t st) {
    if (B.n)
        hipLaunchKernelGGL(k_echo_fix, dim3(cdiv(B.n, 256)), dim3(256), 0, st, B, K, hdrop, h, status, rel, out_h, out_status,
                           out_rel);
}
void launch_echo_rebuild(const EchoLedger& from, const EchoLedger& to, uint32_t used, hipStream_t st) {
    if (used) hipLaunchKernelGGL(k_echo_rebuild, dim3(cdiv(used, 256)), dim3(256), 0, st, from, to, used);
}

}  // namespace kwok
