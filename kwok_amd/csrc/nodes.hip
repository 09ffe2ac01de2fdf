// nodes.hip - the node uid directory (kwok_watch.h): a uid per node slot
// beside the device node directory (ingest.hip: node_key / node_name / node_state), and
// the batched name -> handle lookup on that directory.
//
// Per node slot: KWOK_UID_MAX bytes of uid, one byte node_uid_len[slot] = the length in
// its low 6 bits (ND_NO_UID: a node recorded without one) | ND_STALE, and node_uid_key[slot],
// the node_key of the entry the uid was stored for (a placeholder made in a freed slot is
// another node: it does not answer the bytes).  A slot's bytes are never cleared: a Deleted
// node's uid stays answerable (stale) until the slot is created into again.
//
//   k_nd_lookup         ND_LOOKUP_LANES lanes per name.  The group hashes the name once
//                       (every lane reads the same bytes: one broadcast load per byte),
//                       reads the bucket's node_key words ND_LOOKUP_LANES at a time (one
//                       128-byte line per step), a ballot finds the key matches, and only
//                       a matching lane compares the bytes and tests NS_EXISTS.  Names
//                       come from the caller's arena (kwok_node_lookup) ...
//   k_nd_lookup_frames  ... or from the frames' name spans in the resident stream (the
//                       dropped records of kwok_ingest_nodes_framed_echo); both run
//                       nd_group_find
//   k_nd_uid_note       behind the last k_nd_apply of every node batch: one wave per
//                       bucket present in the batch walks the range k_nd_apply walked, in
//                       event order, and applies the uid rule from out_handle / out_status
//                       and the record's op; the lanes copy the uid bytes
//   k_nd_uid_bind       kwok_node_bind: the same store from the caller's arena,
//                       ND_BIND_LANES lanes per item
//   k_nd_frame_recs     the device-input node ingest: one thread per index of a device-resident
//                       list, frames[idx] -> k_json_nodes' off / len / op and the uid span
//   k_nd_stat_scatter   the host codec's statuses of the few documents it decided
//   k_nd_echo_fix       the node form of k_echo_fix: the call's answers in the caller's order
//
// Every loop is bounded by a capacity (cn, a batch's range) or a constant; no block waits
// on another; no local array is indexed dynamically (no scratch).  Counters are added once
// per 1024-thread block (k_nd_uid_note: once per bucket with something to count).
#include <hip/hip_runtime.h>

#include "../../include/kwok_engine.h"
#include "../../include/kwok_watch.h"
#include "device.h"
#include "echo.h"
#include "kernels.h"

namespace kwok {
namespace {

static_assert(KWOK_UID_MAX < ND_NO_UID && ND_NO_UID <= ND_LEN_MASK && KWOK_UID_MAX <= 64, "a uid length fits 6 bits below ND_NO_UID, its bytes one wave");
static_assert(64 % ND_LOOKUP_LANES == 0 && ND_LOOKUP_LANES * 8 == 128, "a step of a lookup group reads one 128-byte line of keys");
static_assert(ND_BIND_LANES * 8 >= KWOK_UID_MAX, "a bind group copies a uid in 8-byte pieces");

constexpr uint32_t COUNT_BLOCK = 1024;  // threads per block of the kernels that count
__device__ __forceinline__ uint32_t lane() { return threadIdx.x & 63u; }
// a counter of the directory: one atomic per block (every thread of the block calls it)
__device__ __forceinline__ void block_add(bool c, unsigned long long* ctr) {
    const int n = __syncthreads_count(c);
    if (threadIdx.x == 0 && n && ctr) atomicAdd(ctr, (unsigned long long)n);
}
__device__ __forceinline__ void mem_sync() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// a byte this wave may have stored for an earlier record: an agent-scope load of its aligned word
__device__ __forceinline__ uint32_t ld8_coh(const uint8_t* p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t w = __hip_atomic_load(reinterpret_cast<uint32_t*>(a & ~(uintptr_t)3), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (w >> (8 * (a & 3))) & 0xFFu;
}
__device__ __forceinline__ bool bytes_eq(const uint8_t* a, const uint8_t* b, uint32_t n) {
    for (uint32_t k = 0; k < n; k++)
        if (a[k] != b[k]) return false;
    return true;
}
__device__ __forceinline__ bool span_ok(uint64_t off, uint32_t len, uint64_t total) { return off <= total && len <= total - off; }

// The existing node (NS_EXISTS) named nm[0, len), or -1, by a group of ND_LOOKUP_LANES lanes of which
// this is lane `sub`; every lane of the wave calls it (the ballots), `valid` false answers -1.  The
// caller checked 1 <= len <= NODE_NAME_MAX and the span for a valid name.
__device__ __forceinline__ int32_t nd_group_find(const DevState& S, const uint8_t* nm, uint32_t len, bool valid, uint32_t sub) {
    uint32_t hs = 0x811C9DC5u;
    if (valid)
        for (uint32_t k = 0; k < len; k++) hs = (hs ^ nm[k]) * 0x01000193u;
    const uint32_t b = hs & (S.buckets - 1);
    const bool mine = valid && b >= S.b_lo && b < S.b_lo + S.nb;
    const uint64_t key = (uint64_t)hs | ((uint64_t)len << 32);
    const size_t nbase = mine ? (size_t)(b - S.b_lo) * S.cn : 0;
    const uint32_t gsh = lane() & ~(ND_LOOKUP_LANES - 1u);  // the group's first lane
    int32_t h = -1;
    for (uint32_t j0 = 0; j0 < S.cn; j0 += ND_LOOKUP_LANES) {  // (S.cn is uniform: the wave stays together)
        const uint32_t j = j0 + sub;
        bool hit = mine && h < 0 && j < S.cn && S.node_key[nbase + j] == key;
        if (hit) hit = (S.node_state[nbase + j] & NS_EXISTS) && bytes_eq(S.node_name + (nbase + j) * NAME_STRIDE, nm, len);
        const uint32_t m = (uint32_t)(__ballot(hit) >> gsh) & ((1u << ND_LOOKUP_LANES) - 1u);
        if (m && h < 0) h = (int32_t)(b * S.cn + j0 + (uint32_t)__builtin_ctz(m));
    }
    return h;
}

__global__ __launch_bounds__(COUNT_BLOCK) void k_nd_lookup(DevState S, NodeDirCounters* ctr, const uint8_t* arena, uint64_t arena_len,
                                                           const uint64_t* off, const uint32_t* len, uint32_t n, int32_t* out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = (uint32_t)(t / ND_LOOKUP_LANES), sub = (uint32_t)(t % ND_LOOKUP_LANES);
    const bool in = t / ND_LOOKUP_LANES < n;
    const uint32_t ln = in ? len[i] : 0u;
    const uint64_t o = in ? off[i] : 0ull;
    const bool valid = in && ln && ln <= NODE_NAME_MAX && span_ok(o, ln, arena_len);
    const int32_t h = nd_group_find(S, arena + (valid ? o : 0), ln, valid, sub);
    if (in && sub == 0) out[i] = h;
    block_add(valid && sub == 0, ctr ? &ctr->lookups : nullptr);
    block_add(h >= 0 && sub == 0, ctr ? &ctr->hits : nullptr);
}

// a dropped node frame's handle (the other records of the call: -1)
__global__ __launch_bounds__(COUNT_BLOCK) void k_nd_lookup_frames(DevState S, NodeDirCounters* ctr, EchoBatch B, EchoFrames F,
                                                                  int32_t* hdrop) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = (uint32_t)(t / ND_LOOKUP_LANES), sub = (uint32_t)(t % ND_LOOKUP_LANES);
    const bool in = t / ND_LOOKUP_LANES < B.n;
    bool valid = false;
    uint32_t ln = 0;
    uint64_t o = 0;
    if (in && B.res[i] == ER_DROP) {
        const uint32_t fi = F.frame_idx[i];
        if (fi < F.n_frames) {
            const kwok_watch_frame* f = F.frames + fi;
            ln = f->name.len, o = f->name.off;
            valid = !(f->flags & KWOK_FRAME_ESC_NAME) && ln && ln <= NODE_NAME_MAX && span_ok(o, ln, B.base_len);
        }
    }
    const int32_t h = nd_group_find(S, B.base + (valid ? o : 0), ln, valid, sub);
    if (in && sub == 0) hdrop[i] = h;
    block_add(valid && sub == 0, &ctr->lookups);
    block_add(h >= 0 && sub == 0, &ctr->hits);
}

constexpr int NOTE_WAVES = 4;
// The uid rule (kwok_watch.h), one wave per bucket: its records of the batch in event order, as k_nd_apply
// applied them.  A DELETE that ended KWOK_OK marks the slot's uid stale; any other record that ended
// KWOK_OK on a slot with no uid or a stale one stores the record's uid (length 0: the entry carried
// none, or the device cannot store it exactly); a slot that holds a live uid keeps it.
__global__ __launch_bounds__(64 * NOTE_WAVES) void k_nd_uid_note(DevState S, NodeBatch N, NodeDirX D, NodeUidNote U) {
    const uint32_t l = lane();
    const uint32_t b = blockIdx.x * NOTE_WAVES + (threadIdx.x >> 6);
    if (b >= S.nb) return;
    const uint32_t pbeg = N.beg[b], pend = N.end[b];
    if (pbeg >= pend || pend > N.n || N.keys_sorted[pbeg] != b) return;  // (stale ranges: k_nd_apply)
    const uint32_t slot0 = b * S.cn;
    uint32_t notes = 0, unbound = 0;
    for (uint32_t p = pbeg; p < pend; p++) {
        const uint32_t idx = N.idx_sorted[p];
        if (idx >= N.n || N.out_status[idx] != KWOK_OK) continue;
        const int64_t s = (int64_t)N.out_handle[idx] - S.node_handle_base;
        if (s < (int64_t)slot0 || s >= (int64_t)slot0 + S.cn) continue;  // (the apply pass answers slots of this bucket only)
        const uint32_t slot = (uint32_t)s;
        mem_sync();  // this wave's stores for the records before, ahead of its coherent load
        const uint32_t cur = ld8_coh(D.node_uid_len + slot);
        if (N.rec[idx].op == KWOK_OP_DELETE) {
            if (l == 0 && !(cur & ND_STALE)) D.node_uid_len[slot] = (uint8_t)(cur | ND_STALE);
            continue;
        }
        const uint32_t clen = cur & ND_LEN_MASK;
        if (clen && clen != ND_NO_UID && !(cur & ND_STALE)) continue;  // a known node keeps its uid
        uint32_t ul = U.ulen ? U.ulen[idx] : 0u;
        const uint32_t uo = ul ? U.uoff[idx] : 0u;
        if (ul > KWOK_UID_MAX || !span_ok(uo, ul, U.stream_len)) ul = 0;
        const bool known = cur == ND_NO_UID;  // a node already recorded without a uid: no create, nothing to rewrite
        if (known && !ul) continue;
        if (l < ul) D.node_uid[(size_t)slot * KWOK_UID_MAX + l] = U.stream[uo + l];
        if (l == 0) {
            D.node_uid_len[slot] = (uint8_t)(ul ? ul : ND_NO_UID);
            D.node_uid_key[slot] = S.node_key[slot];  // whose uid this is (a later entry in the slot may be another node's)
        }
        notes += ul ? 1u : 0u, unbound += ul || known ? 0u : 1u;
    }
    if (l == 0) {
        if (notes) atomicAdd(&D.ctr->notes, (unsigned long long)notes);
        if (unbound) atomicAdd(&D.ctr->unbound, (unsigned long long)unbound);
    }
}

__global__ __launch_bounds__(COUNT_BLOCK) void k_nd_uid_bind(DevState S, NodeDirX D, const int32_t* handles, const uint8_t* arena,
                                                             uint64_t arena_len, const uint64_t* off, const uint32_t* len, uint32_t n) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = (uint32_t)(t / ND_BIND_LANES), sub = (uint32_t)(t % ND_BIND_LANES);
    const bool in = t / ND_BIND_LANES < n;
    bool ok = false;
    if (in) {
        const uint32_t ul = len[i];
        const int64_t s = (int64_t)handles[i] - S.node_handle_base;
        ok = ul && ul <= KWOK_UID_MAX && span_ok(off[i], ul, arena_len) && s >= 0 && s < (int64_t)S.n_node_slots &&
             (S.node_state[s] & NS_EXISTS);
        if (ok) {
            const uint8_t* src = arena + off[i];
            uint8_t* dst = D.node_uid + (size_t)s * KWOK_UID_MAX;
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) {
                const uint32_t q = sub * 8u + k;
                if (q < ul) dst[q] = src[q];
            }
            if (sub == 0) D.node_uid_len[s] = (uint8_t)ul, D.node_uid_key[s] = S.node_key[s];
        }
    }
    block_add(ok && sub == 0, &D.ctr->binds);
    block_add(in && !ok && sub == 0, &D.ctr->bad);
}

// The records of a framed node batch from the resident frames: record k is frame idx[k] of a device-resident
// index list.  off / len / op (null: not wanted) are k_json_nodes' inputs, uoff / ulen the uid span the note
// stores (0 / 0: none the device can store exactly).  strict: the list names ingestible frames only (the echo
// filter's kept records); an index out of range or a frame that is not one sets *err and the record gets the
// out-of-stream span the decode answers with KWOK_EINVAL - nothing is read out of bounds.
__global__ __launch_bounds__(256) void k_nd_frame_recs(const kwok_watch_frame* frames, uint32_t n_frames, uint64_t stream_len,
                                                       const uint32_t* idx, uint32_t n, uint32_t strict, uint64_t* off,
                                                       uint32_t* len, uint8_t* op, uint32_t* uoff, uint8_t* ulen, uint32_t* err) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t fi = idx[k];
    uint64_t o = ~0ull;
    uint32_t ln = 0, uo = 0, ul = 0;
    uint8_t p = KWOK_OP_UPSERT;
    bool ok = false;
    if (fi < n_frames) {
        const kwok_watch_frame f = frames[fi];
        ok = f.status == KWOK_OK && (f.type == KWOK_WATCH_ADDED || f.type == KWOK_WATCH_MODIFIED || f.type == KWOK_WATCH_DELETED);
        if (ok) {
            o = f.doc_off, ln = f.doc_len;
            if (f.type == KWOK_WATCH_DELETED) p = KWOK_OP_DELETE;
            if (!(f.flags & KWOK_FRAME_ESC_UID) && f.uid.len && f.uid.len <= KWOK_UID_MAX && span_ok(f.uid.off, f.uid.len, stream_len))
                uo = f.uid.off, ul = f.uid.len;
        }
    }
    if (!ok && strict) atomicOr(err, 1u);
    if (off) off[k] = o, len[k] = ln, op[k] = p;
    uoff[k] = uo, ulen[k] = (uint8_t)ul;
}

// the host codec's statuses of the documents it decided, into the decode's status array
__global__ __launch_bounds__(256) void k_nd_stat_scatter(int32_t* nstat, const uint32_t* list, const int32_t* vals, uint32_t n) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) nstat[list[q]] = vals[q];
}

// The node form of k_echo_fix: record i of the call in the caller's order.  A kept record (the nk kept ones ran
// through the device-input ingest in kept order) takes its decode status if that is not KWOK_OK, else the apply's
// handle and status; a dropped one KWOK_ECHO with the looked-up handle; the others KWOK_EDOMAIN / KWOK_EINVAL.
// *rejected: the records whose status is neither KWOK_OK nor KWOK_ECHO, added once per block.
__global__ __launch_bounds__(COUNT_BLOCK) void k_nd_echo_fix(EchoBatch B, EchoKeep K, uint32_t nk, const int32_t* hdrop, const int32_t* h,
                                                             const int32_t* st, const int32_t* nstat, int32_t* out_h, int32_t* out_st,
                                                             unsigned long long* rejected) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < B.n) {
        const uint8_t res = B.res[i];
        const uint32_t p = K.kpos[i];
        int32_t hh = -1, s = KWOK_EINVAL;
        if (res == ER_KEEP && p < nk) {
            const int32_t ds = nstat[p];
            s = ds != KWOK_OK ? ds : st[p];
            hh = ds != KWOK_OK ? -1 : h[p];
        } else if (res == ER_DROP) {
            hh = hdrop[i], s = KWOK_ECHO;
        } else if (res == ER_EDOMAIN) {
            s = KWOK_EDOMAIN;
        }
        out_h[i] = hh, out_st[i] = s;
        bad = s != KWOK_OK && s != KWOK_ECHO;
    }
    block_add(bad, rejected);
}

inline uint32_t cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

}  // namespace

void launch_nd_frame_recs(const kwok_watch_frame* frames, uint32_t n_frames, uint64_t stream_len, const uint32_t* idx, uint32_t n,
                          bool strict, uint64_t* off, uint32_t* len, uint8_t* op, uint32_t* uoff, uint8_t* ulen, uint32_t* err,
                          hipStream_t st) {
    if (n)
        hipLaunchKernelGGL(k_nd_frame_recs, dim3(cdiv(n, 256)), dim3(256), 0, st, frames, n_frames, stream_len, idx, n, strict ? 1u : 0u,
                           off, len, op, uoff, ulen, err);
}
void launch_nd_stat_scatter(int32_t* nstat, const uint32_t* list, const int32_t* vals, uint32_t n, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_nd_stat_scatter, dim3(cdiv(n, 256)), dim3(256), 0, st, nstat, list, vals, n);
}
void launch_nd_echo_fix(const EchoBatch& B, const EchoKeep& K, uint32_t nk, const int32_t* hdrop, const int32_t* h, const int32_t* status,
                        const int32_t* nstat, int32_t* out_h, int32_t* out_status, unsigned long long* rejected, hipStream_t st) {
    if (B.n)
        hipLaunchKernelGGL(k_nd_echo_fix, dim3(cdiv(B.n, COUNT_BLOCK)), dim3(COUNT_BLOCK), 0, st, B, K, nk, hdrop, h, status, nstat, out_h,
                           out_status, rejected);
}

void launch_nd_lookup(const DevState& S, NodeDirCounters* ctr, const uint8_t* arena, uint64_t arena_len, const uint64_t* off,
                      const uint32_t* len, uint32_t n, int32_t* out, hipStream_t st) {
    if (n)
        hipLaunchKernelGGL(k_nd_lookup, dim3(cdiv((uint64_t)n * ND_LOOKUP_LANES, COUNT_BLOCK)), dim3(COUNT_BLOCK), 0, st, S, ctr, arena,
                           arena_len, off, len, n, out);
}
void launch_nd_lookup_frames(const DevState& S, const NodeDirX& D, const EchoBatch& B, const EchoFrames& F, int32_t* hdrop,
                             hipStream_t st) {
    if (B.n)
        hipLaunchKernelGGL(k_nd_lookup_frames, dim3(cdiv((uint64_t)B.n * ND_LOOKUP_LANES, COUNT_BLOCK)), dim3(COUNT_BLOCK), 0, st, S, D.ctr,
                           B, F, hdrop);
}
void launch_nd_uid_note(const DevState& S, const NodeBatch& N, const NodeDirX& D, const NodeUidNote& U, hipStream_t st) {
    if (N.n) hipLaunchKernelGGL(k_nd_uid_note, dim3(cdiv(S.nb, NOTE_WAVES)), dim3(64 * NOTE_WAVES), 0, st, S, N, D, U);
}
void launch_nd_uid_bind(const DevState& S, const NodeDirX& D, const int32_t* handles, const uint8_t* arena, uint64_t arena_len,
                        const uint64_t* off, const uint32_t* len, uint32_t n, hipStream_t st) {
    if (n)
        hipLaunchKernelGGL(k_nd_uid_bind, dim3(cdiv((uint64_t)n * ND_BIND_LANES, COUNT_BLOCK)), dim3(COUNT_BLOCK), 0, st, S, D, handles,
                           arena, arena_len, off, len, n);
}

}  // namespace kwok
