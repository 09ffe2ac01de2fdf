// refs.hip - the pod and node reference directory (kwok_watch.h): what a
// patch is addressed to, kept per slot and handed back in the order of a handle list.
//
// Per pod slot: KWOK_REF_STRIDE bytes holding the namespace and then the name from the
// record's first byte, and pod_ref_len[slot] = ns_len | name_len << 8 (0: no name
// stored).  The uid is the uid directory's (pod_uid, stride KWOK_UID_MAX = 40, so it is
// read in 8-byte words); a node's name is the node directory's (S.node_name, node_key).
// Freeing a slot touches none of these bytes.
//
//   k_refs_note    behind the apply pass of every pod chunk, next to k_uid_note: a create
//                  through a by-uid entry takes its frame's namespace and name from the
//                  resident stream; any other create, and a frame whose name the device
//                  cannot store exactly, stores length 0.  REF_NOTE_LANES lanes per
//                  record, each writes whole 16-byte units of the record
//   k_refs_bind    kwok_refs_bind: the same store from the caller's arena
//   k_refs_size    one thread per item of a handle list: status, lengths, the padded size
//                  (reads the length array and the state word, no record)
//   (rocprim exclusive scan of the sizes)
//   k_refs_gather  REF_GATHER_LANES lanes per item: only the units the lengths say are in
//                  use, 16-byte loads of the record, 8-byte loads of the uid, aligned
//                  16-byte stores of the item; the group's first lane writes refs[i]
//   k_refs_size_nd / k_refs_gather_nd  the two above for node queries while the node uid directory
//                  (nodes.hip) is on: the uid behind the name, from node_uid (stride
//                  40) and node_uid_len (length | ND_STALE)
//
// Every loop is bounded by a constant; no block waits on another; no kernel indexes a
// local array dynamically (no scratch).  The kernels that count (notes, binds, reads) add
// once per 1024-thread block.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <rocprim/device/device_scan.hpp>

#include "../../include/kwok_engine.h"
#include "../../include/kwok_watch.h"
#include "device.h"
#include "kernels.h"

namespace kwok {
namespace {

static_assert(KWOK_REF_STRIDE % 16 == 0 && KWOK_REF_NS_MAX + KWOK_REF_NAME_MAX <= KWOK_REF_STRIDE, "record units");
static_assert(NAME_STRIDE % 16 == 0 && KWOK_UID_MAX % 8 == 0, "node names in 16-byte units, uids in 8-byte words");
static_assert(sizeof(kwok_ref) == 16 && offsetof(kwok_ref, ns_len) == 8 && offsetof(kwok_ref, status) == 11, "kwok_ref is 16 bytes");
constexpr uint32_t REC_UNITS = (KWOK_REF_NS_MAX + KWOK_REF_NAME_MAX + 15) / 16;                   // 20
constexpr uint32_t ITEM_UNITS = (KWOK_REF_NS_MAX + KWOK_REF_NAME_MAX + KWOK_UID_MAX + 15) / 16;  // 23
constexpr uint32_t NOTE_STEPS = (REC_UNITS + REF_NOTE_LANES - 1) / REF_NOTE_LANES;
constexpr uint32_t GATHER_STEPS = (ITEM_UNITS + REF_GATHER_LANES - 1) / REF_GATHER_LANES;

// a counter of the directory: one atomic per block (every thread of the block calls it).  The counters sit on one
// address: with an add per wave the adds of a 2M-record batch queue behind each other for longer than the stores take
constexpr uint32_t COUNT_BLOCK = 1024;  // threads per block of the kernels that count
__device__ __forceinline__ void block_add(bool c, unsigned long long* ctr) {
    const int n = __syncthreads_count(c);
    if (threadIdx.x == 0 && n) atomicAdd(ctr, (unsigned long long)n);
}
// pod handle -> local slot of an owned bucket (the inverse of pod_handle_of), or false
__device__ __forceinline__ bool pod_slot_of(const DevState& S, int32_t h, uint32_t* slot) {
    if (h < 0) return false;
    const uint32_t b = (uint32_t)h / S.pod_stride, idx = (uint32_t)h - b * S.pod_stride;
    if (b < S.b_lo || b >= S.b_lo + S.nb || idx >= S.cp) return false;
    *slot = (b - S.b_lo) * S.cp + idx;
    return true;
}
// unit u (16 bytes) of the concatenation a[0, la) | b[0, lb), zero past its end
__device__ __forceinline__ uint4 cat_unit(const uint8_t* a, uint32_t la, const uint8_t* b, uint32_t lb, uint32_t u) {
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        const uint32_t p = 16u * u + k;
        uint32_t v = 0;
        if (p < la) v = a[p];
        else if (p - la < lb) v = b[p - la];
        v <<= (k & 3u) * 8u;
        if (k < 4) w0 |= v;
        else if (k < 8) w1 |= v;
        else if (k < 12) w2 |= v;
        else w3 |= v;
    }
    return make_uint4(w0, w1, w2, w3);
}
// the slot's record <- ns | name (lengths checked by the caller; 0, 0: no name), by the `sub`-th of REF_NOTE_LANES lanes
__device__ __forceinline__ void ref_store(const RefDir& R, uint32_t slot, const uint8_t* ns, uint32_t nsl, const uint8_t* name,
                                          uint32_t nl, uint32_t sub) {
    const uint32_t units = (nsl + nl + 15u) >> 4;
    uint4* dst = reinterpret_cast<uint4*>(R.pod_ref + (size_t)slot * KWOK_REF_STRIDE);
#pragma unroll
    for (uint32_t k = 0; k < NOTE_STEPS; k++) {
        const uint32_t u = sub + k * REF_NOTE_LANES;
        if (u < units && u < REC_UNITS) dst[u] = cat_unit(ns, nsl, name, nl, u);
    }
    if (sub == 0) R.pod_ref_len[slot] = (uint16_t)(nsl | (nl << 8));
}
__device__ __forceinline__ bool span_ok(uint64_t off, uint32_t len, uint64_t total) { return off <= total && len <= total - off; }

__global__ __launch_bounds__(COUNT_BLOCK) void k_refs_note(DevState S, IngestBatch I, RefDir R, RefNote N) {
    // a speculative apply pass that returned for growth wrote no result: the redo notes
    if (I.spec && (I.sum->need > S.cp || *I.abort)) return;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = (uint32_t)(t / REF_NOTE_LANES), sub = (uint32_t)(t % REF_NOTE_LANES);
    bool named = false, unnamed = false;
    if (i < I.n) {
        const PodRec r = I.rec[i];
        uint32_t slot = 0;
        const bool create = r.op == KWOK_OP_UPSERT && !(r.chk & REC_EXISTING) && I.out_status[i] == KWOK_OK &&
                            pod_slot_of(S, I.out_handle[i], &slot);
        if (create) {
            uint32_t nso = 0, nsl = 0, no = 0, nl = 0;
            if (N.cls && N.cls[i] == UID_NEW) {
                const uint32_t fi = N.frame_idx[i];
                if (fi < N.n_frames) {
                    const kwok_watch_frame* f = N.frames + fi;
                    const kwok_str nm = f->name, ns = f->namespace_;
                    if (!(f->flags & (KWOK_FRAME_ESC_NAME | KWOK_FRAME_ESC_NS)) && nm.len && nm.len <= KWOK_REF_NAME_MAX &&
                        ns.len <= KWOK_REF_NS_MAX && span_ok(nm.off, nm.len, N.stream_len) &&
                        span_ok(ns.off, ns.len, N.stream_len))
                        nso = ns.off, nsl = ns.len, no = nm.off, nl = nm.len;
                }
            }
            // (no name: length 0, a reused slot must not keep its previous pod's)
            ref_store(R, slot, N.stream + nso, nsl, N.stream + no, nl, sub);
            named = nl && sub == 0;
            unnamed = !nl && sub == 0;
        }
    }
    block_add(named, &R.ctr->notes);
    block_add(unnamed, &R.ctr->unnamed);
}

__global__ __launch_bounds__(COUNT_BLOCK) void k_refs_bind(DevState S, RefDir R, const int32_t* handles, const uint8_t* arena,
                                                   uint64_t arena_len, const uint64_t* ns_off, const uint32_t* ns_len,
                                                   const uint64_t* name_off, const uint32_t* name_len, uint32_t n) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = (uint32_t)(t / REF_NOTE_LANES), sub = (uint32_t)(t % REF_NOTE_LANES);
    bool ok = false;
    if (i < n) {
        uint32_t slot = 0;
        const uint32_t nsl = ns_len[i], nl = name_len[i];
        ok = nl && nl <= KWOK_REF_NAME_MAX && nsl <= KWOK_REF_NS_MAX && span_ok(name_off[i], nl, arena_len) &&
             (!nsl || span_ok(ns_off[i], nsl, arena_len)) && pod_slot_of(S, handles[i], &slot) && (S.pod_state[slot] & PS_USED);
        if (ok) ref_store(R, slot, arena + (nsl ? ns_off[i] : 0), nsl, arena + name_off[i], nl, sub);
    }
    block_add(ok && sub == 0, &R.ctr->binds);
    block_add(i < n && !ok && sub == 0, &R.ctr->bad);
}

__global__ __launch_bounds__(COUNT_BLOCK) void k_refs_size(DevState S, RefDir R, RefQuery Q, uint32_t* slots) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool read = false, missing = false;
    if (i < Q.n) {
        const int32_t h = Q.handles[Q.first + i];
        uint32_t slot = 0, nsl = 0, nl = 0, ul = 0;
        int32_t status = KWOK_ENOTFOUND;
        if (Q.pods) {
            if (pod_slot_of(S, h, &slot) && (Q.any_slot || (S.pod_state[slot] & PS_USED))) {
                const uint32_t l = R.pod_ref_len[slot];
                ul = min((uint32_t)R.pod_uid_len[slot], (uint32_t)KWOK_UID_MAX);
                nl = min(l >> 8, (uint32_t)KWOK_REF_NAME_MAX);
                nsl = nl ? min(l & 255u, (uint32_t)KWOK_REF_NS_MAX) : 0u;
                status = nl ? KWOK_OK : KWOK_REF_NONE;
            }
        } else {
            const int64_t s = (int64_t)h - S.node_handle_base;
            if (s >= 0 && s < (int64_t)S.n_node_slots) {
                slot = (uint32_t)s;
                const uint64_t key = S.node_key[slot];
                if (key && (Q.any_slot || (S.node_state[slot] & NS_SLOT))) {
                    nl = min((uint32_t)(key >> 32), NODE_NAME_MAX);
                    status = nl ? KWOK_OK : KWOK_ENOTFOUND;
                }
            }
        }
        // kwok_ref as one 16-byte store: off (0 until the gather), the lengths and the status, reserved0
        reinterpret_cast<uint4*>(Q.refs)[i] = make_uint4(0u, 0u, nsl | (nl << 8) | (ul << 16) | ((uint32_t)(uint8_t)status << 24), 0u);
        Q.len[i] = (uint64_t)((nsl + nl + ul + 15u) & ~15u);
        slots[i] = slot;
        read = true;
        missing = status == KWOK_ENOTFOUND;
    }
    block_add(read, &R.ctr->reads);
    block_add(missing, &R.ctr->not_found);
}

// word k of the slot's uid (8 bytes), zero outside [0, ul)
__device__ __forceinline__ uint64_t uid_word(const uint8_t* uid, uint32_t ul, int32_t k) {
    if (k < 0 || (uint32_t)k * 8u >= ul) return 0;
    uint64_t w = reinterpret_cast<const uint64_t*>(uid)[k];
    const uint32_t rem = ul - (uint32_t)k * 8u;
    if (rem < 8) w &= (1ull << (rem * 8u)) - 1ull;
    return w;
}
// the 8 bytes of the uid at byte offset o (negative: before its first byte), zero outside it
__device__ __forceinline__ uint64_t uid_at(const uint8_t* uid, uint32_t ul, int32_t o) {
    const int32_t k = o >> 3;
    const uint32_t sh = ((uint32_t)o & 7u) * 8u;
    const uint64_t w0 = uid_word(uid, ul, k);
    if (!sh) return w0;
    return (w0 >> sh) | (uid_word(uid, ul, k + 1) << (64u - sh));
}

__global__ __launch_bounds__(256) void k_refs_gather(DevState S, RefDir R, RefQuery Q, const uint32_t* slots) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = (uint32_t)(t / REF_GATHER_LANES), sub = (uint32_t)(t % REF_GATHER_LANES);
    if (i >= Q.n) return;
    const uint32_t packed = reinterpret_cast<const uint4*>(Q.refs)[i].z;  // ns_len | name_len << 8 | uid_len << 16 | status << 24
    const uint64_t off = Q.off[i];
    const uint32_t slot = slots[i];
    const uint32_t a = (packed & 255u) + ((packed >> 8) & 255u), ul = (packed >> 16) & 255u, units = (a + ul + 15u) >> 4;
    const uint8_t* rec = Q.pods ? R.pod_ref + (size_t)slot * KWOK_REF_STRIDE : S.node_name + (size_t)slot * NAME_STRIDE;
    const uint8_t* uid = R.pod_uid + (size_t)slot * KWOK_UID_MAX;  // (read only when ul != 0: pods)
    uint4* dst = reinterpret_cast<uint4*>(Q.blob + off);
#pragma unroll
    for (uint32_t k = 0; k < GATHER_STEPS; k++) {
        const uint32_t u = sub + k * REF_GATHER_LANES;
        if (u >= units || u >= ITEM_UNITS) continue;
        uint64_t lo = 0, hi = 0;
        if (16u * u < a) {  // bytes of the record: the unit, cut at the name's end
            const uint4 v = reinterpret_cast<const uint4*>(rec)[u];
            lo = v.x | ((uint64_t)v.y << 32), hi = v.z | ((uint64_t)v.w << 32);
            const uint32_t rem = a - 16u * u;
            if (rem <= 8) hi = 0;
            if (rem < 8) lo &= (1ull << (rem * 8u)) - 1ull;
            else if (rem > 8 && rem < 16) hi &= (1ull << ((rem - 8u) * 8u)) - 1ull;
        }
        if (ul && 16u * u + 16u > a) {  // bytes of the uid, which starts at byte a of the item
            const int32_t o = (int32_t)(16u * u) - (int32_t)a;
            lo |= uid_at(uid, ul, o), hi |= uid_at(uid, ul, o + 8);
        }
        dst[u] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    }
    if (sub == 0) reinterpret_cast<uint4*>(Q.refs)[i] = make_uint4((uint32_t)off, (uint32_t)(off >> 32), packed, 0u);
}

// ---- node queries with the node uid directory on: the uid behind the name.  Kernels of their
// own, so that k_refs_size / k_refs_gather (pods, and nodes with the directory off) stay what they were ----
__global__ __launch_bounds__(COUNT_BLOCK) void k_refs_size_nd(DevState S, RefDir R, NodeDirX D, RefQuery Q, uint32_t* slots) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool read = false, missing = false;
    if (i < Q.n) {
        const int32_t h = Q.handles[Q.first + i];
        uint32_t slot = 0, nl = 0, ul = 0;
        int32_t status = KWOK_ENOTFOUND;
        const int64_t s = (int64_t)h - S.node_handle_base;
        if (s >= 0 && s < (int64_t)S.n_node_slots) {
            slot = (uint32_t)s;
            const uint64_t key = S.node_key[slot];
            const uint32_t lb = D.node_uid_len[slot];
            // a stale uid (its node was deleted) is what the slot last stored: KWOK_REFS_ANY_SLOT alone answers it
            const uint32_t ln = lb & (uint32_t)ND_LEN_MASK;
            // ... and only of the entry it was stored for: a placeholder made in a freed slot is another node
            const bool own = !key || D.node_uid_key[slot] == key;
            const uint32_t stored = own && ln != ND_NO_UID && (Q.any_slot || !(lb & ND_STALE)) ? min(ln, (uint32_t)KWOK_UID_MAX) : 0u;
            if (key && (Q.any_slot || (S.node_state[slot] & NS_SLOT))) {
                nl = min((uint32_t)(key >> 32), NODE_NAME_MAX);
                status = nl ? KWOK_OK : KWOK_ENOTFOUND;
                ul = nl ? stored : 0u;
            } else if (!key && Q.any_slot && stored) {  // the entry is gone, its uid bytes remain
                status = KWOK_REF_NONE;
                ul = stored;
            }
        }
        reinterpret_cast<uint4*>(Q.refs)[i] = make_uint4(0u, 0u, (nl << 8) | (ul << 16) | ((uint32_t)(uint8_t)status << 24), 0u);
        Q.len[i] = (uint64_t)((nl + ul + 15u) & ~15u);
        slots[i] = slot;
        read = true;
        missing = status == KWOK_ENOTFOUND;
    }
    block_add(read, &R.ctr->reads);
    block_add(missing, &R.ctr->not_found);
}

__global__ __launch_bounds__(256) void k_refs_gather_nd(DevState S, NodeDirX D, RefQuery Q, const uint32_t* slots) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = (uint32_t)(t / REF_GATHER_LANES), sub = (uint32_t)(t % REF_GATHER_LANES);
    if (i >= Q.n) return;
    const uint32_t packed = reinterpret_cast<const uint4*>(Q.refs)[i].z;  // name_len << 8 | uid_len << 16 | status << 24
    const uint64_t off = Q.off[i];
    const uint32_t slot = slots[i];
    const uint32_t a = (packed >> 8) & 255u, ul = (packed >> 16) & 255u, units = (a + ul + 15u) >> 4;
    const uint8_t* rec = S.node_name + (size_t)slot * NAME_STRIDE;
    const uint8_t* uid = D.node_uid + (size_t)slot * KWOK_UID_MAX;
    uint4* dst = reinterpret_cast<uint4*>(Q.blob + off);
#pragma unroll
    for (uint32_t k = 0; k < GATHER_STEPS; k++) {
        const uint32_t u = sub + k * REF_GATHER_LANES;
        if (u >= units || u >= ITEM_UNITS) continue;
        uint64_t lo = 0, hi = 0;
        if (16u * u < a) {  // bytes of the name: the unit, cut at its end
            const uint4 v = reinterpret_cast<const uint4*>(rec)[u];
            lo = v.x | ((uint64_t)v.y << 32), hi = v.z | ((uint64_t)v.w << 32);
            const uint32_t rem = a - 16u * u;
            if (rem <= 8) hi = 0;
            if (rem < 8) lo &= (1ull << (rem * 8u)) - 1ull;
            else if (rem > 8 && rem < 16) hi &= (1ull << ((rem - 8u) * 8u)) - 1ull;
        }
        if (ul && 16u * u + 16u > a) {  // bytes of the uid, which starts at byte a of the item
            const int32_t o = (int32_t)(16u * u) - (int32_t)a;
            lo |= uid_at(uid, ul, o), hi |= uid_at(uid, ul, o + 8);
        }
        dst[u] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    }
    if (sub == 0) reinterpret_cast<uint4*>(Q.refs)[i] = make_uint4((uint32_t)off, (uint32_t)(off >> 32), packed, 0u);
}

inline uint32_t cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

}  // namespace

void launch_refs_size_nd(const DevState& S, const RefDir& R, const NodeDirX& D, const RefQuery& Q, uint32_t* slots, hipStream_t st) {
    if (Q.n) hipLaunchKernelGGL(k_refs_size_nd, dim3(cdiv(Q.n, COUNT_BLOCK)), dim3(COUNT_BLOCK), 0, st, S, R, D, Q, slots);
}
void launch_refs_gather_nd(const DevState& S, const NodeDirX& D, const RefQuery& Q, const uint32_t* slots, hipStream_t st) {
    if (Q.n)
        hipLaunchKernelGGL(k_refs_gather_nd, dim3(cdiv((uint64_t)Q.n * REF_GATHER_LANES, 256)), dim3(256), 0, st, S, D, Q, slots);
}
void launch_refs_note(const DevState& S, const IngestBatch& I, const RefDir& R, const RefNote& N, hipStream_t st) {
    if (I.n)
        hipLaunchKernelGGL(k_refs_note, dim3(cdiv((uint64_t)I.n * REF_NOTE_LANES, COUNT_BLOCK)), dim3(COUNT_BLOCK), 0, st, S, I, R, N);
}
void launch_refs_bind(const DevState& S, const RefDir& R, const int32_t* handles, const uint8_t* arena, uint64_t arena_len,
                      const uint64_t* ns_off, const uint32_t* ns_len, const uint64_t* name_off, const uint32_t* name_len,
                      uint32_t n, hipStream_t st) {
    if (n)
        hipLaunchKernelGGL(k_refs_bind, dim3(cdiv((uint64_t)n * REF_NOTE_LANES, COUNT_BLOCK)), dim3(COUNT_BLOCK), 0, st, S, R, handles, arena,
                           arena_len, ns_off, ns_len, name_off, name_len, n);
}
void launch_refs_size(const DevState& S, const RefDir& R, const RefQuery& Q, uint32_t* slots, hipStream_t st) {
    if (Q.n) hipLaunchKernelGGL(k_refs_size, dim3(cdiv(Q.n, COUNT_BLOCK)), dim3(COUNT_BLOCK), 0, st, S, R, Q, slots);
}
size_t refs_scan_bytes(uint32_t n) {
    size_t bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)n,
                                  rocprim::plus<uint64_t>());
    return bytes;
}
int launch_refs_scan(const RefQuery& Q, void* tmp, size_t tmp_bytes, hipStream_t st) {
    if (!Q.n) return KWOK_OK;
    return rocprim::exclusive_scan(tmp, tmp_bytes, (const uint64_t*)Q.len, Q.off, (uint64_t)0, (size_t)Q.n,
                                   rocprim::plus<uint64_t>(), st) == hipSuccess
               ? KWOK_OK
               : KWOK_EDEVICE;
}
// the same scan over any sizes (the node status blob canonicaliser places its blobs with it)
int launch_scan64(const uint64_t* in, uint64_t* out, uint32_t n, void* tmp, size_t tmp_bytes, hipStream_t st) {
    if (!n) return KWOK_OK;
    return rocprim::exclusive_scan(tmp, tmp_bytes, in, out, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), st) == hipSuccess
               ? KWOK_OK
               : KWOK_EDEVICE;
}
void launch_refs_gather(const DevState& S, const RefDir& R, const RefQuery& Q, const uint32_t* slots, hipStream_t st) {
    if (Q.n)
        hipLaunchKernelGGL(k_refs_gather, dim3(cdiv((uint64_t)Q.n * REF_GATHER_LANES, 256)), dim3(256), 0, st, S, R, Q, slots);
}

}  // namespace kwok
