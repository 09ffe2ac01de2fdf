// resync.hip - relist with Replace (kwok_watch.h): the `seen`
// marks of a resync session and the sweep of the objects a complete List did
// not hold.
//
// One byte per pod slot / node slot (pod_seen, node_seen): a mark is a plain,
// idempotent byte store, no atomics.
//
//   k_seen_mark_*   one thread per record of an applied batch (or per handle of
//                   kwok_resync_mark): UPSERT + KWOK_OK -> handle -> local slot ->
//                   seen[slot] = 1.  Launched only while the kind's session is open.
//   k_sweep_count   one block per tile of slots (pods: tiles laid over whole
//                   buckets, stopping at the bucket's fill mark; 8 state words and 8
//                   mark bytes per lane): live && !seen per lane, popcount, wave
//                   shuffle, LDS -> one count per tile.
//   k_frame_scan    (json.hip) over the tile counts; the total goes to the host.
//   k_sweep_emit    the second pass: a block scan of the lanes' popcounts gives
//                   every unmarked object its rank in slot order (= ascending
//                   handle, the canonical order); at base + rank it writes the
//                   object's DELETE record, its handle and (pods) its node's handle.
//
// No block waits on another.  The records then run through the ingest's own
// chain (k_ing_prep -> bucket sort -> k_ing_apply; k_nd_prep -> sort ->
// k_nd_apply): the event switch is not restated here.
#include <hip/hip_runtime.h>

#include "../../include/kwok_engine.h"
#include "../../include/kwok_watch.h"
#include "device.h"
#include "kernels.h"

namespace kwok {
namespace {

constexpr uint32_t SW_THREADS = 256;
static_assert(SWEEP_POD_TILE == SW_THREADS * 8, "a lane takes 8 pod slots (one 16-byte load of states)");
static_assert(SWEEP_NODE_TILE == SW_THREADS * 4, "a lane takes 4 node slots (one 4-byte load of states)");

__device__ __forceinline__ uint32_t lane() { return threadIdx.x & 63u; }
__device__ __forceinline__ uint32_t wave_incl(uint32_t x) {
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, (unsigned)o);
        if ((int)lane() >= o) x += y;
    }
    return x;
}
// marks stored by the wave (one atomic per wave that stored any)
__device__ __forceinline__ void count_marks(bool m, bool bad, ResyncCounters* rc) {
    const uint64_t mm = __ballot(m), mb = __ballot(bad);
    if (lane() == 0) {
        if (mm) atomicAdd(&rc->marked, (unsigned long long)__popcll(mm));
        if (mb) atomicAdd(&rc->bad, (unsigned long long)__popcll(mb));
    }
}
// pod handle -> local slot of an owned bucket (the inverse of pod_handle_of), or false
__device__ __forceinline__ bool pod_slot_of(const DevState& S, int32_t h, size_t* slot) {
    if (h < 0) return false;
    const uint32_t b = (uint32_t)h / S.pod_stride, idx = (uint32_t)h - b * S.pod_stride;
    if (b < S.b_lo || b >= S.b_lo + S.nb || idx >= S.cp) return false;
    *slot = (size_t)(b - S.b_lo) * S.cp + idx;
    return true;
}
// node handle ((b_lo + b) * cn + nd) -> local slot, or false
__device__ __forceinline__ bool node_slot_of(const DevState& S, int32_t h, size_t* slot) {
    const int64_t l = (int64_t)h - (int64_t)S.b_lo * S.cn;
    if (h < 0 || l < 0 || l >= (int64_t)S.n_node_slots) return false;
    *slot = (size_t)l;
    return true;
}

__global__ __launch_bounds__(256) void k_seen_mark_pods(DevState S, IngestBatch I, uint8_t* seen, ResyncCounters* rc) {
    // a speculative apply pass that returned for growth wrote no result: the redo marks
    if (I.spec && (I.sum->need > S.cp || *I.abort)) return;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool m = false;
    size_t slot = 0;
    if (i < I.n && I.rec[i].op == KWOK_OP_UPSERT && I.out_status[i] == KWOK_OK) m = pod_slot_of(S, I.out_handle[i], &slot);
    if (m) seen[slot] = 1;
    count_marks(m, false, rc);
}
__global__ __launch_bounds__(256) void k_seen_mark_nodes(DevState S, NodeBatch N, uint8_t* seen, ResyncCounters* rc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool m = false;
    size_t slot = 0;
    if (i < N.n && N.rec[i].op == KWOK_OP_UPSERT && N.out_status[i] == KWOK_OK) m = node_slot_of(S, N.out_handle[i], &slot);
    if (m) seen[slot] = 1;
    count_marks(m, false, rc);
}
__global__ __launch_bounds__(256) void k_seen_mark_handles(DevState S, int pods, const int32_t* handles, uint32_t n,
                                                           uint8_t* seen, ResyncCounters* rc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool m = false;
    size_t slot = 0;
    if (i < n) {
        if (pods) m = pod_slot_of(S, handles[i], &slot) && (S.pod_state[slot] & PS_USED);
        else m = node_slot_of(S, handles[i], &slot) && (S.node_state[slot] & NS_SLOT);
    }
    if (m) seen[slot] = 1;
    count_marks(m, i < n && !m, rc);
}

// ---- the sweep's windows: bit j = the lane's j-th slot is live and carries no mark ----
// pods: tile t covers slots [(t % tpb) * SWEEP_POD_TILE, +SWEEP_POD_TILE) of bucket t / tpb, below its
// fill mark (cp and the fill marks are multiples of 8: 16-byte state loads, 8-byte mark loads)
__device__ __forceinline__ uint32_t pod_window(const DevState& S, const uint8_t* seen, uint32_t tpb, size_t* g0) {
    const uint32_t b = blockIdx.x / tpb, s = (blockIdx.x % tpb) * SWEEP_POD_TILE + threadIdx.x * 8u;
    const size_t g = (size_t)b * S.cp + s;
    *g0 = g;
    if (s >= S.pod_fill[b]) return 0;
    const uint4 st = *reinterpret_cast<const uint4*>(S.pod_state + g);
    const uint2 mk = *reinterpret_cast<const uint2*>(seen + g);
    const uint32_t w[4] = {st.x, st.y, st.z, st.w};
    const uint64_t mk64 = (uint64_t)mk.x | ((uint64_t)mk.y << 32);
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        m |= (w[k] & PS_USED) << (2 * k);
        m |= ((w[k] >> 16) & PS_USED) << (2 * k + 1);
    }
#pragma unroll
    for (int j = 0; j < 8; j++)
        if ((mk64 >> (8 * j)) & 0xFFu) m &= ~(1u << j);
    return m;
}
static_assert(PS_USED == 1, "pod_window takes PS_USED as bit 0 of a state word");
// nodes: tile t covers node slots [t * SWEEP_NODE_TILE, +SWEEP_NODE_TILE) (ascending slot = ascending handle)
__device__ __forceinline__ uint32_t node_window(const DevState& S, const uint8_t* seen, size_t* g0) {
    const size_t g = (size_t)blockIdx.x * SWEEP_NODE_TILE + threadIdx.x * 4u;
    *g0 = g;
    if (g >= S.n_node_slots) return 0;
    uint32_t st, mk;
    if (g + 4 <= S.n_node_slots) {
        st = *reinterpret_cast<const uint32_t*>(S.node_state + g);
        mk = *reinterpret_cast<const uint32_t*>(seen + g);
    } else {
        st = mk = 0;
        for (uint32_t j = 0; g + j < S.n_node_slots; j++) {
            st |= (uint32_t)S.node_state[g + j] << (8 * j);
            mk |= (uint32_t)seen[g + j] << (8 * j);
        }
    }
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (((st >> (8 * j)) & NS_EXISTS) && !((mk >> (8 * j)) & 0xFFu)) m |= 1u << j;
    return m;
}

template <bool PODS>
__global__ __launch_bounds__(SW_THREADS) void k_sweep_count(DevState S, const uint8_t* seen, uint32_t tpb, uint32_t* tile_cnt) {
    __shared__ uint32_t wsum[SW_THREADS / 64];
    size_t g;
    uint32_t c = __popc(PODS ? pod_window(S, seen, tpb, &g) : node_window(S, seen, &g));
    for (uint32_t o = 32; o; o >>= 1) c += __shfl_down(c, o);
    if (lane() == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < SW_THREADS / 64; w++) t += wsum[w];
        tile_cnt[blockIdx.x] = t;
    }
}

template <bool PODS>
__global__ __launch_bounds__(SW_THREADS) void k_sweep_emit(DevState S, const uint8_t* seen, uint32_t tpb, const uint32_t* tile_base,
                                                          uint32_t n_out, void* recs, int32_t* handles, int32_t* nodes) {
    __shared__ uint32_t wtot[SW_THREADS / 64];
    size_t g;
    uint32_t m = PODS ? pod_window(S, seen, tpb, &g) : node_window(S, seen, &g);
    const uint32_t c = __popc(m), incl = wave_incl(c), wave = threadIdx.x >> 6;
    if (lane() == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t k = tile_base[blockIdx.x] + incl - c;
    for (uint32_t w = 0; w < wave; w++) k += wtot[w];
    while (m) {
        const uint32_t j = (uint32_t)__builtin_ctz(m);
        m &= m - 1;
        const size_t slot = g + j;
        if (k < n_out) {
            if (PODS) {
                const int32_t h = pod_handle_of(S, (uint32_t)slot);
                kwok_pod_rec r;
                r.op = KWOK_OP_DELETE;
                r.flags = 0;
                r.spec_id = 0;
                r.target = h;
                r.creation = 0;
                r.host_ip = 0;
                r.pod_ip = S.pod_ip[slot];  // the Deleted event's status.podIP: the address the slot holds
                static_cast<kwok_pod_rec*>(recs)[k] = r;
                handles[k] = h;
                nodes[k] = (int32_t)((S.b_lo + (uint32_t)(slot / S.cp)) * S.cn + S.pod_node[slot]);
            } else {
                kwok_node_event ev = {};
                ev.op = KWOK_OP_DELETE;
                ev.name.off = (uint32_t)(slot * NAME_STRIDE);  // into the directory's own names (the batch's arena)
                ev.name.len = (uint32_t)(S.node_key[slot] >> 32);
                static_cast<kwok_node_event*>(recs)[k] = ev;
                handles[k] = (int32_t)(S.b_lo * S.cn + (uint32_t)slot);
            }
        }
        k++;
    }
}

inline uint32_t cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }
inline uint32_t tiles_per_bucket(const DevState& S) { return cdiv(S.cp, SWEEP_POD_TILE); }

}  // namespace

void launch_seen_mark_pods(const DevState& S, const IngestBatch& I, uint8_t* seen, ResyncCounters* rc, hipStream_t st) {
    if (I.n) hipLaunchKernelGGL(k_seen_mark_pods, dim3(cdiv(I.n, 256)), dim3(256), 0, st, S, I, seen, rc);
}
void launch_seen_mark_nodes(const DevState& S, const NodeBatch& N, uint8_t* seen, ResyncCounters* rc, hipStream_t st) {
    if (N.n) hipLaunchKernelGGL(k_seen_mark_nodes, dim3(cdiv(N.n, 256)), dim3(256), 0, st, S, N, seen, rc);
}
void launch_seen_mark_handles(const DevState& S, int pods, const int32_t* handles, uint32_t n, uint8_t* seen,
                              ResyncCounters* rc, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_seen_mark_handles, dim3(cdiv(n, 256)), dim3(256), 0, st, S, pods, handles, n, seen, rc);
}
uint32_t sweep_tiles(const DevState& S, int pods) {
    return pods ? S.nb * tiles_per_bucket(S) : cdiv(S.n_node_slots, SWEEP_NODE_TILE);
}
void launch_sweep_count(const DevState& S, int pods, const uint8_t* seen, uint32_t* tile_cnt, hipStream_t st) {
    const uint32_t tiles = sweep_tiles(S, pods);
    if (!tiles) return;
    if (pods) hipLaunchKernelGGL(k_sweep_count<true>, dim3(tiles), dim3(SW_THREADS), 0, st, S, seen, tiles_per_bucket(S), tile_cnt);
    else hipLaunchKernelGGL(k_sweep_count<false>, dim3(tiles), dim3(SW_THREADS), 0, st, S, seen, 1u, tile_cnt);
}
void launch_sweep_emit(const DevState& S, int pods, const uint8_t* seen, const uint32_t* tile_base, uint32_t n_out, void* recs,
                       int32_t* handles, int32_t* nodes, hipStream_t st) {
    const uint32_t tiles = sweep_tiles(S, pods);
    if (!tiles || !n_out) return;
    if (pods)
        hipLaunchKernelGGL(k_sweep_emit<true>, dim3(tiles), dim3(SW_THREADS), 0, st, S, seen, tiles_per_bucket(S), tile_base, n_out,
                           recs, handles, nodes);
    else
        hipLaunchKernelGGL(k_sweep_emit<false>, dim3(tiles), dim3(SW_THREADS), 0, st, S, seen, 1u, tile_base, n_out, recs, handles,
                           nodes);
}

}  // namespace kwok
