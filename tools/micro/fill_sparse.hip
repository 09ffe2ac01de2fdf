// Microbenchmark: rewriting only the dirty pieces of the 1M-node heartbeat
// stream (1M x 1072-byte records, the 4-slot-group walk of fill_hbm.hip).  Two
// ticks of one arena differ in one or two characters per Now timestamp; the
// dirty pieces of a group are the same for every group, so the pass stores the
// (group, dirty piece) items only, at three granularities:
//   u16   the dirty 16-byte units                       (4-slot groups)
//   l64   the whole aligned 64-byte lines they touch    (4-slot groups = 67 lines)
//   l128  the whole aligned 128-byte lines they touch   (8-slot groups = 67 lines)
// each with plain and non-temporal stores at 1 and 2 blocks of 256 per CU, for
// the two dirty sets the benchmark's 30 s steps produce (the Now offsets come
// from the default heartbeat template):
//   set 0  one changed byte per Now value (tens of seconds)
//   set 1  two changed bytes per Now value (minute carry: minutes and tens of seconds)
// The passes alternate between two regions, as the engine's two tick slots do.
// The full fill (fill_hbm's grp-nt) runs first as the yardstick, with its spread.
// Last, the l64 pass once more with every cache-policy form of the 16-byte vector
// store (global_store_dwordx4 with nt / sc0 / sc1 in each combination; sc0 sc1 is
// the write-through, system-scope form), plain and nt among them as the run's own
// reference.  After those, the l64 pass with an address-determined share of the
// groups stored plain and the rest nt ("mixed k/64": group g plain iff
// (g & 63) < k), on two alternating regions and on one, next to the plain nt
// pass on each.
// Every row has two timings: one event pair per pass with a synchronise between
// passes, and "steady", one event pair around 24 passes back to back (per pass),
// which is how queued ticks run.
// usage: fill_sparse [n_hb] [--pmc]   (--pmc: 3 passes per variant and no timing,
// for rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE; the variant is in the kernel name)
// build: hipcc --offload-arch=gfx950 -O3 -I kwok_amd/csrc tools/micro/fill_sparse.hip
//        kwok_amd/csrc/templates.cpp kwok_amd/csrc/gotemplate.cpp -o tools/micro/fill_sparse
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "templates.h"
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t U = 67;       // 16-byte units per body
constexpr uint32_t MAX_E = 8 * U;  // dirty units of a group at most

template <int NT>
__global__ void k_full(u32x4* dst, uint64_t n_hb) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    u32x4 r[5];
#pragma unroll
    for (int k = 0; k < 5; k++) r[k] = u32x4{(uint32_t)((64 * k + l) % 67), 1u, 2u, 3u};
    const uint64_t ng = n_hb / 4, g0 = ng * blockIdx.x / gridDim.x, g1 = ng * (blockIdx.x + 1) / gridDim.x;
    for (uint64_t g = g0 + w; g < g1; g += nw) {
        u32x4* p = dst + g * 268 + l;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (NT) __builtin_nontemporal_store(r[k], p + 64 * k);
            else p[64 * k] = r[k];
        }
        if (l < 12) {
            if (NT) __builtin_nontemporal_store(r[4], p + 256);
            else p[256] = r[4];
        }
    }
}

// el: the n_e dirty unit offsets of a group of GS slots, ascending.  Lane x of
// the block's flat walk stores item x = (group, el[x % n_e]): every lane has a
// store whatever n_e is.  P / SET / BPC only name the variant for the profiler.
template <int NT, int P, int SET, int BPC>
__global__ __launch_bounds__(256) void k_sparse(u32x4* dst, uint64_t n_hb, uint32_t GS, const uint16_t* el_g, uint32_t n_e) {
    __shared__ uint16_t el[MAX_E];
    __shared__ u32x4 tmpl[U];
    for (uint32_t i = threadIdx.x; i < n_e; i += blockDim.x) el[i] = el_g[i];
    for (uint32_t i = threadIdx.x; i < U; i += blockDim.x) tmpl[i] = u32x4{i, 1u, 2u, 3u};
    __syncthreads();
    if (!n_e) return;
    const uint64_t units = n_hb * U, GU = (uint64_t)GS * U;
    const uint64_t ng = (n_hb + GS - 1) / GS, g0 = ng * blockIdx.x / gridDim.x, g1 = ng * (blockIdx.x + 1) / gridDim.x;
    const uint32_t step = blockDim.x, dg = step / n_e, dr = step % n_e;
    uint64_t g = g0 + threadIdx.x / n_e;
    uint32_t r = threadIdx.x % n_e;
    while (g < g1) {
        const uint32_t u = el[r];
        const uint64_t i = g * GU + u;
        if (i < units) {
            if (NT) __builtin_nontemporal_store(tmpl[u % U], dst + i);
            else dst[i] = tmpl[u % U];
        }
        g += dg;
        r += dr;
        if (r >= n_e) r -= n_e, g++;
    }
}

// k_sparse's l64 walk with the policy a function of the group's address alone:
// group g is resident iff (g & 63) < keep and is stored plain, every other group
// non-temporal.  keep 0 is the nt pass, keep 64 the plain one.
template <int SET, int BPC>
__global__ __launch_bounds__(256) void k_mixed(u32x4* dst, uint64_t n_hb, uint32_t GS, const uint16_t* el_g, uint32_t n_e, uint32_t keep) {
    __shared__ uint16_t el[MAX_E];
    __shared__ u32x4 tmpl[U];
    for (uint32_t i = threadIdx.x; i < n_e; i += blockDim.x) el[i] = el_g[i];
    for (uint32_t i = threadIdx.x; i < U; i += blockDim.x) tmpl[i] = u32x4{i, 1u, 2u, 3u};
    __syncthreads();
    if (!n_e) return;
    const uint64_t units = n_hb * U, GU = (uint64_t)GS * U;
    const uint64_t ng = (n_hb + GS - 1) / GS, g0 = ng * blockIdx.x / gridDim.x, g1 = ng * (blockIdx.x + 1) / gridDim.x;
    const uint32_t step = blockDim.x, dg = step / n_e, dr = step % n_e;
    uint64_t g = g0 + threadIdx.x / n_e;
    uint32_t r = threadIdx.x % n_e;
    while (g < g1) {
        const uint32_t u = el[r];
        const uint64_t i = g * GU + u;
        if (i < units) {
            // spelled as instructions: written as two C++ stores under one
            // condition, the compiler merges them into a single plain store
            const u32x4 v = tmpl[u % U];
            if (((uint32_t)g & 63u) < keep) asm volatile("global_store_dwordx4 %0, %1, off" ::"v"(dst + i), "v"(v) : "memory");
            else asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(dst + i), "v"(v) : "memory");
        }
        g += dg;
        r += dr;
        if (r >= n_e) r -= n_e, g++;
    }
}

// k_sparse's l64 walk with the store's cache policy spelled out: POL bit 0 nt, bit 1 sc0, bit 2 sc1
template <int POL>
__device__ __forceinline__ void store_pol(u32x4* p, u32x4 v) {
    if (POL == 0) asm volatile("global_store_dwordx4 %0, %1, off" ::"v"(p), "v"(v) : "memory");
    if (POL == 1) asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(p), "v"(v) : "memory");
    if (POL == 2) asm volatile("global_store_dwordx4 %0, %1, off sc0" ::"v"(p), "v"(v) : "memory");
    if (POL == 3) asm volatile("global_store_dwordx4 %0, %1, off sc0 nt" ::"v"(p), "v"(v) : "memory");
    if (POL == 4) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
    if (POL == 5) asm volatile("global_store_dwordx4 %0, %1, off sc1 nt" ::"v"(p), "v"(v) : "memory");
    if (POL == 6) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(p), "v"(v) : "memory");
    if (POL == 7) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1 nt" ::"v"(p), "v"(v) : "memory");
}
template <int POL, int SET, int BPC>
__global__ __launch_bounds__(256) void k_sparse_pol(u32x4* dst, uint64_t n_hb, uint32_t GS, const uint16_t* el_g, uint32_t n_e) {
    __shared__ uint16_t el[MAX_E];
    __shared__ u32x4 tmpl[U];
    for (uint32_t i = threadIdx.x; i < n_e; i += blockDim.x) el[i] = el_g[i];
    for (uint32_t i = threadIdx.x; i < U; i += blockDim.x) tmpl[i] = u32x4{i, 1u, 2u, 3u};
    __syncthreads();
    if (!n_e) return;
    const uint64_t units = n_hb * U, GU = (uint64_t)GS * U;
    const uint64_t ng = (n_hb + GS - 1) / GS, g0 = ng * blockIdx.x / gridDim.x, g1 = ng * (blockIdx.x + 1) / gridDim.x;
    const uint32_t step = blockDim.x, dg = step / n_e, dr = step % n_e;
    uint64_t g = g0 + threadIdx.x / n_e;
    uint32_t r = threadIdx.x % n_e;
    while (g < g1) {
        const uint32_t u = el[r];
        const uint64_t i = g * GU + u;
        if (i < units) store_pol<POL>(dst + i, tmpl[u % U]);
        g += dg;
        r += dr;
        if (r >= n_e) r -= n_e, g++;
    }
}

typedef void (*sparse_fn)(u32x4*, uint64_t, uint32_t, const uint16_t*, uint32_t);
template <int POL>
static sparse_fn pick_pol(int set, int bpc) {
    return set == 0 ? (bpc == 1 ? k_sparse_pol<POL, 0, 1> : k_sparse_pol<POL, 0, 2>)
                    : (bpc == 1 ? k_sparse_pol<POL, 1, 1> : k_sparse_pol<POL, 1, 2>);
}
template <int NT, int P, int SET>
static sparse_fn pick_bpc(int bpc) {
    return bpc == 1 ? k_sparse<NT, P, SET, 1> : k_sparse<NT, P, SET, 2>;
}
template <int NT, int P>
static sparse_fn pick_set(int set, int bpc) {
    return set == 0 ? pick_bpc<NT, P, 0>(bpc) : pick_bpc<NT, P, 1>(bpc);
}
template <int NT>
static sparse_fn pick_p(int p, int set, int bpc) {
    return p == 1 ? pick_set<NT, 1>(set, bpc) : p == 4 ? pick_set<NT, 4>(set, bpc) : pick_set<NT, 8>(set, bpc);
}

int main(int argc, char** argv) {
    uint64_t n_hb = 1000000;
    bool pmc = false;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--pmc")) pmc = true;
        else n_hb = strtoull(argv[i], 0, 10);
    }
    const kwok::HeartbeatTemplate hb = kwok::build_heartbeat_template();
    if ((hb.bytes.size() + 15) / 16 != U) return fprintf(stderr, "default template: %zu bytes\n", hb.bytes.size()), 1;
    // "YYYY-MM-DDTHH:MM:SSZ": tens of seconds at 17, minutes at 15
    bool dirty[2][U] = {};
    for (uint16_t o : hb.now_slots) {
        dirty[0][(o + 17) / 16] = dirty[1][(o + 17) / 16] = true;
        dirty[1][(o + 15) / 16] = true;
    }
    printf("Now slots at");
    for (uint16_t o : hb.now_slots) printf(" %u", o);
    printf("; dirty units of a body: set 0 %d, set 1 %d of %u\n", (int)std::count(dirty[0], dirty[0] + U, true),
           (int)std::count(dirty[1], dirty[1] + U, true), U);
    u32x4* dst[2];
    uint16_t* el_d;
    if (hipMalloc(&dst[0], n_hb * 1072 + 4096) != hipSuccess || hipMalloc(&dst[1], n_hb * 1072 + 4096) != hipSuccess ||
        hipMalloc(&el_d, MAX_E * 2) != hipSuccess)
        return 1;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
    printf("n_hb %llu (%.1f MB per region, two regions alternating), %d CUs, blocks of 256\n", (unsigned long long)n_hb,
           n_hb * 1072 / 1e6, cus);
    int pass = 0, regions = 2;  // regions 1: every pass rewrites dst[0] (one tick slot)
    constexpr int STEADY_PASSES = 24, STEADY_REPEATS = 6;
    auto measure = [&](const char* name, double bytes, auto&& launch) {
        if (pmc) {
            for (int r = 0; r < 3; r++) launch(dst[pass++ & (regions - 1)]);
            (void)hipDeviceSynchronize();
            printf("%s: %.1f MB stored per pass\n", name, bytes / 1e6);
            return;
        }
        for (int w = 0; w < 4; w++) launch(dst[pass++ & (regions - 1)]);
        (void)hipDeviceSynchronize();
        float best = 1e9, worst = 0, sum = 0;
        for (int r = 0; r < 10; r++) {
            (void)hipEventRecord(e0);
            launch(dst[pass++ & (regions - 1)]);
            (void)hipEventRecord(e1);
            (void)hipEventSynchronize(e1);
            float ms;
            (void)hipEventElapsedTime(&ms, e0, e1);
            best = std::min(best, ms), worst = std::max(worst, ms), sum += ms;
        }
        // steady: the passes back to back in one event pair, as queued ticks run;
        // the memory side does not drain between them
        float sbest = 1e9, sworst = 0, ssum = 0;
        for (int r = 0; r < STEADY_REPEATS; r++) {
            (void)hipEventRecord(e0);
            for (int p = 0; p < STEADY_PASSES; p++) launch(dst[pass++ & (regions - 1)]);
            (void)hipEventRecord(e1);
            (void)hipEventSynchronize(e1);
            float ms;
            (void)hipEventElapsedTime(&ms, e0, e1);
            ms /= STEADY_PASSES;
            sbest = std::min(sbest, ms), sworst = std::max(sworst, ms), ssum += ms;
        }
        printf("%-28s %7.1f MB/pass: best %7.1f mean %7.1f worst %7.1f us -> %.2f TB/s stored (best); steady best %7.1f mean %7.1f worst %7.1f us\n",
               name, bytes / 1e6, best * 1e3, sum * 1e2, worst * 1e3, bytes / (best * 1e-3) / 1e12, sbest * 1e3,
               ssum * 1e3 / STEADY_REPEATS, sworst * 1e3);
    };
    // both regions hold bodies before any sparse pass (and the yardstick: the full stream)
    for (int bpc : {1, 2}) {
        char name[64];
        snprintf(name, sizeof name, "full-nt b/CU %d", bpc);
        measure(name, (double)(n_hb / 4 * 4) * 1072, [&](u32x4* d) { hipLaunchKernelGGL(k_full<1>, dim3(cus * bpc), dim3(256), 0, 0, d, n_hb); });
        snprintf(name, sizeof name, "full-plain b/CU %d", bpc);
        measure(name, (double)(n_hb / 4 * 4) * 1072, [&](u32x4* d) { hipLaunchKernelGGL(k_full<0>, dim3(cus * bpc), dim3(256), 0, 0, d, n_hb); });
    }
    for (int set = 0; set < 2; set++)
        for (int P : {1, 4, 8}) {
            const uint32_t GS = P == 8 ? 8 : 4, GU = GS * U;
            std::vector<uint16_t> el;
            for (uint32_t p0 = 0; p0 < GU; p0 += P) {
                bool d = false;
                for (uint32_t u = p0; u < p0 + P; u++) d |= dirty[set][u % U];
                if (d)
                    for (uint32_t u = p0; u < p0 + P; u++) el.push_back((uint16_t)u);
            }
            if (hipMemcpy(el_d, el.data(), el.size() * 2, hipMemcpyHostToDevice) != hipSuccess) return 1;
            const double bytes = (double)((n_hb + GS - 1) / GS) * el.size() * 16;
            for (int nt : {0, 1})
                for (int bpc : {1, 2}) {
                    char name[64];
                    snprintf(name, sizeof name, "set %d %s %s b/CU %d", set, P == 1 ? "u16" : P == 4 ? "l64" : "l128",
                             nt ? "nt" : "plain", bpc);
                    sparse_fn fn = nt ? pick_p<1>(P, set, bpc) : pick_p<0>(P, set, bpc);
                    measure(name, bytes, [&](u32x4* d) {
                        hipLaunchKernelGGL(fn, dim3(cus * bpc), dim3(256), 0, 0, d, n_hb, GS, el_d, (uint32_t)el.size());
                    });
                }
        }
    // the l64 pass under every cache-policy form of the vector store
    static const char* pol_name[8] = {"plain", "nt", "sc0", "sc0 nt", "sc1", "sc1 nt", "sc0 sc1", "sc0 sc1 nt"};
    for (int set = 0; set < 2; set++) {
        const uint32_t GS = 4, GU = GS * U;
        std::vector<uint16_t> el;
        for (uint32_t p0 = 0; p0 < GU; p0 += 4) {
            bool d = false;
            for (uint32_t u = p0; u < p0 + 4; u++) d |= dirty[set][u % U];
            if (d)
                for (uint32_t u = p0; u < p0 + 4; u++) el.push_back((uint16_t)u);
        }
        if (hipMemcpy(el_d, el.data(), el.size() * 2, hipMemcpyHostToDevice) != hipSuccess) return 1;
        const double bytes = (double)((n_hb + GS - 1) / GS) * el.size() * 16;
        for (int pol = 0; pol < 8; pol++)
            for (int bpc : {1, 2}) {
                char name[64];
                snprintf(name, sizeof name, "set %d l64 [%s] b/CU %d", set, pol_name[pol], bpc);
                sparse_fn fn = pol == 0 ? pick_pol<0>(set, bpc) : pol == 1 ? pick_pol<1>(set, bpc) : pol == 2 ? pick_pol<2>(set, bpc)
                             : pol == 3 ? pick_pol<3>(set, bpc) : pol == 4 ? pick_pol<4>(set, bpc) : pol == 5 ? pick_pol<5>(set, bpc)
                             : pol == 6 ? pick_pol<6>(set, bpc) : pick_pol<7>(set, bpc);
                measure(name, bytes, [&](u32x4* d) {
                    hipLaunchKernelGGL(fn, dim3(cus * bpc), dim3(256), 0, 0, d, n_hb, GS, el_d, (uint32_t)el.size());
                });
            }
    }
    // the l64 pass with k of every 64 groups stored plain (resident on die if the
    // cache keeps them), the rest nt: two regions alternating (two tick slots) and
    // one region (blocking ticks); k 0 is the nt pass and the row to beat.  The
    // sweep runs twice, so a drift of the machine shows as a difference of rounds.
    for (int round = 0; round < 2; round++)
        for (regions = 2; regions >= 1; regions--)
            for (int set = 0; set < 2; set++) {
                const uint32_t GS = 4, GU = GS * U;
                std::vector<uint16_t> el;
                for (uint32_t p0 = 0; p0 < GU; p0 += 4) {
                    bool d = false;
                    for (uint32_t u = p0; u < p0 + 4; u++) d |= dirty[set][u % U];
                    if (d)
                        for (uint32_t u = p0; u < p0 + 4; u++) el.push_back((uint16_t)u);
                }
                if (hipMemcpy(el_d, el.data(), el.size() * 2, hipMemcpyHostToDevice) != hipSuccess) return 1;
                const double bytes = (double)((n_hb + GS - 1) / GS) * el.size() * 16;
                if (round == 0) {
                    char name[64];
                    snprintf(name, sizeof name, "set %d l64 nt %dreg b/CU 2", set, regions);
                    sparse_fn fn = pick_p<1>(4, set, 2);
                    measure(name, bytes, [&](u32x4* d) {
                        hipLaunchKernelGGL(fn, dim3(cus * 2), dim3(256), 0, 0, d, n_hb, GS, el_d, (uint32_t)el.size());
                    });
                }
                for (uint32_t k : {0u, 8u, 16u, 24u, 32u, 48u, 64u}) {
                    char name[64];
                    snprintf(name, sizeof name, "set %d l64 mixed %2u/64 %dreg r%d", set, k, regions, round);
                    auto fn = set == 0 ? k_mixed<0, 2> : k_mixed<1, 2>;
                    measure(name, bytes, [&](u32x4* d) {
                        hipLaunchKernelGGL(fn, dim3(cus * 2), dim3(256), 0, 0, d, n_hb, GS, el_d, (uint32_t)el.size(), k);
                    });
                }
            }
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
