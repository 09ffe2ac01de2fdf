// engine.cpp - host runtime behind include/kwok_engine.h.
//
// Owns one GPU: device SoA state, the output arena, the replicated ipPool
// bitmaps and (multi-rank) an RCCL communicator.  Host-side it keeps only what
// the slot policy needs (names -> node slots, slot occupancy, refcounts); all
// per-object status lives in HBM and is advanced by the kernels of one tick.
//
// Reference interfaces replaced (hezhizhen/kwok, pkg/kwok/controllers):
//   NewController / NewNodeController / NewPodController  controller.go:80-152,
//                                                          node_controller.go:79-117, pod_controller.go:84-128
//   WatchNodes/ListNodes, WatchPods/ListPods event switch node_controller.go:256-295, pod_controller.go:301-367
//   ipPool                                                utils.go:52-117
//
// The tick queue (output slots and arena, enqueue / retire, submit / collect) is engine_tick.cpp;
// engine_state.h holds the state both files work on.
#include "../../include/kwok_response.h"
#include "engine_state.h"
#include "node_spans.h"


namespace {

// FNV-1a 64 of a pod spec's strings (json.hip spec_key is the same function):
// each container's name 0x1F image 0x1E, 0x1D, the init containers alike, 0x1D,
// each readiness gate 0x1E
// The canonical byte string the key hashes; the GPU codec compares a document's
// spec with it after a table hit (the key alone is not collision-resistant)
std::string json_spec_canon(const std::vector<Container>& cs, const std::vector<Container>& ics,
                            const std::vector<std::string>& gates) {
    std::string o;
    for (auto& c : cs) o += c.name, o += '\x1F', o += c.image, o += '\x1E';
    o += '\x1D';
    for (auto& c : ics) o += c.name, o += '\x1F', o += c.image, o += '\x1E';
    o += '\x1D';
    for (auto& g : gates) o += g, o += '\x1E';
    return o;
}
// KWOK_DEBUG_SPEC_KEY_BITS=b (tests): keys cut to their low b bits, so that
// distinct specs collide and the device's byte check decides
uint64_t spec_key_mask() {  // (read per call: registrations and decode launches are rare)
    const char* v = getenv("KWOK_DEBUG_SPEC_KEY_BITS");
    const unsigned b = v ? (unsigned)atoi(v) : 64u;
    return b >= 64 || b == 0 ? ~0ull : (1ull << b) - 1ull;
}
uint64_t json_spec_key(const std::string& canon) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (unsigned char c : canon) h = (h ^ c) * 0x100000001B3ull;
    return h & spec_key_mask();
}
uint64_t json_spec_key(const std::vector<Container>& cs, const std::vector<Container>& ics,
                       const std::vector<std::string>& gates) {
    return json_spec_key(json_spec_canon(cs, ics, gates));
}

thread_local std::string g_create_err;  // kwok_last_error(NULL) after a failed create

uint32_t fnv1a32(const char* s, size_t n) {
    uint32_t h = 0x811C9DC5u;
    for (size_t i = 0; i < n; i++) {
        h ^= (unsigned char)s[i];
        h *= 0x01000193u;
    }
    return h;
}

}  // namespace

namespace {

// kwok_host_alloc buffers (base -> length, device address, mmap'd + registered)
struct HostReg {
    size_t len;
    uint8_t* dev;
    bool mmapped;
};
std::mutex g_host_mu;
std::map<uintptr_t, HostReg> g_host_reg;
// the device address of [p, p + n) when it lies inside one kwok_host_alloc
// buffer (kernels read it in place over the link), else null
const void* host_mapped(const void* p, size_t n) {
    const uintptr_t a = (uintptr_t)p;
    std::lock_guard<std::mutex> l(g_host_mu);
    auto it = g_host_reg.upper_bound(a);
    if (it == g_host_reg.begin()) return nullptr;
    --it;
    const HostReg& r = it->second;
    if (!r.dev || a + n > it->first + r.len) return nullptr;
    return r.dev + (a - it->first);
}

}  // namespace

int kwok::DevGroup::reserve(kwok_engine* e, size_t need, size_t want) {
    if (need <= cap) return KWOK_OK;
    release();
    const size_t c = std::max(want, floor_);
    for (auto& m : m_)
        if (int rc = dalloc(e, (uint8_t**)m.p, std::max<size_t>(m.count ? m.count(c) : c, 1) * m.elem)) return rc;
    cap = c;
    return KWOK_OK;
}

namespace {

int ensure_pinned(kwok_engine* e, size_t bytes) {
    if (bytes <= e->pinned_cap) return KWOK_OK;
    if (e->pinned) (void)hipHostFree(e->pinned);
    e->pinned_cap = std::max(bytes, e->pinned_cap * 2);
    if (hipHostMalloc(&e->pinned, e->pinned_cap, hipHostMallocDefault) != hipSuccess)
        return e->fail(KWOK_ENOMEM, "pinned %zu", e->pinned_cap);
    if (e->d_ops_cap < e->pinned_cap) {
        if (e->d_ops) (void)hipFree(e->d_ops);
        e->d_ops_cap = e->pinned_cap;
        if (hipMalloc(&e->d_ops, e->d_ops_cap) != hipSuccess) return e->fail(KWOK_ENOMEM, "ops %zu", e->d_ops_cap);
    }
    return KWOK_OK;
}


// Run f(p) for every ingest partition p: on n_part host threads when the batch
// is large enough to pay for them, else in order on the caller's thread.
template <class F>
void run_parts(kwok_engine* e, bool parallel, F&& f) {
    if (!parallel || e->n_part == 1) {
        for (int p = 0; p < e->n_part; p++) f(p);
        return;
    }
    const std::function<void(int)> fn = [&f](int p) { f(p); };
    e->workers.run(e->n_part, fn);
}
constexpr size_t NODE_PAR_MIN = 2048;  // node records (the per-record work is heavier)

// kwok_pool_put's staged releases -> one host-to-device copy -> the pool
int flush_ops(kwok_engine* e) {
    const size_t nu = e->puts.size();
    if (!nu) return KWOK_OK;
    if (int rc = ensure_pinned(e, nu * 4 + 256)) return rc;
    memcpy(e->pinned, e->puts.data(), nu * 4);
    HIPCHK(e, hipMemcpyAsync(e->d_ops, e->pinned, nu * 4, hipMemcpyHostToDevice, e->st));
    // ingest-time releases of other ranks (pod_controller.go:329-336)
    launch_pool_puts_now(e->S, (const uint32_t*)e->d_ops, (uint32_t)nu, e->st);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->st));
    e->puts.clear();
    return KWOK_OK;
}

int upload_specs(kwok_engine* e) {
    int rc;
    if ((rc = dgrow(e, e->d_specs, e->specs_h.size()))) return rc;
    // the kernels read the spec bytes as 32-bit words, up to SRC_PAD_FRONT bytes
    // before a segment and SRC_PAD_BACK past the end
    std::string bytes(SRC_PAD_FRONT, '\0');
    bytes += e->spec_bytes_h;
    bytes.resize(((bytes.size() + 3) & ~(size_t)3) + SRC_PAD_BACK, '\0');
    if ((rc = dgrow(e, e->d_spec_bytes, bytes.size()))) return rc;
    if ((rc = dgrow(e, e->d_spec_nxt, std::max<size_t>(e->spec_nxt_h.size(), 1)))) return rc;
    HIPCHK(e, hipMemcpyAsync(e->d_specs.p, e->specs_h.data(), e->specs_h.size() * sizeof(SpecDesc),
                             hipMemcpyHostToDevice, e->st));
    HIPCHK(e, hipMemcpyAsync(e->d_spec_bytes.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, e->st));
    if (!e->spec_nxt_h.empty())
        HIPCHK(e, hipMemcpyAsync(e->d_spec_nxt.p, e->spec_nxt_h.data(), e->spec_nxt_h.size() * 2, hipMemcpyHostToDevice, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    e->S.specs = e->d_specs.p;
    e->S.spec_bytes = e->d_spec_bytes.p + SRC_PAD_FRONT;
    e->S.spec_nxt = e->d_spec_nxt.p;
    e->S.nxt_total = (uint32_t)e->spec_nxt_h.size();
    e->S.n_specs = (uint32_t)e->specs_h.size();
    e->S.spec_total = (uint32_t)e->spec_bytes_h.size();
    return KWOK_OK;
}

}  // namespace

namespace kwok {
int poisoned(kwok_engine* e) {
    return e->fail(KWOK_EDEVICE, "a failed tick left the engine out of step with the device: destroy it and "
                                 "recreate it (re-ingest by List)");
}
}  // namespace kwok

namespace {

uint64_t intern_blob(kwok_engine* e, const NodeBlob& b, int* rc) {
    std::string key = b.pre + '\x01' + b.post;
    auto it = e->blob_ids.find(key);
    if (it != e->blob_ids.end()) return it->second;
    // k_emit keeps patch positions in 16 bits
    if (b.pre.size() + e->hb_tpl.conds_len + b.post.size() > 0xFFF0 || e->blob_h.size() > 0xFFFFFFFFull - 0x20000) {
        *rc = KWOK_EDOMAIN;
        return 0;
    }
    uint64_t off = e->blob_h.size();
    e->blob_h += b.pre;
    e->blob_h += b.post;
    uint64_t word = off | ((uint64_t)b.pre.size() << 32) | ((uint64_t)b.post.size() << 48);
    e->blob_ids.emplace(key, word);
    uint32_t ilen = (uint32_t)b.pre.size() + e->hb_tpl.conds_len + (uint32_t)b.post.size();
    e->max_init_len = std::max(e->max_init_len, ilen);
    e->blob_up_lo = std::min<size_t>(e->blob_up_lo, off);  // uploaded once per batch (upload_blobs)
    return word;
}

// The blobs interned since the last upload -> the device copy (SRC_PAD_FRONT
// zero bytes, the blobs, SRC_PAD_BACK zero bytes: k_emit reads around them).
// Once per node batch, after every ingest thread is done appending to blob_h,
// and synchronised before return: blob_h (pageable) may grow at the next batch.
int upload_blobs(kwok_engine* e) {
    if (e->blob_up_lo >= e->blob_h.size()) return KWOK_OK;
    const size_t lo = e->blob_up_lo;
    const size_t padded = ((SRC_PAD_FRONT + e->blob_h.size() + 3) & ~(size_t)3) + SRC_PAD_BACK;
    if (padded > e->d_blob.n) {
        uint8_t* p = nullptr;
        const size_t cap = std::max<size_t>(padded, 2 * e->d_blob.n);
        if (hipMalloc((void**)&p, cap) != hipSuccess) return e->fail(KWOK_ENOMEM, "blob %zu", cap);
        HIPCHK(e, hipMemsetAsync(p, 0, cap, e->st));
        if (e->d_blob.p) HIPCHK(e, hipMemcpyAsync(p, e->d_blob.p, SRC_PAD_FRONT + lo, hipMemcpyDeviceToDevice, e->st));
        HIPCHK(e, hipStreamSynchronize(e->st));
        if (e->d_blob.p) (void)hipFree(e->d_blob.p);
        e->d_blob.p = p;
        e->d_blob.n = cap;
    }
    HIPCHK(e, hipMemcpyAsync(e->d_blob.p + SRC_PAD_FRONT + lo, e->blob_h.data() + lo, e->blob_h.size() - lo,
                             hipMemcpyHostToDevice, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    e->blob_up_lo = SIZE_MAX;
    e->S.blob = e->d_blob.p + SRC_PAD_FRONT;
    e->S.blob_total = (uint32_t)e->blob_h.size();
    return KWOK_OK;
}

bool node_conforms(const kwok_node_event& ev, const std::string info[10]) {
    // A.5: configureNode's merged status equals the original iff no default applies
    return ev.addresses.len && ev.allocatable.len && ev.capacity.len && ev.phase == KWOK_PHASE_RUNNING &&
           !info[KWOK_NI_ARCHITECTURE].empty() && !info[KWOK_NI_KUBE_PROXY_VERSION].empty() &&
           !info[KWOK_NI_KUBELET_VERSION].empty() && !info[KWOK_NI_OPERATING_SYSTEM].empty() &&
           info[KWOK_NI_SYSTEM_UUID] == info[KWOK_NI_OS_IMAGE];
}

int parse_opt_ip(const char* arena, kwok_str s, uint32_t* ip) {
    *ip = 0;
    if (!s.len) return KWOK_OK;
    if (!parse_ipv4(arena + s.off, s.len, ip) || *ip == 0) return KWOK_EDOMAIN;
    return KWOK_OK;
}

}  // namespace

namespace kwok {
int exchange(kwok_engine* e, void* send, size_t bytes, void* recv) {
    if (e->comm) {
        ncclResult_t r = ncclAllGather(send, recv, bytes, ncclUint8, e->comm, e->st);
        if (r != ncclSuccess) return e->fail(KWOK_ECOMM, "ncclAllGather: %s", ncclGetErrorString(r));
        return KWOK_OK;
    }
    // host-memory exchange through the caller's allgather
    std::vector<char> hs(bytes), hr(bytes * e->W);
    if (int rc = release_for_host(e)) return rc;
    HIPCHK(e, hipMemcpyAsync(hs.data(), send, bytes, hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    if (e->cfg.allgather(e->cfg.allgather_user, hs.data(), bytes, hr.data()))
        return e->fail(KWOK_ECOMM, "allgather callback failed");
    HIPCHK(e, hipMemcpyAsync(recv, hr.data(), bytes * e->W, hipMemcpyHostToDevice, e->st));
    return KWOK_OK;
}
}  // namespace kwok

namespace {

// Grow every bucket's pod capacity to new_cp (<= the handle stride): the device
// pod arrays are re-laid out bucket by bucket (a bucket's pods keep their index,
// so handles, canonical order and IP order are unchanged); per-slot lists are
// reallocated.  Runs between ticks (drained), before a batch's apply pass.
int grow_pods(kwok_engine* e, uint32_t new_cp) {
    const uint32_t old = e->Cp, nb = e->nb;
    if (new_cp <= old) return KWOK_OK;
    e->state_changed();  // (the pod rows move)
    hipStream_t st = e->st;
    DevState& S = e->S;
    const size_t PL2 = (size_t)nb * new_cp, PLa2 = PL2 + 16;
    auto relayout = [&](auto*& p) -> int {
        using T = std::remove_reference_t<decltype(*p)>;
        T* q = nullptr;
        if (hipMalloc((void**)&q, PLa2 * sizeof(T)) != hipSuccess) return e->fail(KWOK_ENOMEM, "grow pods");
        HIPCHK(e, hipMemsetAsync(q, 0, PLa2 * sizeof(T), st));
        HIPCHK(e, hipMemcpy2DAsync(q, (size_t)new_cp * sizeof(T), p, (size_t)old * sizeof(T), (size_t)old * sizeof(T), nb,
                                   hipMemcpyDeviceToDevice, st));
        HIPCHK(e, hipStreamSynchronize(st));
        (void)hipFree(p);
        p = q;
        return KWOK_OK;
    };
    auto resize = [&](auto*& p, bool keep) -> int {  // per-ordinal lists: contents kept (the last tick's outputs)
        using T = std::remove_reference_t<decltype(*p)>;
        T* q = nullptr;
        if (hipMalloc((void**)&q, PLa2 * sizeof(T)) != hipSuccess) return e->fail(KWOK_ENOMEM, "grow pod lists");
        HIPCHK(e, hipMemsetAsync(q, 0, PLa2 * sizeof(T), st));
        if (keep && p) HIPCHK(e, hipMemcpyAsync(q, p, e->PLa * sizeof(T), hipMemcpyDeviceToDevice, st));
        HIPCHK(e, hipStreamSynchronize(st));
        if (p) (void)hipFree(p);
        p = q;
        return KWOK_OK;
    };
    int rc = 0;
    if ((rc = relayout(S.pod_state)) || (rc = relayout(S.pod_node)) || (rc = relayout(S.pod_spec)) ||
        (rc = relayout(S.pod_ctime)) || (rc = relayout(S.pod_ip)) || (rc = relayout(S.host_ip)) ||
        (rc = resize(S.alloc_addr, false)) || (rc = resize(S.use_list, false)) || (rc = resize(S.rel_list, false)))
        return rc;
    if (e->resync.pod_seen && (rc = relayout(e->resync.pod_seen.p))) return rc;  // (a growth inside a session keeps the marks)
    // the uid directory's per-slot uids move with their pods (handles are stable; the table is rebuilt
    // to the new size before its next use, uid_ensure)
    if (e->uid.on && ((rc = relayout(e->uid.pod_uid.p)) || (rc = relayout(e->uid.pod_uid_len.p)))) return rc;
    // ... and the reference directory's namespaces and names
    if (e->refs.on && ((rc = relayout(e->refs.pod_ref.p)) || (rc = relayout(e->refs.pod_ref_len.p)))) return rc;
    for (auto& T : e->slots) {
        if (!T.alloc) continue;
        if ((rc = resize(T.pp_pods, true)) || (rc = resize(T.pp_off, true)) || (rc = resize(T.pp_len, true)) ||
            (rc = resize(T.del_pods, true)) || (rc = resize(T.del_fin, true)) || (rc = resize(T.pp_job, true)))
            return rc;
    }
    e->Cp = new_cp;
    e->PL = (uint32_t)PL2;
    e->PLa = PLa2;
    S.cp = new_cp;
    S.n_pod_slots = e->PL;
    return size_arena(e);
}

// ---- GPU pod ingest: host side -------------------------------------------------
uint32_t sort_bits(const kwok_engine* e) {  // sort keys are local buckets 0..nb (nb: nothing to apply)
    uint32_t b = 1;
    while ((1ull << b) <= e->nb) b++;
    return b;
}
// per-record device buffers for batches of n records (grown with headroom)
int ingest_reserve(kwok_engine* e, size_t n, size_t arena_len) {
    auto& G = e->ing;
    int rc = G.recs.reserve(e, n);
    G.sort_bytes = G.recs.cap ? G.sort_need(G.recs.cap) : 0;
    if (rc) return rc;
    if ((rc = G.arena.reserve(e, arena_len))) return rc;
    return KWOK_OK;
}
IngestBatch ingest_batch(kwok_engine* e, uint32_t n, size_t arena_len) {
    auto& G = e->ing;
    IngestBatch I{};
    I.ev = G.d_ev;
    I.n = n;
    I.n_specs = (uint32_t)e->specs_h.size();
    I.arena = G.arena_src ? G.arena_src : G.d_arena;
    I.arena_len = arena_len;
    I.rec = G.rec;
    I.keys = G.keys;
    I.keys_sorted = G.keys_sorted;
    I.idx_sorted = G.idx_sorted;
    I.out_handle = G.out_handle;
    I.out_status = G.out_status;
    I.out_released = G.out_released;
    I.beg = G.beg;
    I.end = G.end;
    I.sum = G.sum;
    return I;
}
// the batch summary -> pinned host memory (waits for the stream)
int read_summary(kwok_engine* e, const IngSummary* sum = nullptr) {
    if (int rc = release_for_host(e)) return rc;
    HIPCHK(e, hipMemcpyAsync(e->ing.sum_h, sum ? sum : e->ing.sum, sizeof(IngSummary), hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    return KWOK_OK;
}
// The largest pod capacity a chain block's pod chunks cover (engine_create's limit)
uint32_t max_pod_capacity(const kwok_engine* e) {
    const uint64_t bpb = (e->nb + e->S.n_chain - 1) / e->S.n_chain;
    const uint64_t lim = (uint64_t)MAX_POD_CHUNKS * BLOCK * POD_PER_THREAD / bpb;
    return (uint32_t)std::min<uint64_t>(e->Hs, lim & ~7ull);
}

}  // namespace

// ===========================================================================
// C-ABI
// ===========================================================================
extern "C" {

uint32_t kwok_abi_version(void) { return KWOK_ABI_VERSION; }

int kwok_comm_id(uint8_t out[KWOK_COMM_ID_BYTES]) {
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return KWOK_ECOMM;
    static_assert(sizeof(id) <= KWOK_COMM_ID_BYTES, "comm id size");
    memset(out, 0, KWOK_COMM_ID_BYTES);
    memcpy(out, &id, sizeof(id));
    return KWOK_OK;
}

const char* kwok_finalizer_patch(size_t* len) {
    static const char p[] = "{\"metadata\":{\"finalizers\":null}}";  // pod_controller.go:45
    if (len) *len = sizeof(p) - 1;
    return p;
}

uint32_t kwok_bucket_of(const char* name, size_t len, uint32_t buckets) { return fnv1a32(name, len) & (buckets - 1); }

namespace {
thread_local std::string g_tpl_err;
}
const char* kwok_template_last_error(void) { return g_tpl_err.c_str(); }

int kwok_heartbeat_template_patch(const char* tpl, int64_t start_unix, const char* node_ip, int64_t now_unix, char* out,
                                  size_t cap, size_t* out_len) {
    if (!node_ip || !out_len || (cap && !out)) return KWOK_EINVAL;
    g_tpl_err.clear();
    auto rfc3339 = [](int64_t u) {
        time_t t = (time_t)u;
        struct tm tm;
        gmtime_r(&t, &tm);
        char b[32];
        strftime(b, sizeof b, "%Y-%m-%dT%H:%M:%SZ", &tm);
        return std::string(b);
    };
    HeartbeatTemplate hb = build_heartbeat_template();
    if (tpl && !compile_heartbeat_template(tpl, rfc3339(start_unix), node_ip, hb, g_tpl_err)) return KWOK_EDOMAIN;
    const std::string o = heartbeat_patch(hb, rfc3339(now_unix), rfc3339(start_unix));
    *out_len = o.size();
    if (o.size() > cap) return KWOK_EINVAL;
    memcpy(out, o.data(), o.size());
    return KWOK_OK;
}

int kwok_node_template_patch(const char* tpl, const char* heartbeat_tpl, const kwok_node_event* ev, const char* arena,
                             size_t arena_len, int64_t start_unix, const char* node_ip, int64_t now_unix, char* out,
                             size_t cap, size_t* out_len) {
    if (!tpl || !ev || !node_ip || !out_len || (cap && !out)) return KWOK_EINVAL;
    g_tpl_err.clear();
    auto get = [&](kwok_str s) { return (size_t)s.off + s.len <= arena_len ? std::string(arena + s.off, s.len) : std::string(); };
    std::string info[KWOK_NI_COUNT];
    for (int k = 0; k < KWOK_NI_COUNT; k++) info[k] = get(ev->node_info[k]);
    auto rfc3339 = [](int64_t u) {
        time_t t = (time_t)u;
        struct tm tm;
        gmtime_r(&t, &tm);
        char b[32];
        strftime(b, sizeof b, "%Y-%m-%dT%H:%M:%SZ", &tm);
        return std::string(b);
    };
    HeartbeatTemplate hb = build_heartbeat_template();
    if (heartbeat_tpl && !compile_heartbeat_template(heartbeat_tpl, rfc3339(start_unix), node_ip, hb, g_tpl_err))
        return KWOK_EDOMAIN;
    NodeBlob nb;
    if (!compile_node_template(tpl, get(ev->addresses), get(ev->allocatable), get(ev->capacity), info, ev->phase, node_ip,
                               rfc3339(start_unix), hb, nb, g_tpl_err))
        return KWOK_EDOMAIN;
    const std::string o = nb.pre + heartbeat_conditions(hb, rfc3339(now_unix), rfc3339(start_unix)) + nb.post;
    *out_len = o.size();
    if (o.size() > cap) return KWOK_EINVAL;
    memcpy(out, o.data(), o.size());
    return KWOK_OK;
}

int kwok_pod_template_patch(const char* tpl, const kwok_pod_spec* spec, const char* arena, size_t arena_len,
                            int64_t start_unix, const char* node_ip, int64_t creation_unix, uint32_t host_ip,
                            uint32_t pod_ip, int32_t status_nonempty, char* out, size_t cap, size_t* out_len) {
    if (!tpl || !spec || !node_ip || !out_len || (cap && !out)) return KWOK_EINVAL;
    g_tpl_err.clear();
    auto get = [&](kwok_str s) { return (size_t)s.off + s.len <= arena_len ? std::string(arena + s.off, s.len) : std::string(); };
    std::vector<Container> cs, ics;
    std::vector<std::string> gates;
    for (uint32_t i = 0; i < spec->n_containers; i++) cs.push_back({get(spec->containers[i].name), get(spec->containers[i].image)});
    for (uint32_t i = 0; i < spec->n_init_containers; i++)
        ics.push_back({get(spec->init_containers[i].name), get(spec->init_containers[i].image)});
    for (uint32_t i = 0; i < spec->n_readiness_gates; i++) gates.push_back(get(spec->readiness_gates[i]));
    auto rfc3339 = [](int64_t u) {
        time_t t = (time_t)u;
        struct tm tm;
        gmtime_r(&t, &tm);
        char b[32];
        strftime(b, sizeof b, "%Y-%m-%dT%H:%M:%SZ", &tm);
        return std::string(b);
    };
    SpecProgram p;
    if (!compile_pod_template(tpl, cs, ics, gates, rfc3339(start_unix), p, g_tpl_err)) return KWOK_EDOMAIN;
    const std::string ts = rfc3339(creation_unix);
    auto fill = [&](const std::string& seg, const std::string& kind) {
        std::string o = seg;
        for (size_t i = 0; i < o.size(); i++)
            if ((uint8_t)kind[i] != KIND_LIT) o[i] = ts[(uint8_t)kind[i]];
        return o;
    };
    std::string o = fill(p.a, p.ka);
    if (status_nonempty) {  // the kernels' `{{ with .status }}` pieces (k_emit)
        uint32_t nip = 0;
        parse_ipv4(node_ip, strlen(node_ip), &nip);
        o += "\"hostIP\":\"" + format_ipv4(host_ip ? host_ip : nip) + "\",";
        o += fill(p.b, p.kb);
        o += "\"podIP\":\"" + format_ipv4(pod_ip) + "\",";
    } else {
        o += fill(p.b, p.kb);
    }
    o += fill(p.c, p.kc);
    *out_len = o.size();
    if (o.size() > cap) return KWOK_EINVAL;
    memcpy(out, o.data(), o.size());
    return KWOK_OK;
}

int kwok_template_render(const char* tpl, size_t tpl_len, const char* doc, size_t doc_len, const char* funcs,
                         size_t funcs_len, char* out, size_t cap, size_t* out_len) {
    using namespace kwok::gotpl;
    if (!tpl || !doc || !out_len || (cap && !out)) return KWOK_EINVAL;
    g_tpl_err.clear();
    VPtr d, f;
    if (!parse_json(std::string(doc, doc_len), d, g_tpl_err)) return KWOK_EDOMAIN;
    Env env;
    if (funcs && funcs_len) {
        if (!parse_json(std::string(funcs, funcs_len), f, g_tpl_err)) return KWOK_EDOMAIN;
        if (f->kind != Value::MAP) {
            g_tpl_err = "funcs must be a JSON object of strings";
            return KWOK_EINVAL;
        }
        for (auto& kv : f->map) {
            const std::string v = kv.second->s;
            env.funcs[kv.first] = [v] { return v; };
        }
    }
    std::string o;
    if (!render_to_json(std::string(tpl, tpl_len), d, env, o, g_tpl_err)) return KWOK_EDOMAIN;
    *out_len = o.size();
    if (o.size() > cap) return KWOK_EINVAL;
    memcpy(out, o.data(), o.size());
    return KWOK_OK;
}
int32_t kwok_rank_of_bucket(uint32_t bucket, uint32_t buckets, int32_t world) {
    return (int32_t)(((uint64_t)bucket * (uint64_t)world) / buckets);
}

const char* kwok_last_error(const kwok_engine* e) { return e ? e->err.c_str() : g_create_err.c_str(); }

void kwok_engine_destroy(kwok_engine* e) {
    if (!e) return;
    if (e->trace_ticks) {
        static const char* names[TRACE_SLOTS] = {"entry", "nodes-done", "pods-done", "arrived", "reduced", "pool-done",
                                                 "exit", "header-done", "node-flags", "pool-folded", "block-sum",
                                                 "drained", "hb-handles", "share-done", "nodes-emitted", "back-start",
                                                 // tick_back's pool phase (multi rank: the BACK launch)
                                                 "B-entry", "B-records", "B-prepped", "B-scanned", "B-selected",
                                                 "-", "-", "-"};
        fprintf(stderr, "[kwok trace] %u chain + %u streamer blocks, %llu ticks, us after the first chain block "
                        "start (min / median / max block)\n",
                e->S.n_chain, e->n_stream, (unsigned long long)e->trace_ticks);
        for (int k = 0; k < TRACE_SLOTS; k++)
            if (names[k][0] != '-' && e->trace_sum[k][2] > 0)
                fprintf(stderr, "[kwok trace] chain    %-11s %8.2f %8.2f %8.2f\n", names[k],
                        e->trace_sum[k][0] / e->trace_ticks, e->trace_sum[k][1] / e->trace_ticks,
                        e->trace_sum[k][2] / e->trace_ticks);
        for (int k = 0; k < 2; k++)
            fprintf(stderr, "[kwok trace] streamer %-11s %8.2f %8.2f %8.2f\n", k ? "exit" : "entry",
                    e->trace_sum[TRACE_SLOTS + k][0] / e->trace_ticks, e->trace_sum[TRACE_SLOTS + k][1] / e->trace_ticks,
                    e->trace_sum[TRACE_SLOTS + k][2] / e->trace_ticks);
    }
    if (e->st) (void)hipStreamSynchronize(e->st);
    if (e->rst) (void)hipStreamSynchronize(e->rst);  // (asynchronous arena reads)
    for (int i = 0; i < 3; i++) {
        if (e->rsx[i]) (void)hipStreamSynchronize(e->rsx[i]), (void)hipStreamDestroy(e->rsx[i]);
        if (e->rd_part[i]) (void)hipEventDestroy(e->rd_part[i]);
    }
    if (e->rd_go) (void)hipEventDestroy(e->rd_go);
    void* ptrs[] = {e->S.trace, e->S.jtrace, e->S.once_sum, e->S.node_state, e->S.node_blob, e->S.node_tick, e->S.pod_state, e->S.pod_node, e->S.pod_spec,
                    e->S.pod_ctime, e->S.pod_ip, e->S.host_ip, e->S.used_bm, e->S.usable_bm, e->S.pool_index,
                    e->S.pool_blk, e->S.alloc_addr, e->S.rel_bm, e->S.list_counts, (void*)e->S.hb_static,
                    (void*)e->S.hb_kind, e->S.bar, e->S.blockagg, e->S.dmask, e->S.list_blk, e->S.wc_pre, e->S.wc_dirty, e->S.jbase, e->S.gjob, e->d_hb_pre, e->d_hb_bpre, e->S.hdr, e->S.xmsg, e->S.node_key, e->S.node_name, e->S.mb_count, e->S.zb_count,
                    e->S.use_list, e->S.rel_list, e->d_specs.p, e->d_spec_bytes.p, e->d_spec_nxt.p, e->d_unit_tab.p, e->d_unit_desc.p, e->d_blob.p, e->d_ops,
                    e->d_ld, e->d_xall, e->d_xsend, e->d_xrecv, e->d_ssend, e->d_srecv};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    for (auto& T : e->slots) free_slot(T);
    // (the scratch of the ingests, the codec, the framers and the directories owns itself: freed with the engine below)
    auto& g = e->ing;
    void* ip[] = {g.abort, g.sums, g.beg, g.end, g.sum, g.sum1, g.nsum};
    for (void* p : ip)
        if (p) (void)hipFree(p);
    if (g.sum_h) (void)hipHostFree(g.sum_h);
    if (g.nsum_h) (void)hipHostFree(g.nsum_h);
    if (g.sums_h) (void)hipHostFree(g.sums_h);
    hipEvent_t evs[] = {g.go, g.prepped[0], g.prepped[1], g.used[0], g.used[1], g.rdone, g.idone};
    for (hipEvent_t x : evs)
        if (x) (void)hipEventDestroy(x);
    if (e->h_xall) (void)hipHostFree(e->h_xall);
    if (e->pinned) (void)hipHostFree(e->pinned);
    if (e->dump_h) (void)hipHostFree(e->dump_h);
    if (e->comm) ncclCommDestroy(e->comm);
    if (e->d_pod_fill) (void)hipFree(e->d_pod_fill);
    if (e->fence) (void)hipEventDestroy(e->fence);
    // the engine's members free their device and pinned memory here, while the streams still exist
    const hipStream_t streams[] = {g.pst, g.dst, e->rst, e->st};
    delete e;
    for (hipStream_t x : streams)
        if (x) (void)hipStreamDestroy(x);
}

int kwok_engine_create(const kwok_config* cfg, kwok_engine** out) {
    if (!out) return KWOK_EINVAL;
    *out = nullptr;
    if (!cfg || cfg->abi_version != KWOK_ABI_VERSION) return KWOK_EINVAL;
    if ((cfg->custom_templates & ~(KWOK_TPL_POD | KWOK_TPL_NODE_INIT | KWOK_TPL_HEARTBEAT)) || (cfg->flags & ~1u) ||
        ((cfg->custom_templates & KWOK_TPL_POD) && !cfg->pod_status_template) ||
        ((cfg->custom_templates & KWOK_TPL_NODE_INIT) && !cfg->node_init_template) ||
        ((cfg->custom_templates & KWOK_TPL_HEARTBEAT) && !cfg->node_heartbeat_template))
        return KWOK_EINVAL;
    const uint32_t hs = cfg->pod_handle_stride ? cfg->pod_handle_stride : cfg->pod_slots_per_bucket;
    if (!cfg->buckets || (cfg->buckets & (cfg->buckets - 1)) || cfg->node_slots_per_bucket % 4 ||
        !cfg->node_slots_per_bucket || cfg->node_slots_per_bucket > 65536 || cfg->pod_slots_per_bucket % 8 ||
        !cfg->pod_slots_per_bucket || hs % 8 || hs < cfg->pod_slots_per_bucket ||
        hs > 65528 /* fill marks are u16 */ || (uint64_t)cfg->buckets * hs > 0x7FFFFFFFull /* int32 handles */)
        return KWOK_EINVAL;
    int W = cfg->world_size > 0 ? cfg->world_size : 1;
    if (cfg->rank < 0 || cfg->rank >= W || (W > 1 && !cfg->comm_id && !cfg->allgather) || (uint32_t)W > cfg->buckets)
        return KWOK_EINVAL;
    kwok_engine* e = new kwok_engine();
    e->cfg = *cfg;
    e->W = W;
    // KWOK_FORCE_MULTI=1 (tests): one rank through the multi-rank tick, so the exchange
    // (RCCL with comm_id, else the allgather callback) runs on a single GPU
    e->multi = W > 1 || (getenv("KWOK_FORCE_MULTI") && (cfg->comm_id || cfg->allgather));
    e->rank = cfg->rank;
    e->dev = cfg->device;
    e->B = cfg->buckets;
    e->Cn = cfg->node_slots_per_bucket;
    e->Cp = cfg->pod_slots_per_bucket;
    e->Hs = hs;
    e->b_lo = (uint32_t)((uint64_t)cfg->rank * e->B / W);
    e->b_hi = (uint32_t)((uint64_t)(cfg->rank + 1) * e->B / W);
    // kwok_rank_of_bucket must agree with [b_lo, b_hi)
    e->nb = e->b_hi - e->b_lo;
    e->NL = e->nb * e->Cn;
    e->PL = e->nb * e->Cp;
    e->start = cfg->start_time_unix;
    auto bail = [&](int rc) {
        g_create_err = e->err.empty() ? std::string("create failed (") + std::to_string(rc) + ")" : e->err;
        kwok_engine_destroy(e);
        return rc;
    };
    // parseCIDR (utils.go:28-35): keep the host IP of the CIDR string as the pool base
    if (!cfg->cidr || !cfg->node_ip) return bail(KWOK_EINVAL);
    const char* slash = strchr(cfg->cidr, '/');
    uint32_t base = 0;
    if (!slash || !parse_ipv4(cfg->cidr, (size_t)(slash - cfg->cidr), &base)) return bail(KWOK_EDOMAIN);
    int plen = atoi(slash + 1);
    if (plen < 4 || plen > 32) return bail(KWOK_EDOMAIN);  // pool bitmaps: <= 2^28 addresses (32 MiB each)
    uint32_t mask = plen == 32 ? 0xFFFFFFFFu : (uint32_t)(0xFFFFFFFFull << (32 - plen));
    e->pool.net = base & mask;
    e->pool.base = base;
    e->pool.size = 1ull << (32 - plen);
    e->pool.words = (e->pool.size + 63) / 64;
    if (!parse_ipv4(cfg->node_ip, strlen(cfg->node_ip), &e->node_ip) || !e->node_ip) return bail(KWOK_EDOMAIN);
    e->node_ip_s = format_ipv4(e->node_ip);
    if (cfg->start_time_unix < 0 || cfg->start_time_unix > 0xFFFFFFFFll) return bail(KWOK_EDOMAIN);
    {
        time_t t = (time_t)cfg->start_time_unix;
        struct tm tm;
        gmtime_r(&t, &tm);
        char b[32];
        strftime(b, sizeof b, "%Y-%m-%dT%H:%M:%SZ", &tm);  // time.RFC3339 in UTC
        e->start_s = b;
    }
    // the heartbeat template first: its conditions list is part of every node init patch
    e->hb_tpl = build_heartbeat_template();
    if (cfg->custom_templates & KWOK_TPL_HEARTBEAT) {
        e->custom_hb = true;
        e->hb_tpl_text = cfg->node_heartbeat_template;
        std::string why;
        if (!compile_heartbeat_template(e->hb_tpl_text, e->start_s, e->node_ip_s, e->hb_tpl, why))
            return bail(e->fail(KWOK_EDOMAIN, "node heartbeat template: %s", why.c_str()));
    }
    e->hb_len = (uint32_t)e->hb_tpl.bytes.size();
    e->hb_stride = (e->hb_len + 15u) & ~15u;
    if (cfg->custom_templates & KWOK_TPL_NODE_INIT) {
        // compiled per node status at ingest; a trial node rejects a template outside the subset here
        e->custom_node = true;
        e->node_tpl = cfg->node_init_template;
        NodeBlob b;
        std::string why, info[KWOK_NI_COUNT];
        if (!compile_node_template(e->node_tpl, "", "", "", info, KWOK_PHASE_NONE, e->node_ip_s, e->start_s, e->hb_tpl, b,
                                   why))
            return bail(e->fail(KWOK_EDOMAIN, "node initialization template: %s", why.c_str()));
    }
    if (cfg->custom_templates & KWOK_TPL_POD) {
        // compiled per spec at kwok_register_pod_spec; a trial spec rejects a template
        // outside the covered subset here already
        e->custom_pod = true;
        e->pod_tpl = cfg->pod_status_template;
        SpecProgram p;
        std::string why;
        if (!compile_pod_template(e->pod_tpl, {Container{"c", "img"}}, {}, {}, e->start_s, p, why))
            return bail(e->fail(KWOK_EDOMAIN, "pod status template: %s", why.c_str()));
    }

    {
        hipError_t r = hipSetDevice(e->dev);
        if (r != hipSuccess) return bail(e->fail(KWOK_EDEVICE, "hipSetDevice(%d): %s", e->dev, hipGetErrorString(r)));
    }
    {
        hipError_t r = hipStreamCreateWithFlags(&e->st, hipStreamNonBlocking);
        if (r == hipSuccess) r = hipEventCreateWithFlags(&e->fence, hipEventDisableTiming);
        if (r == hipSuccess) r = hipStreamCreateWithFlags(&e->rst, hipStreamNonBlocking);
        if (r != hipSuccess) return bail(e->fail(KWOK_EDEVICE, "stream/event create: %s", hipGetErrorString(r)));
    }
    DevState& S = e->S;
    {
        // k_tick's grid: chain blocks (KWOK_TICK_BLOCKS_PER_CU per CU, default 1)
        // must be co-resident (dirty ticks wait on each other); streamer blocks
        // (KWOK_TICK_STREAMERS_PER_CU, default 1) only stream and exit.  Lower
        // both when several engines share one GPU (their grids must fit together).
        int cus = 0, occ = tick_occupancy(), want = 1, wants = 1;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->dev);
        // heartbeat-once ticks stream one body: the CU's second k_tick slot goes to a
        // second chain block (twice the classification loads in flight), and a few
        // streamer blocks write the body after the chain blocks
        const bool once = (cfg->flags & KWOK_CFG_HEARTBEAT_ONCE) != 0;
        if (once) want = 2;
        if (const char* v = getenv("KWOK_TICK_BLOCKS_PER_CU")) want = std::max(1, atoi(v));
        if (const char* v = getenv("KWOK_TICK_STREAMERS_PER_CU")) wants = std::max(1, atoi(v));
        if (cus <= 0 || occ <= 0) return bail(e->fail(KWOK_EDEVICE, "k_tick occupancy query failed"));
        S.n_chain = std::min<uint32_t>((uint32_t)(cus * std::min(occ, want)), (uint32_t)MAX_CHAIN);
        // KWOK_TICK_CHAIN_BLOCKS: fewer chain blocks, so that the grids of many engines
        // sharing one GPU (the 8-rank C3 test) are co-resident together
        if (const char* v = getenv("KWOK_TICK_CHAIN_BLOCKS")) S.n_chain = std::min<uint32_t>(S.n_chain, (uint32_t)std::max(1, atoi(v)));
        // (heartbeat-once: no streamer blocks - the one body is a chain block's slice,
        // written after its arrival, not by blocks that wait for the chain's CUs)
        e->n_stream = once ? 0u : (uint32_t)(cus * wants);
        // multi rank: the BACK launch fills the CUs' spare k_tick slots with pool-only
        // blocks (the pool phase's word-blocks over more blocks; all co-resident).  Not
        // when several engines share the GPU (KWOK_TICK_BLOCKS_PER_CU / _CHAIN_BLOCKS:
        // their grids must fit together, and a BACK launch waits for all its blocks)
        const bool shared = getenv("KWOK_TICK_BLOCKS_PER_CU") || getenv("KWOK_TICK_CHAIN_BLOCKS");
        S.n_pool_extra = shared ? 0u : (uint32_t)std::min<int64_t>(std::max<int64_t>(0, (int64_t)cus * occ - S.n_chain), e->n_stream);
        if (const char* v = getenv("KWOK_POOL_EXTRA"))
            S.n_pool_extra = (uint32_t)std::min<int64_t>(std::max(0, atoi(v)), std::min<int64_t>((int64_t)cus * occ - S.n_chain, e->n_stream));
        e->emit_grid = (uint32_t)(cus * std::max(1, std::min(emit_occupancy(), 8)));
        if (const char* v = getenv("KWOK_EMIT_BLOCKS_PER_CU")) e->emit_grid = (uint32_t)(cus * std::max(1, std::min(atoi(v), 8)));
        if (const char* v = getenv("KWOK_TICK_STREAMERS")) e->n_stream = e->n_once_stream = (uint32_t)std::max(1, atoi(v));
        if (const char* v = getenv("KWOK_ONCE_STREAMERS")) e->n_once_stream = (uint32_t)std::max(1, atoi(v));
        const char* pr = getenv("KWOK_TICK_PRIO");
        e->chain_prio = pr && pr[0] == '1';
        if (const char* v = getenv("KWOK_TICK_STREAM_DELAY_NS")) S.stream_delay = (uint32_t)std::max(0, atoi(v) / 10);
        if (const char* v = getenv("KWOK_TICK_STREAM_SHARE")) e->share_env = std::min(1024, std::max(0, atoi(v)));
        if (const char* v = getenv("KWOK_HB_NT")) e->nt_env = atoi(v) != 0;
        if (const char* v = getenv("KWOK_HB_KEEP")) e->keep_env = std::min(64, std::max(0, atoi(v)));
        if (const char* v = getenv("KWOK_HB_DELTA")) e->hb_delta = atoi(v) != 0;
        if (const char* v = getenv("KWOK_DEBUG_LAYOUT_FAULT_TICK")) e->debug_fault_tick = strtoull(v, nullptr, 10);
        if (const char* v = getenv("KWOK_DEBUG_INGEST_FAIL_CHUNK")) e->debug_fail_chunk = (uint32_t)strtoul(v, nullptr, 10);
        if (const char* v = getenv("KWOK_DEBUG_INGEST_FAIL_APPLY")) e->debug_fail_apply = (uint32_t)strtoul(v, nullptr, 10);
        e->iprof = getenv("KWOK_INGEST_PROF") != nullptr;
        if (const char* v = getenv("KWOK_INGEST_RESULTS_KERNEL")) e->results_kernel = v[0] == '1';
        if (const char* v = getenv("KWOK_INGEST_RS")) e->results_stream = v[0] != '0';
        if (const char* v = getenv("KWOK_INGEST_NEW_MAPPED")) e->new_mapped = v[0] != '0';
        if (const char* v = getenv("KWOK_INGEST_LAST_CUT")) e->last_chunk_cut = std::min(0.9, std::max(0.0, atof(v)));
        if (e->iprof)
            for (hipEvent_t& x : e->ing.tev) (void)hipEventCreate(&x);
        const char* ns = getenv("KWOK_TICK_NO_STREAM");
        e->no_stream = ns && ns[0] == '1';
        const char* qt = getenv("KWOK_QUIET");
        e->quiet_ok = !(qt && qt[0] == '0');
        const char* sj = getenv("KWOK_SPLIT");
        e->split_jobs = !(sj && sj[0] == '0');
        if (const char* v = getenv("KWOK_READ_STREAMS")) e->read_streams = std::max(1, std::min(4, atoi(v)));
        const char* sj2 = getenv("KWOK_SPARSE_JOBS");  // 0: k_pod_jobs<false> re-classifies the runs (A/B)
        e->sparse_jobs = !(sj2 && sj2[0] == '0');
        const char* fe = getenv("KWOK_FUSE_EMIT");
        e->fuse_emit = fe && fe[0] ? (fe[0] == '0' ? 0 : 1) : -1;
        const char* fi = getenv("KWOK_FOLD_INITS");
        e->fold_inits = !(fi && fi[0] == '0');
        const char* on = getenv("KWOK_ONCE");
        e->once_ok = !(on && on[0] == '0');
        const char* ost = getenv("KWOK_ONCE_STREAM");
        e->once_stream_ok = !(ost && ost[0] == '0');
        const char* cre = getenv("KWOK_COUNT_REUSE");
        e->count_reuse_ok = !(cre && cre[0] == '0');
        const char* os = getenv("KWOK_ONCE_SUM");
        e->once_sum_ok = !(os && os[0] == '0');
        const char* zc = getenv("KWOK_INGEST_ZC");
        e->ingest_zc = !(zc && zc[0] == '0');
    }
    S.n_node_slots = e->NL;
    S.n_pod_slots = e->PL;
    S.nb = e->nb;
    S.cn = e->Cn;
    S.cp = e->Cp;
    S.node_handle_base = (int32_t)(e->b_lo * e->Cn);
    S.pod_handle_base = 0;  // pod handles: pod_handle_of (stride)
    S.hb_units = e->hb_stride / 16;
    S.conds_off = e->hb_tpl.conds_off;
    S.conds_len = e->hb_tpl.conds_len;
    S.b_lo = e->b_lo;
    S.pod_stride = e->Hs;
    S.pool = e->pool;
    S.node_ip = e->node_ip;
    e->XW = W;
    if (const char* v = getenv("KWOK_XSPEC")) e->xspec_env = atoi(v);
    if (const char* v = getenv("KWOK_EMULATE_RANKS"))
        if (e->multi && W == 1) e->XW = std::max(1, std::min(atoi(v), 64));
    S.world = e->XW;  // the messages BACK folds
    S.multi = e->multi ? 1 : 0;
    S.cni = cfg->enable_cni ? 1u : 0u;
    S.custom_pod = (cfg->custom_templates & KWOK_TPL_POD) ? 1u : 0u;
    S.hb_once = (cfg->flags & KWOK_CFG_HEARTBEAT_ONCE) ? 1u : 0u;
    S.buckets = e->B;
    {
        // a chain block's bucket range must fit its LDS node flags and 64 pod chunks
        const uint32_t bpb = (e->nb + S.n_chain - 1) / S.n_chain;
        if (bpb > (uint32_t)MAX_BPB || (uint64_t)bpb * e->Cn > (uint64_t)NODE_LDS ||
            (uint64_t)bpb * (e->Cp / POD_PER_THREAD) > (uint64_t)MAX_POD_CHUNKS * BLOCK)
            return bail(e->fail(KWOK_EDOMAIN,
                                "%u buckets x (%u node, %u pod slots) per k_tick chain block exceed its limits "
                                "(%d buckets, %d node slots, %d pod groups): shard over more GPUs",
                                bpb, e->Cn, e->Cp, MAX_BPB, NODE_LDS, MAX_POD_CHUNKS * BLOCK));
    }
    const uint32_t nblk = (uint32_t)((e->pool.words + BLOCK * POOL_WPT_MIN - 1) / (BLOCK * POOL_WPT_MIN));
    // node / pod arrays: whole 16-byte vectors at the end (Cn % 4 == 0, Cp % 8 == 0)
    const size_t NLa = (size_t)e->NL + 16, PLa = (size_t)e->PL + 16;
    e->NLa = NLa;
    e->PLa = PLa;
    int rc = 0;
    if ((rc = dalloc(e, &S.node_state, NLa)) || (rc = dalloc(e, &S.node_blob, NLa)) ||
        (rc = dalloc(e, &S.node_tick, NLa)) || (rc = dalloc(e, &S.pod_state, PLa)) ||
        (rc = dalloc(e, &S.pod_node, PLa)) || (rc = dalloc(e, &S.pod_spec, PLa)) ||
        (rc = dalloc(e, &S.pod_ctime, PLa)) || (rc = dalloc(e, &S.pod_ip, PLa)) ||
        (rc = dalloc(e, &S.host_ip, PLa)) || (rc = dalloc(e, &S.used_bm, e->pool.words)) ||
        (rc = dalloc(e, &S.usable_bm, e->pool.words)) || (rc = dalloc(e, &S.rel_bm, e->pool.words)) ||
        (rc = dalloc(e, &S.list_counts, 2)) || (rc = dalloc(e, &e->d_pod_fill, e->nb)) || (rc = dalloc(e, &S.pool_index, 1)) ||
        (rc = dalloc(e, &S.pool_blk, 2 * (size_t)nblk)) || (rc = dalloc(e, &S.bar, 1)) ||
        (rc = dalloc(e, &S.blockagg, (size_t)S.n_chain * AG_STRIDE)) ||
        (rc = dalloc(e, &S.dmask, (size_t)S.n_chain * 2)) || (rc = dalloc(e, &S.list_blk, (size_t)S.n_chain * 2)) || (rc = dalloc(e, &e->d_hb_pre, (size_t)S.n_chain + 1)) ||
        (rc = dalloc(e, &e->d_hb_bpre, (size_t)e->nb + 1)) ||
        (rc = dalloc(e, &S.wc_pre, (size_t)S.n_chain * MAX_WC)) ||
        (rc = dalloc(e, &S.wc_dirty, (size_t)S.n_chain * WC_DIRTY_WORDS)) || (rc = dalloc(e, &S.jbase, (size_t)S.n_chain)) ||
        (e->sparse_jobs && (rc = dalloc(e, &S.gjob, (size_t)S.n_chain * MAX_WC * WC_GROUPS))) ||
        (getenv("KWOK_TICK_TRACE") && (rc = dalloc(e, &S.trace, (size_t)(S.n_chain + std::max(2 * e->n_stream, e->n_once_stream)) * TRACE_SLOTS))) ||
        (getenv("KWOK_JOBS_TRACE") && (rc = dalloc(e, &S.jtrace, (size_t)S.n_chain * (MAX_WC + 4) * 4))) ||
        (rc = dalloc(e, &S.alloc_addr, PLa)) || (rc = dalloc(e, (uint8_t**)&S.hb_static, HB_MAX_STRIDE)) ||
        (rc = dalloc(e, (uint8_t**)&S.hb_kind, HB_MAX_STRIDE)) ||
        (rc = dalloc(e, &S.hdr, 1)) || (rc = dalloc(e, &S.xmsg, 1)) || (rc = dalloc(e, &S.use_list, PLa)) ||
        (rc = dalloc(e, &S.rel_list, PLa)) || (rc = dalloc(e, &e->d_ld, (size_t)std::max(e->XW, 1))) ||
        (rc = dalloc(e, &S.node_key, NLa)) || (rc = dalloc(e, &S.node_name, NLa * NAME_STRIDE)) ||
        (rc = dalloc(e, &S.mb_count, e->nb)) || (rc = dalloc(e, &S.zb_count, e->nb)) ||
        (rc = dalloc(e, &S.once_sum, e->nb)) ||
        (rc = alloc_slot(e, 0)))
        return bail(rc);
    // heartbeat template: static bytes + kinds (0..19 Now, 20..39 StartTime)
    {
        const HeartbeatTemplate& hb = e->hb_tpl;
        std::vector<uint8_t> bytes(HB_MAX_STRIDE, 0), kind(HB_MAX_STRIDE, 0xFF);
        memcpy(bytes.data(), hb.bytes.data(), hb.bytes.size());
        for (uint16_t o : hb.now_slots)
            for (int i = 0; i < TS_LEN; i++) kind[o + i] = (uint8_t)i;
        for (uint16_t o : hb.start_slots)
            for (int i = 0; i < TS_LEN; i++) kind[o + i] = (uint8_t)(TS_LEN + i);
        // on the engine's stream, after dalloc's zero fills (a null-stream copy is
        // not ordered with a non-blocking stream: the fill could land after it)
        hipError_t r = hipMemcpyAsync((void*)S.hb_static, bytes.data(), HB_MAX_STRIDE, hipMemcpyHostToDevice, e->st);
        if (r == hipSuccess) r = hipMemcpyAsync((void*)S.hb_kind, kind.data(), HB_MAX_STRIDE, hipMemcpyHostToDevice, e->st);
        if (r == hipSuccess) r = hipStreamSynchronize(e->st);
        if (r != hipSuccess) return bail(e->fail(KWOK_EDEVICE, "template upload: %s", hipGetErrorString(r)));
        e->hb_gen++;  // (the template and `start` are fixed from here on: nothing else bumps it)
        e->state_changed();
        for (auto& T : e->slots) T.hb_valid.ok = false;
    }
    {
        const char* sy = getenv("KWOK_SYNC");
        e->sync_spin = !(sy && strcmp(sy, "block") == 0);
    }
    S.hb_pre = e->d_hb_pre;
    S.hb_bpre = e->d_hb_bpre;
    S.pod_fill = e->d_pod_fill;
    S.rank = e->rank;
    if (e->multi) {
        if ((rc = dalloc(e, &e->d_xall, (size_t)e->XW))) return bail(rc);
        S.xall = e->d_xall;
        if (hipHostMalloc((void**)&e->h_xall, sizeof(XMsg) * e->XW, hipHostMallocDefault) != hipSuccess)
            return bail(KWOK_ENOMEM);
        if (cfg->comm_id) {
            ncclUniqueId id;
            memcpy(&id, cfg->comm_id, sizeof(id));
            ncclResult_t r = ncclCommInitRank(&e->comm, W, id, e->rank);
            if (r != ncclSuccess) return bail(e->fail(KWOK_ECOMM, "ncclCommInitRank: %s", ncclGetErrorString(r)));
        }
    }
    {
        // host threads of node batches' string work: KWOK_INGEST_THREADS, else up to 16
        unsigned hw = std::thread::hardware_concurrency();
        int np = (int)std::min(16u, hw ? hw : 1u);
        if (const char* v = getenv("KWOK_INGEST_THREADS")) np = atoi(v);
        e->n_part = std::max(1, std::min(np, 64));
    }
    {  // GPU pod ingest: per-bucket / per-node-slot scratch and the batch summary
        auto& g = e->ing;
        if ((rc = dalloc(e, &g.abort, 1)) || (rc = dalloc(e, &g.beg, e->nb)) || (rc = dalloc(e, &g.end, e->nb)) ||
            (rc = dalloc(e, &g.sum, 1)) || (rc = dalloc(e, &g.nsum, 1)) || (rc = dalloc(e, &g.sum1, 1)))
            return bail(rc);
        if (hipHostMalloc((void**)&g.sum_h, sizeof(IngSummary), hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc((void**)&g.nsum_h, sizeof(NodeSummary), hipHostMallocDefault) != hipSuccess)
            return bail(KWOK_ENOMEM);
        hipError_t r = hipStreamCreateWithFlags(&g.pst, hipStreamNonBlocking);
        if (r == hipSuccess) r = hipStreamCreateWithFlags(&g.dst, hipStreamNonBlocking);
        hipEvent_t* evs[] = {&g.go, &g.prepped[0], &g.prepped[1], &g.used[0], &g.used[1], &g.rdone, &g.idone};
        for (hipEvent_t* x : evs)
            if (r == hipSuccess) r = hipEventCreateWithFlags(x, hipEventDisableTiming);
        if (r != hipSuccess) return bail(e->fail(KWOK_EDEVICE, "ingest stream/events: %s", hipGetErrorString(r)));
        if (const char* v = getenv("KWOK_INGEST_CHUNK")) g.chunk = std::max<size_t>(1, strtoull(v, nullptr, 10));
        // The runtime creates a copy engine's queue the first time it hands that engine a
        // copy, holding the submitting host thread ~6 ms (C4: one or two batches of a
        // process's first ~10 paid it inside the timed ingest, whatever the host memory;
        // tools/gpu_r4v.sh, profiles/r4v_sdma_ab.txt).  Copies in both directions on every
        // stream the engine uses, several in flight at once, spread over the engines here
        // at create time instead (KWOK_COPY_WARM=0: off).
        const char* cw = getenv("KWOK_COPY_WARM");
        if (!(cw && cw[0] == '0')) {
            const size_t wb = (size_t)8 << 20;
            void *hbuf = nullptr, *dbuf = nullptr;
            if (hipHostMalloc(&hbuf, wb * 4, hipHostMallocDefault) == hipSuccess && hipMalloc(&dbuf, wb * 4) == hipSuccess) {
                hipStream_t ss[4] = {e->st, g.pst, g.dst, e->rst};
                for (int round = 0; round < 4; round++)
                    for (int q = 0; q < 4; q++) {
                        char* h = (char*)hbuf + (size_t)q * wb;
                        char* d = (char*)dbuf + (size_t)q * wb;
                        (void)hipMemcpyAsync(round & 1 ? h : d, round & 1 ? d : h, wb,
                                             round & 1 ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice, ss[q]);
                    }
                for (hipStream_t x : ss) (void)hipStreamSynchronize(x);
            }
            if (dbuf) (void)hipFree(dbuf);
            if (hbuf) (void)hipHostFree(hbuf);
        }
    }
    e->max_init_len = 0;
    if ((rc = size_arena(e)) || (rc = grow_arena(e, e->slots[0]))) return bail(rc);
    // a warm-up launch of k_tick (phases 0: every block returns at once): the runtime
    // sets up the queue's scratch for the kernel here, not inside the first tick
    // (measured ~0.3-0.6 ms on the initial tick when k_tick's frame is not empty)
    launch_tick(S, e->n_stream, 0, 0, 0, 0, 0, 0, e->st);
    {
        hipError_t r = hipStreamSynchronize(e->st);
        if (r != hipSuccess) return bail(e->fail(KWOK_EDEVICE, "create sync: %s", hipGetErrorString(r)));
    }
    *out = e;
    return KWOK_OK;
}

int kwok_register_pod_spec(kwok_engine* e, const kwok_pod_spec* spec, const char* arena, size_t arena_len,
                           int32_t* out_id) {
    if (!e || !spec || !out_id) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    drain(e);  // the host mirrors reflect every submitted tick
    if (e->poisoned) return poisoned(e);
    auto get = [&](kwok_str s, std::string& o) {
        if ((size_t)s.off + s.len > arena_len) return false;
        o.assign(arena + s.off, s.len);
        return safe_string(o.data(), o.size());
    };
    std::vector<Container> cs(spec->n_containers), ics(spec->n_init_containers);
    std::vector<std::string> gates(spec->n_readiness_gates);
    for (uint32_t i = 0; i < spec->n_containers; i++)
        if (!get(spec->containers[i].name, cs[i].name) || !get(spec->containers[i].image, cs[i].image))
            return e->fail(KWOK_EDOMAIN, "container %u: not a safe string", i);
    for (uint32_t i = 0; i < spec->n_init_containers; i++)
        if (!get(spec->init_containers[i].name, ics[i].name) || !get(spec->init_containers[i].image, ics[i].image))
            return e->fail(KWOK_EDOMAIN, "init container %u: not a safe string", i);
    for (uint32_t i = 0; i < spec->n_readiness_gates; i++)
        if (!get(spec->readiness_gates[i], gates[i])) return e->fail(KWOK_EDOMAIN, "readiness gate %u: not a safe string", i);
    SpecProgram p;
    if (e->custom_pod) {
        std::string why;
        if (!compile_pod_template(e->pod_tpl, cs, ics, gates, e->start_s, p, why))
            return e->fail(KWOK_EDOMAIN, "pod status template: %s", why.c_str());
    } else {
        p = build_spec_program(cs, ics, gates);
    }
    if (p.max_len > 0xFFF0) return e->fail(KWOK_EDOMAIN, "pod patch longer than 64 KiB");
    std::vector<uint16_t> nxt;
    if (!build_ts_lookup(p, nxt)) return e->fail(KWOK_EDOMAIN, "pod patch layout outside the emitter's domain");
    std::string tab;
    std::vector<uint16_t> tdesc;
    const bool tabled = build_unit_tables(p, tab, tdesc);  // else: the general emitter path only
    std::string key = p.a + '\x01' + p.ka + '\x01' + p.b + '\x01' + p.kb + '\x01' + p.c + '\x01' + p.kc;
    std::string canon = json_spec_canon(cs, ics, gates);
    const uint64_t skey = json_spec_key(canon);  // the GPU codec finds the spec by this key (and checks canon)
    auto note = [&](int32_t id) {
        auto k = e->spec_keys.emplace(skey, id);
        if (k.second) e->spec_canon[skey] = std::move(canon);
        if (!k.second && k.first->second != id) k.first->second = -2;  // (a 64-bit collision: the host decides)
        if (k.second || k.first->second == -2) e->json.tab_dirty = true;
    };
    auto it = e->spec_ids.find(key);
    if (it != e->spec_ids.end()) {
        *out_id = it->second;
        note(it->second);
        return KWOK_OK;
    }
    uint32_t cap = e->cfg.max_pod_specs ? std::min<uint32_t>(e->cfg.max_pod_specs, 65535) : 1024;
    if (e->specs_h.size() >= cap) return e->fail(KWOK_EFULL, "max_pod_specs reached");
    SpecDesc d{};
    d.off = (uint32_t)e->spec_bytes_h.size();
    d.len_a = (uint16_t)p.a.size();
    d.len_b = (uint16_t)p.b.size();
    d.len_c = (uint16_t)p.c.size();
    d.max_len = (uint16_t)p.max_len;
    d.nxt_off = (uint32_t)e->spec_nxt_h.size();
    d.tab_off = NO_TAB;
    // KWOK_EMIT_TAB_UNITS caps the table units (tests: 0 = the general emitter only, small = mixed chunks)
    const char* cap_env = getenv("KWOK_EMIT_TAB_UNITS");
    const size_t tab_cap = cap_env ? (size_t)strtoull(cap_env, nullptr, 10) : (size_t)MAX_TAB_UNITS;
    if (tabled && e->tab_units + tdesc.size() <= std::min(tab_cap, (size_t)MAX_TAB_UNITS)) {
        const size_t n = e->tab_units + tdesc.size();
        int rc;
        if ((rc = dgrow(e, e->d_unit_tab, n * 16)) || (rc = dgrow(e, e->d_unit_desc, n))) return rc;
        HIPCHK(e, hipMemcpyAsync(e->d_unit_tab.p + (size_t)e->tab_units * 16, tab.data(), tab.size(),
                                 hipMemcpyHostToDevice, e->st));
        HIPCHK(e, hipMemcpyAsync(e->d_unit_desc.p + e->tab_units, tdesc.data(), tdesc.size() * 2,
                                 hipMemcpyHostToDevice, e->st));
        d.tab_off = e->tab_units;
        e->tab_units = (uint32_t)n;
        e->S.unit_tab = reinterpret_cast<const uint4*>(e->d_unit_tab.p);
        e->S.unit_desc = e->d_unit_desc.p;
    }
    if (d.tab_off == NO_TAB) e->n_untabled++;
    const std::string kinds = p.ka + p.kb + p.kc;
    for (size_t i = 0; i < kinds.size(); i++)  // slot starts (kinds 0..19 in a row)
        if (kinds[i] == 0) d.n_ts++;
    e->spec_nxt_h.insert(e->spec_nxt_h.end(), nxt.begin(), nxt.end());
    e->spec_bytes_h += p.a + p.b + p.c;
    e->specs_h.push_back(d);
    int rc = upload_specs(e);
    if (rc) return rc;
    e->max_pod_len = std::max(e->max_pod_len, p.max_len);
    if ((rc = size_arena(e))) return rc;
    *out_id = (int32_t)(e->specs_h.size() - 1);
    e->spec_ids.emplace(key, *out_id);
    note(*out_id);
    return KWOK_OK;
}

// node batch buffers for n records (the pod batch's sort buffers are shared)
int node_reserve(kwok_engine* e, size_t n, size_t arena_len) {
    auto& G = e->ing;
    if (int rc = ingest_reserve(e, n, arena_len)) return rc;
    if (n <= G.nodes.cap) return KWOK_OK;
    G.res_h.release();
    if (int rc = G.nodes.reserve(e, n)) return rc;
    if (hipHostMalloc((void**)&G.res_h.p, G.nodes.cap * 8, hipHostMallocDefault) != hipSuccess) {
        G.nodes.release();
        return e->fail(KWOK_ENOMEM, "node results");
    }
    return KWOK_OK;
}

// The status of a node the device could not settle alone (a non-empty status, or
// a custom node template): the string checks and the init blob (node.init.tpl /
// Config.NodeInitializationTemplate), CONFORMS (A.5).  Host string work, on the
// partition threads; blob interning under blob_mu.
// cd (kwok_canon.h): the record's blob spans are the raw values of a document the device canonicalised;
// the canonical bytes are cd's, in cbytes.
NodeFix complete_node(kwok_engine* e, const kwok_node_event& x, uint32_t idx, const char* arena, std::mutex& blob_mu,
                      const CanonDoc* cd = nullptr, const char* cbytes = nullptr) {
    NodeFix f{};
    f.idx = idx;
    int st = KWOK_OK;
    std::string info[KWOK_NI_COUNT];
    for (int k = 0; k < KWOK_NI_COUNT && st == KWOK_OK; k++)
        if (x.node_info[k].len) {
            info[k].assign(arena + x.node_info[k].off, x.node_info[k].len);
            if (!safe_string(info[k].data(), info[k].size())) st = KWOK_EDOMAIN;
        }
    std::string js[3];
    const kwok_str* jr[3] = {&x.addresses, &x.allocatable, &x.capacity};
    for (int k = 0; k < 3 && st == KWOK_OK; k++)
        if (jr[k]->len) {
            if (cd) js[k].assign(cbytes + cd->off[k], cd->len[k]);
            else js[k].assign(arena + jr[k]->off, jr[k]->len);
            if (!valid_json_blob(js[k].data(), js[k].size(), k == 0 ? '[' : '{')) st = KWOK_EDOMAIN;
        }
    if (st == KWOK_OK) {
        std::lock_guard<std::mutex> lock(blob_mu);
        if (e->custom_node) {
            // one compile per distinct status (the fields the template may read)
            std::string key = std::to_string(x.phase);
            for (int k = 0; k < 3; k++) key += '\x01' + js[k];
            for (int k = 0; k < KWOK_NI_COUNT; k++) key += '\x01' + info[k];
            auto it = e->node_tpl_blobs.find(key);
            if (it != e->node_tpl_blobs.end()) {
                f.blob = it->second;
            } else {
                NodeBlob nb;
                std::string why;
                if (!compile_node_template(e->node_tpl, js[0], js[1], js[2], info, x.phase, e->node_ip_s, e->start_s,
                                           e->hb_tpl, nb, why)) {
                    st = KWOK_EDOMAIN;
                } else {
                    f.blob = intern_blob(e, nb, &st);
                    if (st == KWOK_OK) e->node_tpl_blobs.emplace(std::move(key), f.blob);
                }
            }
        } else {
            f.blob = intern_blob(e, build_node_blob(js[0], js[1], js[2], info, e->node_ip_s), &st);
        }
    }
    f.status = st;
    f.conforms = st == KWOK_OK && !e->custom_node && node_conforms(x, info) ? 1u : 0u;
    return f;
}

// kwok_ingest_nodes: the WatchNodes / ListNodes event switch (node_controller.go:
// 256-270) on the GPU over the device node directory (ingest.hip): prep, the host's
// completions of non-empty statuses, a stable sort by bucket, one wave per bucket
// in event order.  Two host round trips per batch (the prep summary, the results).
// kwok_ingest_nodes_json: the records were decoded on the device (G.d_nev, the
// documents in G.d_arena); the records the host completes come from here
struct NodeJsonCtx {
    const char* arena;                            // the caller's documents (device-decoded records' spans)
    const std::unordered_map<uint32_t, uint32_t>* hdoc;  // document -> its host decode (hrec / hbuf)
    const std::vector<kwok_node_event>* hrec;     // host-decoded records, spans into their hbuf
    const std::vector<std::string>* hbuf;
    const kwok_engine::Canon* canon = nullptr;    // the decode's device-canonicalised documents (kwok_canon.h), or null
};
int ingest_nodes_impl(kwok_engine* e, const kwok_node_event* ev, size_t n, const char* arena, size_t arena_len,
                      int32_t* out_handles, int32_t* out_status, const NodeJsonCtx* nj);
int kwok_ingest_nodes(kwok_engine* e, const kwok_node_event* ev, size_t n, const char* arena, size_t arena_len,
                      int32_t* out_handles, int32_t* out_status) {
    if (!e || (n && !ev) || n > 0x7FFFFFF0ull || (arena_len && !arena)) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    drain(e);  // the device state reflects every submitted tick
    if (e->poisoned) return poisoned(e);
    e->emit_hint = true;
    e->quiet = 0;
    e->state_changed();
    if (!n) return 0;
    int rc = node_reserve(e, n, arena_len);
    if (rc) return rc;
    return ingest_nodes_impl(e, ev, n, arena, arena_len, out_handles, out_status, nullptr);
}
int ingest_nodes_impl(kwok_engine* e, const kwok_node_event* ev, size_t n, const char* arena, size_t arena_len,
                      int32_t* out_handles, int32_t* out_status, const NodeJsonCtx* nj) {
    const auto t0 = clk::now();
    int rc = 0;
    e->state_changed();  // (every node batch, whatever its entry point: node states, hb_bpre, the managed count)
    if (e->refs.on && n) e->refs.gen[KWOK_KIND_NODES]++;  // (kwok_read_refs' stale guard: the batch may create nodes)
    auto& G = e->ing;
    hipStream_t st = e->st;
    // the empty-status blob (kwok's own fleets create Nodes with an empty status)
    if (!e->custom_node && !e->has_empty_blob.load()) {
        std::string empty[KWOK_NI_COUNT];
        int brc = KWOK_OK;
        const uint64_t b = intern_blob(e, build_node_blob("", "", "", empty, e->node_ip_s), &brc);
        if (brc) return e->fail(brc, "empty node status blob");
        e->empty_blob = b;
        e->has_empty_blob.store(true);
    }
    // the batch in kwok_host_alloc memory is read in place by k_nd_prep; any other is copied
    // (kwok_ingest_nodes_json: both on the device already)
    const void* zev = !nj && e->ingest_zc ? host_mapped(ev, n * sizeof(kwok_node_event)) : nullptr;
    const void* zar = !nj && e->ingest_zc && arena_len ? host_mapped(arena, arena_len) : nullptr;
    if (!zev && !nj) HIPCHK(e, hipMemcpyAsync(G.d_nev, ev, n * sizeof(kwok_node_event), hipMemcpyHostToDevice, st));
    if (arena_len && !zar && !nj) HIPCHK(e, hipMemcpyAsync(G.d_arena, arena, arena_len, hipMemcpyHostToDevice, st));
    NodeBatch N{};
    N.ev = static_cast<const kwok_node_event*>(zev ? zev : (const void*)G.d_nev);
    N.n = (uint32_t)n;
    N.host_all = e->custom_node ? 1u : 0u;
    N.arena = zar ? static_cast<const uint8_t*>(zar) : G.arena_src ? G.arena_src : G.d_arena;
    N.arena_len = arena_len;
    N.empty_blob = e->empty_blob;
    N.rec = G.nrec;
    N.names = G.d_nnames;
    N.keys = G.keys;
    N.keys_sorted = G.keys_sorted;
    N.idx_sorted = G.idx_sorted;
    N.beg = G.beg;
    N.end = G.end;
    N.out_handle = G.out_handle;
    N.out_status = G.out_status;
    N.host_idx = G.host_idx;
    N.sum = G.nsum;
    HIPCHK(e, hipMemsetAsync(G.nsum, 0, sizeof(NodeSummary), st));
    launch_node_prep(e->S, N, st);
    HIPCHK(e, hipGetLastError());
    // sort + apply + results queued right behind the prep: the apply pass returns at
    // once on the device when the prep listed records for the host (then the host
    // completes them and runs the sort and the pass again); one round trip otherwise
    auto sort_apply_results = [&]() -> int {
        if (launch_node_sort(e->S, N, G.sort_tmp, G.sort_bytes, sort_bits(e), st))
            return e->fail(KWOK_EDEVICE, "node sort");
        launch_node_apply(e->S, N, st);
        HIPCHK(e, hipGetLastError());
        if (int r = release_for_host(e)) return r;
        if (out_handles) HIPCHK(e, hipMemcpyAsync(G.res_h, G.out_handle, n * 4, hipMemcpyDeviceToHost, st));
        if (out_status) HIPCHK(e, hipMemcpyAsync(G.res_h + n, G.out_status, n * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipMemcpyAsync(G.nsum_h, G.nsum, sizeof(NodeSummary), hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipStreamSynchronize(st));
        return KWOK_OK;
    };
    // from the apply pass on the batch is in the device state: a failure poisons the engine
    auto failed = [&](int r) {
        e->poisoned = true;
        return r;
    };
    if ((rc = upload_blobs(e))) return rc;  // (the empty-status blob, first batch)
    if ((rc = sort_apply_results())) return failed(rc);
    const auto t1 = clk::now();
    const uint32_t n_host = G.nsum_h->n_host;
    if (n_host) {
        // the records whose status strings need the host, in batch order (blob offsets do not
        // depend on it, but a deterministic interning order keeps the blob store reproducible)
        std::vector<uint32_t> idx(n_host);
        HIPCHK(e, hipMemcpyAsync(idx.data(), G.host_idx, (size_t)n_host * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipStreamSynchronize(st));
        std::sort(idx.begin(), idx.end());
        std::vector<NodeFix> fix(n_host);
        std::mutex blob_mu;
        const bool par = n_host >= NODE_PAR_MIN && e->n_part > 1;
        // kwok_ingest_nodes_json: the listed records the device decoded come back from
        // the device (their spans index the caller's documents); the host-decoded ones
        // are at hand with their canonical blobs
        std::vector<kwok_node_event> dev_rec;
        if (nj) {
            dev_rec.resize(n_host);
            HIPCHK(e, hipMemcpyAsync(G.host_idx, idx.data(), (size_t)n_host * 4, hipMemcpyHostToDevice, st));
            launch_node_gather(G.d_nev, G.host_idx, n_host, e->json.nev_fix, st);
            HIPCHK(e, hipGetLastError());
            HIPCHK(e, hipMemcpyAsync(dev_rec.data(), e->json.nev_fix, (size_t)n_host * sizeof(kwok_node_event),
                                     hipMemcpyDeviceToHost, st));
            HIPCHK(e, hipStreamSynchronize(st));
        }
        run_parts(e, par, [&](int p) {
            const size_t lo = par ? (size_t)n_host * p / e->n_part : (p ? n_host : 0);
            const size_t hi = par ? (size_t)n_host * (p + 1) / e->n_part : n_host;
            for (size_t k = lo; k < hi; k++) {
                if (!nj) {
                    fix[k] = complete_node(e, ev[idx[k]], idx[k], arena, blob_mu);
                    continue;
                }
                auto h = nj->hdoc->find(idx[k]);
                if (h != nj->hdoc->end()) {
                    fix[k] = complete_node(e, (*nj->hrec)[h->second], idx[k], (*nj->hbuf)[h->second].data(), blob_mu);
                    continue;
                }
                // (a document the device canonicalised: its blobs from the canonical buffer, never the document's)
                const CanonDoc* cd = nj->canon ? nj->canon->find(idx[k]) : nullptr;
                fix[k] = complete_node(e, dev_rec[k], idx[k], nj->arena, blob_mu, cd, cd ? nj->canon->bytes_h.data() : nullptr);
            }
        });
        if ((rc = upload_blobs(e))) return rc;
        HIPCHK(e, hipMemcpyAsync(G.d_nfix, fix.data(), fix.size() * sizeof(NodeFix), hipMemcpyHostToDevice, st));
        launch_node_fix(e->S, N, G.d_nfix, n_host, st);
        HIPCHK(e, hipGetLastError());
        N.force = 1;
        if ((rc = sort_apply_results())) return failed(rc);
    }
    if (e->ndir.on) {  // the uid rule behind the batch's last apply pass (reads its results; no node_state is written)
        const NodeUidNote none{};
        launch_nd_uid_note(e->S, N, e->ndir.dir(), e->ndir.note ? *e->ndir.note : none, st);
        if (hipGetLastError() != hipSuccess) return failed(e->fail(KWOK_EDEVICE, "node uid note"));
    }
    if (e->resync.open[KWOK_KIND_NODES]) {  // the batch's final results mark their nodes (before the buffers' next use)
        launch_seen_mark_nodes(e->S, N, e->resync.node_seen, e->resync.ctr, st);
        HIPCHK(e, hipGetLastError());
    }
    const auto t2 = clk::now();
    if (out_handles) memcpy(out_handles, G.res_h, n * 4);
    if (out_status) memcpy(out_status, G.res_h + n, n * 4);
    const NodeSummary sum = *G.nsum_h;
    e->n_managed = (uint64_t)((int64_t)e->n_managed + sum.d_managed);
    if (sum.changed) {
        e->hb_pre_dirty = true;
        e->hb_epoch++;  // the managed set changed in this batch
    }
    if ((rc = size_arena(e))) return failed(rc);
    if (e->iprof)
        fprintf(stderr, "[kwok ingest] %zu node records (GPU%s): prep + sort + apply + results %.3f ms, host %u "
                        "records + again %.3f ms (%u created, %u freed)\n", n, zev ? ", read in place" : "",
                ms_between(t0, t1), n_host, ms_between(t1, t2), sum.created, sum.freed);
    return (int)sum.rejected;
}

// The stable sort by bucket of one chunk and its growth check (k_ing_need counts
// the creates in each bucket's sorted range), queued on the engine stream
int enqueue_sort_need(kwok_engine* e, const IngestBatch& I) {
    auto& G = e->ing;
    hipStream_t st = e->st;
    if (launch_ingest_sort(e->S, I, G.sort_tmp, G.sort_bytes, sort_bits(e), st))
        return e->fail(KWOK_EDEVICE, "ingest sort");
    launch_ingest_need(e->S, I, st);
    HIPCHK(e, hipGetLastError());
    return KWOK_OK;
}
// ... and its apply pass (spec: queued without the host's growth check; the pass
// then returns on the device if the chunk needs growth)
int enqueue_apply(kwok_engine* e, IngestBatch I, bool spec) {
    I.spec = spec ? 1u : 0u;
    if (I.n) e->ing_mutated = true;  // pod slots, node entries and references and the pool change from here on
    launch_ingest_apply(e->S, I, e->st);
    HIPCHK(e, hipGetLastError());
    return KWOK_OK;
}

// One chunk of a pod batch after its prep (I: the chunk's records, indices
// chunk-local), with the host in the loop: the growth check, the stable sort by
// bucket and the apply pass (by-name creates resolve their node in it).  Returns
// the chunk's rejected count (>= 0) or an error.  (The batch path queues the
// chunks without it and comes here only for a chunk that needs growth.)
int ingest_chunk(kwok_engine* e, const IngestBatch& I) {
    auto& G = e->ing;
    int rc = 0;
    if ((rc = enqueue_sort_need(e, I))) return rc;
    if ((rc = read_summary(e, I.sum))) return rc;
    const IngSummary sum = *G.sum_h;
    // growth: every bucket to a larger capacity (up to the handle stride) when the
    // chunk's creates could fill one
    if (sum.need > e->Cp) {
        const uint32_t cap = max_pod_capacity(e);
        if (cap > e->Cp) {
            e->ing_mutated = true;  // (a failed growth leaves the layout half changed)
            const uint32_t want = (uint32_t)std::min<uint64_t>(cap, std::max<uint64_t>(((uint64_t)sum.need + 7) & ~7ull, 2ull * e->Cp));
            if (e->iprof) fprintf(stderr, "[kwok grow] pod capacity per bucket %u -> %u\n", e->Cp, want);
            if ((rc = grow_pods(e, want))) return rc;
        }
    }
    if ((rc = enqueue_apply(e, I, false))) return rc;
    if ((rc = read_summary(e, I.sum))) return rc;
    if (G.sum_h->foreign) e->foreign_ips = true;
    return (int)G.sum_h->rejected;
}

// kwok_ingest_pods / kwok_ingest_pods_packed: recs are kwok_pod_event (with their
// string arena) or, packed, kwok_pod_rec (no arena); statuses to out_status
// (int32) or out_status8 (int8)
// resident: the records (kwok_pod_event) and their arena are on the device already,
// in the ingest buffers (kwok_ingest_pods_json decoded them there)
// packed: 0 kwok_pod_event, 1 kwok_pod_rec, 2 kwok_pod_rec12 (the creates' handles to
// out_new[k < new_cap], in create order; out_handles unused)
int ingest_pods_impl(kwok_engine* e, const void* recs, int packed, size_t n, const char* arena, size_t arena_len,
                     int32_t* out_handles, int32_t* out_status, int8_t* out_status8, uint32_t* out_released,
                     bool resident = false, int32_t* out_new = nullptr, size_t new_cap = 0, int64_t tick_now = -1) {
    const size_t RB = packed == 2 ? sizeof(kwok_pod_rec12) : packed ? sizeof(kwok_pod_rec) : sizeof(kwok_pod_event);
    static_assert(sizeof(kwok_pod_rec12) == 12, "kwok_pod_rec12 is 12 bytes");
    auto rec_at = [&](const void* base, size_t i) { return static_cast<const uint8_t*>(base) + i * RB; };
    if (e->poisoned) return poisoned(e);
    drain(e);  // the device state reflects every submitted tick
    if (e->poisoned) return poisoned(e);
    if (tick_now >= 0) {  // (checked before anything is queued)
        if (e->multi) return e->fail(KWOK_EINVAL, "ingest + tick in one call: single-rank engines only");
        if (int rc = tick_submit_check(e, tick_now)) return rc;
    }
    e->emit_hint = true;
    e->quiet = 0;
    e->state_changed();
    if (!n) return tick_now >= 0 ? tick_submit_impl(e, tick_now) : 0;
    if (e->refs.on) e->refs.gen[KWOK_KIND_PODS]++;  // (kwok_read_refs' stale guard: the batch may create pods)
    e->pod_records_since_tick += n;
    const auto t0 = clk::now();
    int rc = ingest_reserve(e, n, e->ing.arena_src ? 0 : arena_len);  // (a framed batch: its strings are resident)
    if (rc) return rc;
    auto& G = e->ing;
    hipStream_t st = e->st, ps = G.pst;
    // Chunks of the batch in event order: applying them one after the other is
    // applying the batch (every record is applied in event order; a chunk is what
    // a separate call with those records would do).  The copy engine moves chunk
    // k+1's records to HBM (and k_ing_prep prepares them) on the prep stream while
    // the engine stream applies chunk k, and chunk k's results go back on the
    // results stream: the link carries the batch once in each direction, with the
    // apply passes under it.  The last chunk is shorter (its apply and results are
    // the part nothing hides).  The prep of chunk k + 2 waits until chunk k has
    // released its accumulator set.
    // kwok_pod_rec12's chunks start at multiples of 256 records (its create counts are
    // per 256-record tile, tile_new[lo / 256 + block]); its chunks hold at least 512
    // records, so that every chunk start rounds to a new tile and no chunk is empty.
    // The other wire forms split anywhere.
    const size_t chunk = packed == 2 ? std::max<size_t>(G.chunk, 512) : G.chunk;
    const uint32_t K = n > chunk ? (uint32_t)((n + chunk - 1) / chunk) : 1u;
    const double W = K > 1 ? K - e->last_chunk_cut : 1.0;
    const size_t lo_mask = packed == 2 ? ~(size_t)255 : ~(size_t)0;
    auto lo_of = [&](uint32_t k) { return k >= K ? n : (size_t)((double)n * k / W) & lo_mask; };
    // a one-chunk batch in kwok_host_alloc memory is read in place by k_ing_prep
    // (the only kernel that reads the records and their strings): one pass over
    // the link, no copy engine (KWOK_INGEST_ZC=0: copy it to HBM first).  Chunked
    // batches are copied: kernels reading host memory in place hold their CUs for
    // the link's latency, and the apply passes beside them stall (1M deletes + 1M
    // creates in 4 chunks: 4.9 ms read in place against 2.8 ms copied).
    if (K > G.nsums) {  // one summary per chunk: the batch reads them back once, at its end
        if (G.sums) (void)hipFree(G.sums);
        if (G.sums_h) (void)hipHostFree(G.sums_h);
        G.sums = nullptr, G.sums_h = nullptr, G.nsums = 0;
        const size_t m = std::max<size_t>(K, 16);
        if ((rc = dalloc(e, &G.sums, m))) return rc;
        if (hipHostMalloc((void**)&G.sums_h, m * sizeof(IngSummary), hipHostMallocDefault) != hipSuccess)
            return e->fail(KWOK_ENOMEM, "ingest summaries");
        G.nsums = m;
    }
    // (kwok_pod_rec12 records are read as three dwords: in place only when 4-byte aligned)
    const bool zc_ok = e->ingest_zc && K == 1 && !resident && (packed != 2 || ((uintptr_t)recs & 3) == 0);
    // kwok_pod_rec12's create handles: written by the kernel straight into a
    // kwok_host_alloc out_new_handles (each chunk's as it completes; no copy at the
    // batch's end), else into HBM and copied back after the last chunk.  With the
    // tick behind the batch they always take the copy: the kernel's writes over the
    // link hold CUs beside the tick's persistent blocks (C4 step 1.08-1.10 -> 1.04-1.05
    // ms, profiles/r13_new_handles_ab.txt; as two calls the in-place form is as fast)
    int32_t* new_map = packed == 2 && new_cap && e->new_mapped && tick_now < 0
                           ? (int32_t*)host_mapped(out_new, new_cap * 4)
                           : nullptr;
    int32_t* new_dst = new_map ? new_map : G.new_handle;
    const void* zev = zc_ok ? host_mapped(recs, n * RB) : nullptr;
    const void* zar = zc_ok && arena_len ? host_mapped(arena, arena_len) : nullptr;
    auto chunk_batch = [&](uint32_t k) {
        const size_t lo = lo_of(k);
        IngestBatch b = ingest_batch(e, (uint32_t)(lo_of(k + 1) - lo), arena_len);
        b.packed = (uint32_t)packed;
        if (packed == 2) b.tile_new = G.tile_new, b.tile_pre = G.tile_pre, b.tile0 = (uint32_t)(lo / 256);
        b.ev = rec_at(zev ? zev : (const void*)G.d_ev, lo);
        if (zar) b.arena = (const uint8_t*)zar;
        b.rec += lo, b.keys += lo, b.keys_sorted += lo, b.idx_sorted += lo;
        b.out_handle += lo, b.out_status += lo, b.out_released += lo;
        b.sum = G.sums + k;
        b.abort = G.abort;
        return b;
    };
    // prep of chunk k on stream s (the batch: the prep stream; a redo: the engine stream)
    auto prep_on = [&](uint32_t k, hipStream_t s) -> int {
        const IngestBatch b = chunk_batch(k);
        HIPCHK(e, hipMemsetAsync(b.sum, 0, sizeof(IngSummary), s));
        if (!zev && !resident)
            HIPCHK(e, hipMemcpyAsync(const_cast<uint8_t*>(rec_at(G.d_ev, lo_of(k))), rec_at(recs, lo_of(k)), (size_t)b.n * RB,
                                     hipMemcpyHostToDevice, s));
        launch_ingest_prep(e->S, b, s);
        HIPCHK(e, hipGetLastError());
        return KWOK_OK;
    };
    const bool tstamp = e->iprof && G.tev[0] && K == 2;
    clk::time_point t_copy0 = t0, t_synced = t0;
    // (the copy goes ahead of the summary reset: the link starts as early as possible.
    // Chunk 0 waits for the engine stream's earlier work first - the buffers' zeroing
    // when ingest_reserve just allocated them, above all)
    auto prep = [&](uint32_t k) -> int {
        const IngestBatch b = chunk_batch(k);
        if (k == 0) {
            t_copy0 = clk::now();
            HIPCHK(e, hipStreamWaitEvent(ps, G.go, 0));
        }
        if (tstamp) HIPCHK(e, hipEventRecord(G.tev[2 * k], ps));  // 0 / 2: chunk k's copy starts
        if (!zev && !resident)
            HIPCHK(e, hipMemcpyAsync(const_cast<uint8_t*>(rec_at(G.d_ev, lo_of(k))), rec_at(recs, lo_of(k)), (size_t)b.n * RB,
                                     hipMemcpyHostToDevice, ps));
        if (k >= 2) HIPCHK(e, hipStreamWaitEvent(ps, G.used[k & 1], 0));
        HIPCHK(e, hipMemsetAsync(b.sum, 0, sizeof(IngSummary), ps));
        launch_ingest_prep(e->S, b, ps);
        HIPCHK(e, hipGetLastError());
        if (tstamp) HIPCHK(e, hipEventRecord(G.tev[2 * k + 1], ps));  // 1 / 3: its prep done
        HIPCHK(e, hipEventRecord(G.prepped[k & 1], ps));
        return KWOK_OK;
    };
    e->ing_mutated = false;  // set by ingest_chunk once the batch changes any state
    // the prep stream starts after the work already queued on the engine stream
    // results of chunk k (after its apply pass, on the results stream) -> the caller's arrays
    auto results = [&](uint32_t k, hipStream_t rs) -> int {
        const size_t lo = lo_of(k);
        const IngestBatch I = chunk_batch(k);
        // KWOK_INGEST_RESULTS_KERNEL=1: results into kwok_host_alloc arrays written by a
        // kernel through their mapped addresses instead of the copy engine (slower:
        // 1.9 vs 1.45 ms per C4 batch; kept for A/B of the host-side stalls, §11)
        int32_t* mh = out_handles ? (int32_t*)host_mapped(out_handles + lo, (size_t)I.n * 4) : nullptr;
        int32_t* ms = out_status ? (int32_t*)host_mapped(out_status + lo, (size_t)I.n * 4) : nullptr;
        int8_t* m8 = out_status8 ? (int8_t*)host_mapped(out_status8 + lo, I.n) : nullptr;
        uint32_t* mr = out_released ? (uint32_t*)host_mapped(out_released + lo, (size_t)I.n * 4) : nullptr;
        if (packed == 2) {  // the chunk's creates' handles at their ordinals (copied back at the batch's end)
            launch_ingest_new_handles(I, new_dst, (uint32_t)std::min<size_t>(new_cap, new_map ? new_cap : G.recs.cap), rs);
            HIPCHK(e, hipGetLastError());
        }
        const bool mapped = e->results_kernel && (!out_handles || mh) && (!out_status || ms) && (!out_status8 || m8) &&
                            (!out_released || mr);
        if (mapped) {
            launch_ingest_results(I, mh, ms, m8, mr, rs);
            HIPCHK(e, hipGetLastError());
            HIPCHK(e, hipEventRecord(e->fence, rs));  // (system-scope release: the host reads them)
            return KWOK_OK;
        }
        if (out_handles) HIPCHK(e, hipMemcpyAsync(out_handles + lo, I.out_handle, (size_t)I.n * 4, hipMemcpyDeviceToHost, rs));
        if (out_status) HIPCHK(e, hipMemcpyAsync(out_status + lo, I.out_status, (size_t)I.n * 4, hipMemcpyDeviceToHost, rs));
        if (out_status8) {  // one byte per record over the link
            launch_ingest_status8(I, G.out_status8 + lo, rs);
            HIPCHK(e, hipGetLastError());
            HIPCHK(e, hipMemcpyAsync(out_status8 + lo, G.out_status8 + lo, I.n, hipMemcpyDeviceToHost, rs));
        }
        if (out_released)
            HIPCHK(e, hipMemcpyAsync(out_released + lo, I.out_released, (size_t)I.n * 4, hipMemcpyDeviceToHost, rs));
        return KWOK_OK;
    };
    // The whole batch is queued without a host round trip per chunk: each chunk's
    // growth check (k_ing_need), sort and apply pass go behind its prep, and the
    // apply pass itself returns when the chunk needs more pod slots than a bucket
    // has (or an earlier chunk did).  One read-back of the chunks' summaries at the
    // end: the rare chunk that needs growth and the chunks after it are then applied
    // again with the host in the loop (ingest_chunk), in order.
    // an open pod session (kwok_watch.h): the chunk's final results mark their pods, behind its apply
    // pass on the engine stream and before its buffers' next use (spec: as the pass, nothing when the
    // chunk returned for growth; the redo marks then)
    auto mark_seen = [&](IngestBatch I, bool spec) -> int {
        if (!e->resync.open[KWOK_KIND_PODS]) return KWOK_OK;
        I.spec = spec ? 1u : 0u;
        launch_seen_mark_pods(e->S, I, e->resync.pod_seen, e->resync.ctr, st);
        HIPCHK(e, hipGetLastError());
        return KWOK_OK;
    };
    // the uid directory, while enabled: behind the apply pass of every pod chunk its creates take their
    // uid (a by-uid batch: and a table entry) or lose the slot's previous one (k: the chunk)
    auto note_uid = [&](IngestBatch I, bool spec, uint32_t k) -> int {
        if (!e->uid.on) return KWOK_OK;
        I.spec = spec ? 1u : 0u;
        UidNote N{};
        if (e->uid.note) {
            const size_t lo = lo_of(k);
            N = *e->uid.note;
            N.uoff += lo, N.ulen += lo, N.hash += lo, N.cls += lo;
        }
        hipEvent_t pe[2] = {};
        if (e->iprof && e->uid.note && hipEventCreate(&pe[0]) == hipSuccess && hipEventCreate(&pe[1]) == hipSuccess) {
            e->uid.note_ev.push_back(pe[0]);
            e->uid.note_ev.push_back(pe[1]);
            (void)hipEventRecord(pe[0], st);
        }
        launch_uid_note(e->S, I, e->uid.dir(), N, st);
        if (pe[1]) (void)hipEventRecord(pe[1], st);
        if (e->refs.on) {  // the reference directory: the creates' namespaces and names, or none
            RefNote RN{};
            if (e->refs.note) {
                const size_t lo = lo_of(k);
                RN = *e->refs.note;
                RN.frame_idx += lo, RN.cls += lo;
            }
            launch_refs_note(e->S, I, e->ref_dir(), RN, st);
        }
        HIPCHK(e, hipGetLastError());
        return KWOK_OK;
    };
    int tick_k = -1;  // tick mode: the slot of the tick queued behind the batch
    auto run = [&]() -> int {
        HIPCHK(e, hipEventRecord(G.go, st));
        if (arena_len && !zar && !resident) {  // (the arena ahead of the records: prep reads both)
            HIPCHK(e, hipStreamWaitEvent(ps, G.go, 0));  // (its buffer's zeroing, if just allocated)
            HIPCHK(e, hipMemcpyAsync(G.d_arena, arena, arena_len, hipMemcpyHostToDevice, ps));
        }
        for (uint32_t k = 0; k < std::min<uint32_t>(K, 2); k++)
            if (int r = prep(k)) return r;
        HIPCHK(e, hipMemsetAsync(G.abort, 0, 4, st));
        // (tick mode: the results always on their own stream, the tick's launches on the engine's)
        hipStream_t rs = (K > 1 && e->results_stream) || tick_now >= 0 ? G.dst : st;
        for (uint32_t k = 0; k < K; k++) {
            const IngestBatch I = chunk_batch(k);
            HIPCHK(e, hipStreamWaitEvent(st, G.prepped[k & 1], 0));
            if (e->debug_fail_chunk == k + 1) return e->fail(KWOK_EDEVICE, "injected failure of ingest chunk %u", k);
            if (int r = enqueue_sort_need(e, I)) return r;
            if (int r = enqueue_apply(e, I, true)) return r;
            if (int r = mark_seen(I, true)) return r;
            if (int r = note_uid(I, true, k)) return r;
            if (tstamp) HIPCHK(e, hipEventRecord(G.tev[4 + k], st));  // 4 / 5: chunk k applied
            // chunk k's results on the results stream; its accumulator set free for chunk k + 2
            HIPCHK(e, hipEventRecord(G.used[k & 1], st));
            if (rs != st) HIPCHK(e, hipStreamWaitEvent(rs, G.used[k & 1], 0));
            if (int r = results(k, rs)) return r;
            if (k + 2 < K)
                if (int r2 = prep(k + 2)) return r2;
        }
        if (int r = release_for_host(e)) return r;
        if (tick_now >= 0) {
            // the tick, right behind the last apply pass (its kernels run while the results
            // travel); every launch of it skips while G.abort says a chunk needs growth
            HIPCHK(e, hipMemcpyAsync(&e->S.bar->skip, G.abort, 4, hipMemcpyDeviceToDevice, st));
            if (int r = tick_submit_impl(e, tick_now)) return r;
            tick_k = e->queue[e->nq - 1];
        }
        // the host waits for the results stream alone when the tick is behind the batch
        hipStream_t ws = tick_now >= 0 ? rs : st;
        if (packed == 2) {  // the creates' handles (every chunk's), and the summaries after them (n_new)
            if (new_map) HIPCHK(e, hipEventRecord(e->fence, rs));  // (system-scope release: the host reads them)
            else HIPCHK(e, hipMemcpyAsync(out_new, G.new_handle, std::min(new_cap, n) * 4, hipMemcpyDeviceToHost, rs));
            if (rs != st && ws == st) {
                HIPCHK(e, hipEventRecord(G.rdone, rs));
                HIPCHK(e, hipStreamWaitEvent(st, G.rdone, 0));
            }
        }
        if (packed != 2 && rs != st && ws == st) {  // (the results stream joins the engine stream: one wait below)
            HIPCHK(e, hipEventRecord(G.rdone, rs));
            HIPCHK(e, hipStreamWaitEvent(st, G.rdone, 0));
        }
        // (tick mode: rs waited for the last apply pass, whose summary is then final)
        HIPCHK(e, hipMemcpyAsync(G.sums_h, G.sums, (size_t)K * sizeof(IngSummary), hipMemcpyDeviceToHost, ws));
        if (tstamp) HIPCHK(e, hipEventRecord(G.tev[6], rs));  // 6: results copied
        const auto tq = clk::now();
        if (e->sync_spin) {  // spin on the batch's last operation (as a tick's completion: no wake-up latency)
            HIPCHK(e, hipEventRecord(G.idone, ws));
            hipError_t q;
            while ((q = hipEventQuery(G.idone)) == hipErrorNotReady) {
            }
            if (q != hipSuccess) return e->fail(KWOK_EDEVICE, "ingest: %s", hipGetErrorString(q));
        } else {
            HIPCHK(e, hipStreamSynchronize(ws));
        }
        t_synced = clk::now();
        if (tstamp) {
            float ms[6] = {};
            for (int q = 1; q < 7; q++) (void)hipEventElapsedTime(&ms[q - 1], G.tev[0], G.tev[q]);
            fprintf(stderr, "[kwok ingest]   queued in %.3f ms; device from chunk 0's copy: prep0 %.3f, copy1 start %.3f, "
                            "prep1 %.3f, apply0 %.3f, apply1 %.3f, results %.3f ms\n", ms_between(t0, tq), ms[0], ms[1],
                    ms[2], ms[3], ms[4], ms[5]);
        }
        if (e->iprof) fprintf(stderr, "[kwok ingest]   %u chunk%s queued and applied +%.3f ms\n", K, K == 1 ? "" : "s",
                              ms_between(t0, clk::now()));
        int rejected = 0;
        uint32_t k = 0;
        for (; k < K; k++) {
            const IngSummary& q = G.sums_h[k];
            if (q.need > e->Cp) break;  // its pass (and every later chunk's) returned: growth first
            rejected += (int)q.rejected;
            if (q.foreign) e->foreign_ips = true;
            if (e->debug_fail_apply == k + 1)
                return e->fail(KWOK_EDEVICE, "injected failure after the apply pass of ingest chunk %u", k);
        }
        const bool regrow = k < K;
        for (; k < K; k++) {  // chunks from the first that needs growth: the host in the loop
            if (e->iprof) fprintf(stderr, "[kwok ingest]   chunk %u again with the growth check\n", k);
            if (int r = prep_on(k, st)) return r;
            e->ing_chunk = k;
            const int r = ingest_chunk(e, chunk_batch(k));
            if (r < 0) return r;
            if (int r2 = mark_seen(chunk_batch(k), false)) return r2;
            if (int r2 = note_uid(chunk_batch(k), false, k)) return r2;
            if (e->debug_fail_apply == k + 1)
                return e->fail(KWOK_EDEVICE, "injected failure after the apply pass of ingest chunk %u", k);
            rejected += r;
            if (int r2 = results(k, st)) return r2;
            if (packed == 2 && k + 1 == K) {
                if (new_map) HIPCHK(e, hipEventRecord(e->fence, st));
                else HIPCHK(e, hipMemcpyAsync(out_new, G.new_handle, std::min(new_cap, n) * 4, hipMemcpyDeviceToHost, st));
                HIPCHK(e, hipMemcpyAsync(G.sums_h + k, G.sums + k, sizeof(IngSummary), hipMemcpyDeviceToHost, st));
            }
            HIPCHK(e, hipStreamSynchronize(st));
        }
        if (regrow && tick_k >= 0) {  // the tick's launches skipped: queued again behind the chunks
            kwok_engine::TickSlot& T = e->slots[tick_k];
            if (int r = grow_arena(e, T)) return r;  // (the growth may have raised the tick's worst case)
            memset(T.hdr_h, 0, sizeof(TickHdr));
            HIPCHK(e, hipMemsetAsync(&e->S.bar->skip, 0, sizeof(uint32_t), st));
            if (int r = enqueue_tick(e, tick_k, true)) return r;
        }
        return rejected;
    };
    rc = run();
    // kwok_pod_rec12 with more creates than out_new_handles holds: the batch is applied
    // (not a failure of the engine), the call reports the lost handles.  A batch that
    // fails once it changed the state (a chunk applied, or the failing chunk's own
    // apply pass, placeholders or growth) is partly in the state: every later call fails
    if (rc >= 0 && packed == 2 && G.sums_h[K - 1].n_new > new_cap)
        rc = e->fail(KWOK_EINVAL, "kwok_ingest_pods_packed12: %u creates, out_new_handles holds %zu",
                     G.sums_h[K - 1].n_new, new_cap);
    else if (rc < 0 && e->ing_mutated)
        e->poisoned = true;
    if (rc < 0 && tick_k >= 0 && e->poisoned) {  // the tick behind a batch that failed half applied fails with it
        kwok_engine::TickSlot& T = e->slots[tick_k];
        if (T.state == SLOT_QUEUED) {
            (void)hipStreamSynchronize(st);
            T.state = SLOT_DONE;
            T.rc = rc;
            T.err = e->err;
        }
    }
    // nothing of this batch stays queued on the engine / prep / results streams (a failed
    // chunk included; a batch that ran to its end synchronised them in run(): the engine
    // stream's applies waited for every prep, the results stream was synchronised)
    if (rc < 0) {
        if (hipStreamSynchronize(st) != hipSuccess && rc >= 0) rc = e->fail(KWOK_EDEVICE, "ingest engine stream");
        if (hipStreamSynchronize(ps) != hipSuccess && rc >= 0) rc = e->fail(KWOK_EDEVICE, "ingest prep stream");
        if (hipStreamSynchronize(G.dst) != hipSuccess && rc >= 0) rc = e->fail(KWOK_EDEVICE, "ingest results stream");
    }
    if (e->iprof)
        fprintf(stderr, "[kwok ingest] %zu pod records (GPU%s, %u chunk%s%s): %.3f ms (first copy queued at %.3f, synced at %.3f)\n",
                n, zev ? ", read in place" : "", K, K == 1 ? "" : "s",
                packed == 2 ? (new_map ? ", create handles mapped" : ", create handles copied") : "", ms_between(t0, clk::now()),
                ms_between(t0, t_copy0), ms_between(t0, t_synced));
    return rc;
}

int kwok_ingest_pods(kwok_engine* e, const kwok_pod_event* ev, size_t n, const char* arena, size_t arena_len,
                     int32_t* out_handles, int32_t* out_status, uint32_t* out_released) {
    if (!e || (n && !ev) || n > 0x7FFFFFF0ull || (arena_len && !arena)) return KWOK_EINVAL;
    return ingest_pods_impl(e, ev, 0, n, arena, arena_len, out_handles, out_status, nullptr, out_released);
}

int kwok_ingest_pods_packed(kwok_engine* e, const kwok_pod_rec* recs, size_t n, int32_t* out_handles, int8_t* out_status,
                            uint32_t* out_released) {
    if (!e || (n && !recs) || n > 0x7FFFFFF0ull) return KWOK_EINVAL;
    return ingest_pods_impl(e, recs, 1, n, nullptr, 0, out_handles, nullptr, out_status, out_released);
}

int kwok_ingest_pods_packed12(kwok_engine* e, const kwok_pod_rec12* recs, size_t n, int32_t* out_new_handles,
                              size_t new_cap, int8_t* out_status, uint32_t* out_released) {
    if (!e || (n && !recs) || n > 0x7FFFFFF0ull || (new_cap && !out_new_handles)) return KWOK_EINVAL;
    return ingest_pods_impl(e, recs, 2, n, nullptr, 0, nullptr, nullptr, out_status, out_released, false,
                            out_new_handles, new_cap);
}

int kwok_ingest_pods_packed12_tick(kwok_engine* e, const kwok_pod_rec12* recs, size_t n, int32_t* out_new_handles,
                                   size_t new_cap, int8_t* out_status, uint32_t* out_released, int64_t now_unix) {
    if (!e || (n && !recs) || n > 0x7FFFFFF0ull || (new_cap && !out_new_handles) || now_unix < 0) return KWOK_EINVAL;
    return ingest_pods_impl(e, recs, 2, n, nullptr, 0, nullptr, nullptr, out_status, out_released, false,
                            out_new_handles, new_cap, now_unix);
}

// ---- the pod codec on the GPU (json.hip) ------------------------------------
namespace {
int json_reserve(kwok_engine* e, size_t n) {
    auto& J = e->json;
    if (!J.cfg) {
        int rc = 0;
        if ((rc = dalloc(e, &J.cfg, 1)) || (rc = dalloc(e, &J.n_host, 1))) return rc;
        if (hipHostMalloc((void**)&J.cfg_h.p, sizeof(JsonCfg), hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc((void**)&J.n_host_h.p, sizeof(uint32_t), hipHostMallocDefault) != hipSuccess)
            return e->fail(KWOK_ENOMEM, "GPU codec staging");
    }
    if (int rc = J.docs.reserve(e, n)) return rc;
    if (J.tab_dirty) {  // the spec table: open addressing at <= 50% load, rebuilt from spec_keys
        uint32_t slots = 1024;
        while (slots < 2 * e->spec_keys.size() + 2) slots <<= 1;
        if (slots - 1 != J.tab_mask || !J.tab_key) {
            dfree(J.tab_key), dfree(J.tab_id), dfree(J.tab_canon);
            int rc = 0;
            if ((rc = dalloc(e, &J.tab_key, slots)) || (rc = dalloc(e, &J.tab_id, slots)) ||
                (rc = dalloc(e, &J.tab_canon, slots)))
                return rc;
            J.tab_mask = slots - 1;
        }
        std::vector<uint64_t> key(slots, 0);
        std::vector<int32_t> id(slots, -1);
        std::vector<uint2> cref(slots, uint2{0, 0});
        std::string canon;
        for (auto& kv : e->spec_keys) {
            uint64_t k = kv.first ? kv.first : 1;  // (0 marks an empty slot: key 0 is never found)
            if (!kv.first) continue;
            uint32_t h = (uint32_t)k & J.tab_mask;
            while (key[h]) h = (h + 1) & J.tab_mask;
            key[h] = k;
            id[h] = kv.second;
            const std::string& c = e->spec_canon[kv.first];
            cref[h] = uint2{(uint32_t)canon.size(), (uint32_t)c.size()};
            canon += c;
        }
        if (int rc = J.canon_bytes.reserve(e, canon.size() + 16, 2 * canon.size() + 16)) return rc;
        HIPCHK(e, hipMemcpyAsync(J.tab_key, key.data(), slots * 8, hipMemcpyHostToDevice, e->st));
        HIPCHK(e, hipMemcpyAsync(J.tab_id, id.data(), slots * 4, hipMemcpyHostToDevice, e->st));
        HIPCHK(e, hipMemcpyAsync(J.tab_canon, cref.data(), slots * sizeof(uint2), hipMemcpyHostToDevice, e->st));
        if (!canon.empty()) HIPCHK(e, hipMemcpyAsync(J.canon, canon.data(), canon.size(), hipMemcpyHostToDevice, e->st));
        HIPCHK(e, hipStreamSynchronize(e->st));
        J.tab_dirty = false;
    }
    return KWOK_OK;
}

// decode documents [0, n) on the device: the arena and the spans go to the ingest
// buffers, k_json_pods writes the records there (ingest form when op != null);
// returns the number of documents listed for the host (JSON_HOST / JSON_SPEC)
int json_decode(kwok_engine* e, const kwok_codec* c, const char* arena, size_t arena_len, const uint64_t* doc_off,
                const uint32_t* doc_len, size_t n, const uint8_t* op, const int32_t* handle, uint32_t* n_host,
                const uint8_t* resident = nullptr, bool dev_inputs = false) {
    // resident: the documents are on the device already, at this address (the watch
    // stream, kwok_ingest_pods_framed): nothing is copied, one decode launch
    // dev_inputs (with resident): the spans, ops and handles are in the codec's device
    // buffers already (k_uid_resolve wrote them); the four host arrays are not read
    auto& G = e->ing;
    auto& J = e->json;
    hipStream_t st = e->st;
    int rc = ingest_reserve(e, n, resident ? 0 : arena_len + 16);  // (the scanner reads whole 16-byte windows)
    if (rc) return rc;
    if ((rc = json_reserve(e, n))) return rc;
    // selectors beyond the device's tables (JSEL_*): every document is decoded by the
    // host codec (JSON_HOST), as any other document the scanner does not decide
    if ((rc = codec_export(c, J.cfg_h))) {
        if (rc != KWOK_EDOMAIN) return e->fail(rc, "%s", kwok_codec_last_error());
        memset(J.cfg_h, 0, sizeof(JsonCfg));
        J.cfg_h->all_host = 1;
    }
    HIPCHK(e, hipMemcpyAsync(J.cfg, J.cfg_h, sizeof(JsonCfg), hipMemcpyHostToDevice, st));
    if (!dev_inputs) {
        HIPCHK(e, hipMemcpyAsync(J.off, doc_off, n * 8, hipMemcpyHostToDevice, st));
        HIPCHK(e, hipMemcpyAsync(J.len, doc_len, n * 4, hipMemcpyHostToDevice, st));
    }
    const bool ingest = op || dev_inputs;
    if (op && !dev_inputs) {
        HIPCHK(e, hipMemcpyAsync(J.op, op, n, hipMemcpyHostToDevice, st));
        HIPCHK(e, hipMemcpyAsync(J.handle, handle, n * 4, hipMemcpyHostToDevice, st));
    }
    HIPCHK(e, hipMemsetAsync(J.n_host, 0, 4, st));
    // Documents in arena order (offsets non-decreasing, the usual batch): the arena
    // crosses the link in K pieces on the prep stream, and each piece's documents
    // are decoded on the engine stream as soon as it has landed - the decode runs
    // under the copy, which bounds the call (the link: ~2.7 GB per C4 tick).
    // Otherwise one copy, then one decode.
    bool sorted = true;
    for (size_t i = 1; i < n && sorted && !dev_inputs; i++) sorted = doc_off[i] >= doc_off[i - 1] + doc_len[i - 1];
    const uint32_t K = !resident && sorted && arena_len > (64u << 20) ? (uint32_t)std::min<size_t>(8, n / 4096 + 1) : 1u;
    hipStream_t ps = G.pst;
    HIPCHK(e, hipEventRecord(G.go, st));  // the copies start after the engine stream's earlier work
    HIPCHK(e, hipStreamWaitEvent(ps, G.go, 0));
    const bool tprof = e->iprof && G.tev[0];
    if (tprof) HIPCHK(e, hipEventRecord(G.tev[0], ps));
    uint64_t copied = 0;
    for (uint32_t k = 0; k < K; k++) {
        const size_t d0 = n * k / K, d1 = n * (k + 1) / K;
        const uint64_t hi = k + 1 == K ? arena_len : std::min<uint64_t>(arena_len, doc_off[d1 - 1] + doc_len[d1 - 1]);
        if (hi > copied && !resident) {
            HIPCHK(e, hipMemcpyAsync(G.d_arena + copied, arena + copied, hi - copied, hipMemcpyHostToDevice, ps));
            copied = hi;
        }
        HIPCHK(e, hipEventRecord(G.prepped[k & 1], ps));
        HIPCHK(e, hipStreamWaitEvent(st, G.prepped[k & 1], 0));
        JsonPodArgs A{};
        A.arena = resident ? resident : G.d_arena;
        A.arena_len = arena_len;
        A.doc_off = J.off + d0;
        A.doc_len = J.len + d0;
        A.n = (uint32_t)(d1 - d0);
        A.base = (uint32_t)d0;
        A.tab_mask = J.tab_mask;
        A.cfg = J.cfg;
        A.op = ingest ? J.op + d0 : nullptr;
        A.handle = ingest ? J.handle + d0 : nullptr;
        A.tab_key = J.tab_key;
        A.tab_id = J.tab_id;
        A.tab_canon = J.tab_canon;
        A.key_mask = spec_key_mask();
        A.canon = J.canon;
        A.ev = static_cast<kwok_pod_event*>(G.d_ev.p) + d0;
        A.side = J.side + d0;
        A.host_list = J.host_list;
        A.n_host = J.n_host;
        launch_json_pods(A, st);
        HIPCHK(e, hipGetLastError());
    }
    if (tprof) HIPCHK(e, hipEventRecord(G.tev[1], ps));
    if (tprof) HIPCHK(e, hipEventRecord(G.tev[2], st));
    HIPCHK(e, hipMemcpyAsync(J.n_host_h, J.n_host, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    *n_host = *J.n_host_h;
    if (tprof) {
        float c = 0, d = 0;
        (void)hipEventElapsedTime(&c, G.tev[0], G.tev[1]);
        (void)hipEventElapsedTime(&d, G.tev[0], G.tev[2]);
        fprintf(stderr, "[kwok json]   %u piece%s: copies %.3f ms (%.1f GB/s), decoded %.3f ms after the first copy\n", K,
                K == 1 ? "" : "s", c, arena_len / (c * 1e6), d);
    }
    return KWOK_OK;
}

// the documents the scanner listed: decoded by the host codec (JSON_HOST), or their
// spec registered (JSON_SPEC: one host decode per new spec key); their records
// completed and written back.  ingest: the records take the caller's op / handle
// and a spec id (kwok_ingest_pods_json); else they stay as the codec writes them
// (names / spec keys back in names_ns / spec_key of the caller, indexed by document).
int json_complete(kwok_engine* e, const kwok_codec* c, const char* arena, size_t arena_len, const uint64_t* doc_off,
                  const uint32_t* doc_len, uint32_t nh, const uint8_t* op, const int32_t* handle,
                  std::vector<JsonPodSide>* sides_out, std::vector<uint32_t>* list_out) {
    auto& G = e->ing;
    auto& J = e->json;
    hipStream_t st = e->st;
    if (!nh) return KWOK_OK;
    std::vector<uint32_t> list(nh);
    std::vector<kwok_pod_event> ev(nh);
    std::vector<JsonPodSide> side(nh);
    launch_json_gather(static_cast<const kwok_pod_event*>(G.d_ev.p), J.side, J.host_list, nh, J.fix_ev, J.fix_side, st);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(list.data(), J.host_list, (size_t)nh * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(ev.data(), J.fix_ev, (size_t)nh * sizeof(kwok_pod_event), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(side.data(), J.fix_side, (size_t)nh * sizeof(JsonPodSide), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    // specs registered here (JSON_SPEC), by both of the device's keys of their
    // canonical string (kwok_spec_key and a second, independent 64-bit hash): a later
    // document of the batch with both keys takes that spec without a host decode
    struct K2Hash {
        size_t operator()(const std::pair<uint64_t, uint64_t>& k) const { return (size_t)(k.first ^ (k.second * 31)); }
    };
    std::unordered_map<std::pair<uint64_t, uint64_t>, int32_t, K2Hash> fresh;
    char* ar = const_cast<char*>(arena);  // (kwok_decode_pod writes only node blobs)
    kwok_pod_doc d;
    // in document order (the device wrote the list in the order its atomics landed): spec ids, and which
    // documents meet KWOK_EFULL, are then those of the host path; the scatter takes any order
    std::vector<uint32_t> order(nh);
    for (uint32_t q = 0; q < nh; q++) order[q] = q;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return list[a] < list[b]; });
    for (uint32_t q : order) {
        const uint32_t i = list[q];
        JsonPodSide& s = side[q];
        const bool ups = !op || op[i] == KWOK_OP_UPSERT;
        const std::pair<uint64_t, uint64_t> dkey{s.spec_key, s.spec_key2};  // (the device's, before the host decode)
        const bool miss = s.status == JSON_SPEC;  // (JSON_SPEC_X, a key that collides with a registered spec: decoded)
        if (miss) {
            auto f = fresh.find(dkey);
            if (f != fresh.end()) {
                ev[q].spec_id = f->second;
                ev[q].reserved0 = 0;
                s.status = KWOK_OK;
                continue;
            }
        }
        // the host codec decides this document (a new spec: one decode registers it)
        int rc = kwok_decode_pod(c, ar, arena_len, doc_off[i], doc_len[i], &d);
        kwok_pod_event x = rc == KWOK_OK ? d.ev : kwok_pod_event{};
        int32_t id = -1;
        if (rc == KWOK_OK) {
            kwok_pod_spec sp{d.containers, d.n_containers, d.init_containers, d.n_init_containers,
                             d.readiness_gates, d.n_readiness_gates};
            s.name_off = d.name.off, s.name_len = d.name.len, s.ns_off = d.namespace_.off, s.ns_len = d.namespace_.len;
            s.n_cont = (uint8_t)d.n_containers, s.n_init = (uint8_t)d.n_init_containers;
            s.n_gates = (uint8_t)d.n_readiness_gates;
            s.spec_key = kwok_spec_key(&sp, arena, arena_len);
            if (op && ups) {
                const int r2 = kwok_register_pod_spec(e, &sp, arena, arena_len, &id);
                if (r2 == KWOK_OK) {
                    if (miss) fresh[dkey] = id;
                } else if (r2 == KWOK_EDOMAIN || r2 == KWOK_EFULL) {
                    rc = r2;  // the spec is outside the domain
                } else {
                    return r2;
                }
            }
        }
        if (op) {
            x.op = op[i];
            x.handle = handle[i];
            x.spec_id = ups ? id : -1;
            x.node_handle = -1;
            x.reserved0 = rc == KWOK_OK ? 0 : (uint8_t)(int8_t)rc;
        } else if (rc != KWOK_OK) {
            x = kwok_pod_event{};
        }
        ev[q] = x;
        s.status = rc;
    }
    HIPCHK(e, hipMemcpyAsync(J.fix_ev, ev.data(), (size_t)nh * sizeof(kwok_pod_event), hipMemcpyHostToDevice, st));
    launch_json_scatter(static_cast<kwok_pod_event*>(G.d_ev.p), J.fix_ev, J.host_list, nh, st);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(st));
    if (sides_out) *sides_out = std::move(side);
    if (list_out) *list_out = std::move(list);
    return KWOK_OK;
}
}  // namespace

uint64_t kwok_spec_key(const kwok_pod_spec* spec, const char* arena, size_t arena_len) {
    if (!spec) return 0;
    auto str = [&](kwok_str s) {
        return (size_t)s.off + s.len <= arena_len ? std::string(arena + s.off, s.len) : std::string();
    };
    std::vector<Container> cs(spec->n_containers), ics(spec->n_init_containers);
    std::vector<std::string> gates(spec->n_readiness_gates);
    for (uint32_t i = 0; i < spec->n_containers; i++) cs[i] = {str(spec->containers[i].name), str(spec->containers[i].image)};
    for (uint32_t i = 0; i < spec->n_init_containers; i++)
        ics[i] = {str(spec->init_containers[i].name), str(spec->init_containers[i].image)};
    for (uint32_t i = 0; i < spec->n_readiness_gates; i++) gates[i] = str(spec->readiness_gates[i]);
    return json_spec_key(cs, ics, gates);
}

// ---- node documents on the GPU (json.hip k_json_nodes) -----------------------
// kwok_ingest_nodes_json: WatchNodes / ListNodes from the documents themselves
// (node_controller.go:206-279): decoded on the device, the host codec only for
// the documents the scanner lists (a non-empty addresses / allocatable /
// capacity blob, whose canonical form is the host's, or an escaped routed
// string), then kwok_ingest_nodes' GPU event switch over the records, which
// stay on the device.  With kwok_canon_enable the blobs of a document inside the
// device domain are canonicalised there (json_nodes_canon): no host codec call.
namespace {
// ---- the status blob canonicaliser (kwok_canon.h, json.hip k_canon) ----
// Before a scan of n documents with the switch on: the canon list and the counters, zeroed.
int canon_reserve(kwok_engine* e, size_t n) {
    auto& C = e->canon;
    if (!C.ctr) {
        if (int rc = dalloc(e, &C.ctr, 1)) return rc;
        if (hipHostMalloc((void**)&C.ctr_h.p, sizeof(CanonCounters), hipHostMallocDefault) != hipSuccess)
            return e->fail(KWOK_ENOMEM, "canonicaliser staging");
    }
    if (int rc = C.docs.reserve(e, n)) return rc;
    HIPCHK(e, hipMemsetAsync(C.ctr, 0, sizeof(CanonCounters), e->st));
    return KWOK_OK;
}
// Behind the scan's launches (every piece of d_arena has landed before the last of them): the listed count
// comes back; if there is any, the raw lengths, their scan, k_canon over the list, then the pairs and the
// canonical bytes to the host (canon.doc_h sorted by document, canon.bytes_h).  The documents k_canon found
// outside its domain are on json.host_list with status JSON_HOST when it returns.  Synchronises.
int json_nodes_canon(kwok_engine* e, const uint8_t* d_arena) {
    auto& C = e->canon;
    auto& J = e->json;
    hipStream_t st = e->st;
    const auto t0 = clk::now();
    HIPCHK(e, hipMemcpyAsync(C.ctr_h, C.ctr, sizeof(CanonCounters), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    const uint32_t nc = C.ctr_h->n;
    const uint64_t raw = C.ctr_h->raw;
    if (!nc) return KWOK_OK;
    if (nc > C.docs.cap) return e->fail(KWOK_EDEVICE, "canonicaliser: %u documents listed, room for %zu", nc, C.docs.cap);
    int rc = 0;
    if ((rc = C.out.reserve(e, (size_t)raw))) return rc;
    const size_t tmp = refs_scan_bytes(nc);
    if (tmp > C.tmp_bytes) {
        C.tmp.release(), C.tmp_bytes = 0;
        const size_t want = tmp + tmp / 4 + 256;
        if (hipMalloc(&C.tmp.p, want) != hipSuccess) return e->fail(KWOK_ENOMEM, "canonicaliser: scan storage");
        C.tmp_bytes = want;
    }
    ProfEvents<2> pev(e->iprof, st);
    pev.stamp(0);
    launch_canon_len(e->ing.d_nev, C.list, nc, C.len, st);
    if (launch_scan64(C.len, C.off, nc, C.tmp, C.tmp_bytes, st)) return e->fail(KWOK_EDEVICE, "canonicaliser: scan");
    CanonArgs A{};
    A.arena = d_arena;
    A.ev = e->ing.d_nev;
    A.status = J.nstat;
    A.list = C.list;
    A.n = nc;
    A.off = C.off;
    A.out = C.bytes;
    A.docs = C.doc;
    A.host_list = J.host_list;
    A.n_host = J.n_host;
    launch_canon(A, st);
    HIPCHK(e, hipGetLastError());
    pev.stamp(1);
    C.doc_h.resize(nc);
    C.bytes_h.resize((size_t)raw);
    HIPCHK(e, hipMemcpyAsync(C.doc_h.data(), C.doc, (size_t)nc * sizeof(CanonDoc), hipMemcpyDeviceToHost, st));
    if (raw) HIPCHK(e, hipMemcpyAsync(C.bytes_h.data(), C.bytes, (size_t)raw, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    std::sort(C.doc_h.begin(), C.doc_h.end(), [](const CanonDoc& a, const CanonDoc& b) { return a.doc < b.doc; });
    uint64_t docs = 0, blobs = 0, in = 0, out = 0;
    for (const CanonDoc& d : C.doc_h) {
        if (d.host) continue;
        docs++;
        for (int j = 0; j < 3; j++) {
            if ((uint64_t)d.off[j] + d.len[j] > raw || d.len[j] > d.raw[j])
                return e->fail(KWOK_EDEVICE, "canonicaliser: a blob outside the canonical buffer");
            blobs += d.len[j] != 0, in += d.len[j] ? d.raw[j] : 0, out += d.len[j];
        }
    }
    C.stats[KWOK_CANON_STAT_DOCS] += docs;
    C.stats[KWOK_CANON_STAT_BLOBS] += blobs;
    C.stats[KWOK_CANON_STAT_BYTES_IN] += in;
    C.stats[KWOK_CANON_STAT_BYTES_OUT] += out;
    C.stats[KWOK_CANON_STAT_DOCS_HOST] += nc - docs;
    C.stats[KWOK_CANON_STAT_CALLS]++;
    if (e->iprof)
        fprintf(stderr, "[kwok canon]  %u documents listed, %llu canonicalised (%llu blobs, %llu -> %llu bytes), %llu to the host: "
                        "lengths + scan + k_canon %.3f ms on the device, the call %.3f ms\n", nc, (unsigned long long)docs,
                (unsigned long long)blobs, (unsigned long long)in, (unsigned long long)out, (unsigned long long)(nc - docs),
                pev.elapsed(0, 1), ms_between(t0, clk::now()));
    return KWOK_OK;
}
// documents [0, n) decoded on the device: records in ing.d_nev (op: the caller's, or
// KWOK_OP_UPSERT when op is null; 0xFF for a document not decided there), the
// decode statuses into dstat, the number listed for the host (json.host_list) in *nh.
// With the canonicaliser on a record holds its blobs' raw spans; the canonical bytes
// are in canon.doc_h / bytes_h
int json_nodes_decode(kwok_engine* e, const kwok_codec* c, const char* arena, size_t arena_len, const uint64_t* doc_off,
                      const uint32_t* doc_len, const uint8_t* op, size_t n, std::vector<int32_t>& dstat, uint32_t* nh,
                      const uint8_t* resident = nullptr) {  // (resident: as json_decode's)
    const auto t0 = clk::now();
    int rc = node_reserve(e, n, resident ? 0 : arena_len + 16);  // (the scanner reads whole 16-byte windows)
    if (rc) return rc;
    if ((rc = json_reserve(e, n))) return rc;
    auto& G = e->ing;
    auto& J = e->json;
    if ((rc = J.node_docs.reserve(e, n))) return rc;
    auto& C = e->canon;
    C.doc_h.clear();
    if (C.on && (rc = canon_reserve(e, n))) return rc;
    hipStream_t st = e->st, ps = G.pst;
    if ((rc = codec_export(c, J.cfg_h))) {  // (selectors beyond the device tables: every document to the host)
        if (rc != KWOK_EDOMAIN) return e->fail(rc, "%s", kwok_codec_last_error());
        memset(J.cfg_h, 0, sizeof(JsonCfg));
        J.cfg_h->all_host = 1;
    }
    HIPCHK(e, hipMemcpyAsync(J.cfg, J.cfg_h, sizeof(JsonCfg), hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(J.off, doc_off, n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(J.len, doc_len, n * 4, hipMemcpyHostToDevice, st));
    if (op) HIPCHK(e, hipMemcpyAsync(J.op, op, n, hipMemcpyHostToDevice, st));
    else HIPCHK(e, hipMemsetAsync(J.op, KWOK_OP_UPSERT, n, st));
    HIPCHK(e, hipMemsetAsync(J.n_host, 0, 4, st));
    // the arena in pieces on the prep stream, each piece's documents decoded as it lands
    bool sorted = true;
    for (size_t i = 1; i < n && sorted; i++) sorted = doc_off[i] >= doc_off[i - 1] + doc_len[i - 1];
    const uint32_t K = !resident && sorted && arena_len > (64u << 20) ? (uint32_t)std::min<size_t>(8, n / 4096 + 1) : 1u;
    HIPCHK(e, hipEventRecord(G.go, st));
    HIPCHK(e, hipStreamWaitEvent(ps, G.go, 0));
    uint64_t copied = 0;
    for (uint32_t k = 0; k < K; k++) {
        const size_t d0 = n * k / K, d1 = n * (k + 1) / K;
        const uint64_t hi = k + 1 == K ? arena_len : std::min<uint64_t>(arena_len, doc_off[d1 - 1] + doc_len[d1 - 1]);
        if (hi > copied && !resident) {
            HIPCHK(e, hipMemcpyAsync(G.d_arena + copied, arena + copied, hi - copied, hipMemcpyHostToDevice, ps));
            copied = hi;
        }
        HIPCHK(e, hipEventRecord(G.prepped[k & 1], ps));
        HIPCHK(e, hipStreamWaitEvent(st, G.prepped[k & 1], 0));
        JsonNodeArgs A{};
        A.arena = resident ? resident : G.d_arena;
        A.arena_len = arena_len;
        A.doc_off = J.off + d0;
        A.doc_len = J.len + d0;
        A.op = J.op + d0;
        A.n = (uint32_t)(d1 - d0);
        A.cfg = J.cfg;
        A.ev = G.d_nev + d0;
        A.status = J.nstat + d0;
        A.host_list = J.host_list;
        A.n_host = J.n_host;
        A.base = (uint32_t)d0;
        A.canon_list = C.on ? C.list.p : nullptr;
        A.canon_ctr = C.ctr;
        launch_json_nodes(A, st);
        HIPCHK(e, hipGetLastError());
    }
    if (C.on && (rc = json_nodes_canon(e, resident ? resident : G.d_arena))) return rc;
    const auto tq = clk::now();
    dstat.resize(n);
    HIPCHK(e, hipMemcpyAsync(dstat.data(), J.nstat, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(J.n_host_h, J.n_host, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    *nh = *J.n_host_h;
    if (e->iprof)
        fprintf(stderr, "[kwok json]   %zu node documents: queued %.3f ms, decoded + statuses back %.3f ms\n", n,
                ms_between(t0, tq), ms_between(tq, clk::now()));
    return KWOK_OK;
}
// the documents json_nodes_decode listed, sorted
int json_nodes_listed(kwok_engine* e, uint32_t nh, std::vector<uint32_t>& list) {
    list.resize(nh);
    if (!nh) return KWOK_OK;
    HIPCHK(e, hipMemcpyAsync(list.data(), e->json.host_list, (size_t)nh * 4, hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    std::sort(list.begin(), list.end());
    return KWOK_OK;
}
// The documents the device listed for the host (list: their batch indices, sorted): the host codec on a
// private copy of each (it writes the canonical blobs over their spans); their records to the device,
// spans moved to the batch's arena (the device only bounds-checks the blob spans: the host completion
// interns the canonical bytes from the private copy).  doc(i): document i's span in arena and its op.
// hstat[q]: the host decode's status of list[q]; hdoc / hrec / hbuf: what NodeJsonCtx carries on.
int nodes_complete_listed(kwok_engine* e, const kwok_codec* c, const char* arena, const std::vector<uint32_t>& list,
                          const std::function<void(uint32_t, uint64_t*, uint32_t*, uint8_t*)>& doc, std::vector<int32_t>& hstat,
                          std::unordered_map<uint32_t, uint32_t>& hdoc, std::vector<kwok_node_event>& hrec,
                          std::vector<std::string>& hbuf) {
    auto& G = e->ing;
    auto& J = e->json;
    hipStream_t st = e->st;
    const uint32_t nh = (uint32_t)list.size();
    std::vector<kwok_node_event> hdev(nh);
    hrec.assign(nh, kwok_node_event{});
    hbuf.assign(nh, std::string());
    hstat.assign(nh, KWOK_OK);
    const bool par = nh >= NODE_PAR_MIN && e->n_part > 1;
    run_parts(e, par, [&](int p) {
        const size_t lo = par ? (size_t)nh * p / e->n_part : (p ? nh : 0);
        const size_t hi = par ? (size_t)nh * (p + 1) / e->n_part : nh;
        for (size_t q = lo; q < hi; q++) {
            uint64_t off = 0;
            uint32_t len = 0;
            uint8_t op = KWOK_OP_UPSERT;
            doc(list[q], &off, &len, &op);
            hbuf[q].assign(arena + off, len);
            kwok_node_event x{};
            const int r = kwok_decode_node(c, hbuf[q].data(), hbuf[q].size(), 0, hbuf[q].size(), &x);
            hrec[q] = x;
            kwok_node_event d = x;
            auto mv = [&](kwok_str& s) {
                if (s.len) s.off += (uint32_t)off;
            };
            mv(d.name), mv(d.addresses), mv(d.allocatable), mv(d.capacity);
            for (int k = 0; k < KWOK_NI_COUNT; k++) mv(d.node_info[k]);
            d.op = r == KWOK_OK ? op : (uint8_t)0xFF;
            if (r != KWOK_OK) d.name = kwok_str{0, 0};
            hdev[q] = d;
            hstat[q] = r;
        }
    });
    for (uint32_t q = 0; q < nh; q++) hdoc.emplace(list[q], q);
    HIPCHK(e, hipMemcpyAsync(J.host_list, list.data(), (size_t)nh * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(J.nev_fix, hdev.data(), (size_t)nh * sizeof(kwok_node_event), hipMemcpyHostToDevice, st));
    launch_node_scatter(G.d_nev, J.nev_fix, J.host_list, nh, st);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(st));  // (hdev is read by the copy above)
    return KWOK_OK;
}
}  // namespace

// kwok_ingest_nodes_json: WatchNodes / ListNodes from the documents themselves
// (node_controller.go:206-279): decoded on the device, the host codec only for
// the documents the scanner lists (a non-empty addresses / allocatable /
// capacity blob, whose canonical form is the host's, or an escaped routed
// string), then kwok_ingest_nodes' GPU event switch over the records, which
// stay on the device.  With kwok_canon_enable the blobs of a document inside the
// device domain are canonicalised there (json_nodes_canon): no host codec call.
namespace {
int ingest_nodes_json_impl(kwok_engine* e, const kwok_codec* c, const char* arena, size_t arena_len,
                           const uint64_t* doc_off, const uint32_t* doc_len, const uint8_t* op, size_t n,
                           int32_t* out_handles, int32_t* out_status, size_t* n_host, const uint8_t* resident);
}
int kwok_ingest_nodes_json(kwok_engine* e, const kwok_codec* c, const char* arena, size_t arena_len,
                           const uint64_t* doc_off, const uint32_t* doc_len, const uint8_t* op, size_t n,
                           int32_t* out_handles, int32_t* out_status, size_t* n_host) {
    if (!e || !c || (n && (!doc_off || !doc_len || !op)) || (arena_len && !arena) || n > 0x7FFFFFF0ull ||
        arena_len > 0xFFFFFFF0ull)
        return KWOK_EINVAL;
    return ingest_nodes_json_impl(e, c, arena, arena_len, doc_off, doc_len, op, n, out_handles, out_status, n_host, nullptr);
}
namespace {
// resident: the documents are in the watch stream on the device (kwok_ingest_nodes_framed);
// arena is then the caller's copy of it, read for the documents the host completes
int ingest_nodes_json_impl(kwok_engine* e, const kwok_codec* c, const char* arena, size_t arena_len,
                           const uint64_t* doc_off, const uint32_t* doc_len, const uint8_t* op, size_t n,
                           int32_t* out_handles, int32_t* out_status, size_t* n_host, const uint8_t* resident) {
    if (e->poisoned) return poisoned(e);
    drain(e);
    if (e->poisoned) return poisoned(e);
    e->emit_hint = true;
    e->quiet = 0;
    e->state_changed();
    if (n_host) *n_host = 0;
    if (!n) return 0;
    const auto t0 = clk::now();
    std::vector<int32_t> dstat;
    uint32_t nh = 0;
    int rc = json_nodes_decode(e, c, arena, arena_len, doc_off, doc_len, op, n, dstat, &nh, resident);
    if (rc) return rc;
    // the listed documents, completed by the host codec
    std::unordered_map<uint32_t, uint32_t> hdoc;
    std::vector<kwok_node_event> hrec;
    std::vector<std::string> hbuf;
    if (nh) {
        std::vector<uint32_t> list;
        std::vector<int32_t> hstat;
        if ((rc = json_nodes_listed(e, nh, list))) return rc;
        if ((rc = nodes_complete_listed(e, c, arena, list, [&](uint32_t i, uint64_t* o, uint32_t* l, uint8_t* p) {
                *o = doc_off[i], *l = doc_len[i], *p = op[i];
            }, hstat, hdoc, hrec, hbuf)))
            return rc;
        for (uint32_t q = 0; q < nh; q++) dstat[list[q]] = hstat[q];
    }
    if (n_host) *n_host = nh;
    if (e->iprof)
        fprintf(stderr, "[kwok json] %zu node documents decoded on the GPU (%u by the host): %.2f ms\n", n, nh,
                ms_between(t0, clk::now()));
    NodeJsonCtx ctx{arena, &hdoc, &hrec, &hbuf, e->canon.on ? &e->canon : nullptr};
    std::vector<int32_t> stat(out_status ? 0 : n);
    int32_t* so = out_status ? out_status : stat.data();
    rc = ingest_nodes_impl(e, nullptr, n, arena, arena_len, out_handles, so, &ctx);
    if (rc < 0) return rc;
    for (size_t i = 0; i < n; i++)  // a document that failed to decode: its decode status
        if (dstat[i] != KWOK_OK) {
            so[i] = dstat[i];
            if (out_handles) out_handles[i] = -1;
        }
    return rc;
}
}  // namespace

// kwok_decode_nodes_gpu: the decode alone (tests): the records kwok_decode_nodes
// would write, the listed documents decoded by the host codec in place (it
// re-serialises their blobs over their spans, as kwok_decode_nodes does)
int kwok_decode_nodes_gpu(kwok_engine* e, const kwok_codec* c, char* arena, size_t arena_len, const uint64_t* doc_off,
                          const uint32_t* doc_len, size_t n, kwok_node_event* ev, int32_t* status, size_t* n_host) {
    if (!e || !c || (n && (!doc_off || !doc_len || !ev || !status)) || (arena_len && !arena) || n > 0x7FFFFFF0ull ||
        arena_len > 0xFFFFFFF0ull)
        return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    drain(e);
    if (e->poisoned) return poisoned(e);
    if (n_host) *n_host = 0;
    if (!n) return 0;
    std::vector<int32_t> dstat;
    uint32_t nh = 0;
    int rc = json_nodes_decode(e, c, arena, arena_len, doc_off, doc_len, nullptr, n, dstat, &nh);
    if (rc) return rc;
    HIPCHK(e, hipMemcpyAsync(ev, e->ing.d_nev, n * sizeof(kwok_node_event), hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    std::vector<uint32_t> list;
    if ((rc = json_nodes_listed(e, nh, list))) return rc;
    for (uint32_t i : list) {
        kwok_node_event x{};
        dstat[i] = kwok_decode_node(c, arena, arena_len, doc_off[i], doc_len[i], &x);
        ev[i] = x;
    }
    // the documents the device canonicalised (kwok_canon.h): each blob over the start of its own span in the
    // caller's arena, the record's length the canonical one - what kwok_decode_node writes
    for (const CanonDoc& d : e->canon.doc_h) {
        if (d.host || d.doc >= n) continue;
        kwok_str* s[3] = {&ev[d.doc].addresses, &ev[d.doc].allocatable, &ev[d.doc].capacity};
        for (int j = 0; j < 3; j++) {
            if (!d.len[j] || (uint64_t)s[j]->off + s[j]->len > arena_len || d.len[j] > s[j]->len) continue;
            memcpy(arena + s[j]->off, e->canon.bytes_h.data() + d.off[j], d.len[j]);
            s[j]->len = d.len[j];
        }
    }
    int bad = 0;
    for (size_t i = 0; i < n; i++) {
        status[i] = dstat[i];
        if (dstat[i] != KWOK_OK) ev[i] = kwok_node_event{};
        else ev[i].op = KWOK_OP_UPSERT;
        bad += dstat[i] != KWOK_OK;
    }
    if (n_host) *n_host = nh;
    return bad;
}

int kwok_decode_pods_gpu(kwok_engine* e, const kwok_codec* c, const char* arena, size_t arena_len,
                         const uint64_t* doc_off, const uint32_t* doc_len, size_t n, kwok_pod_event* ev,
                         kwok_str* name_ns, uint64_t* spec_key, int32_t* status, size_t* n_host) {
    if (!e || !c || (n && (!doc_off || !doc_len || !ev || !status)) || (arena_len && !arena) || n > 0x7FFFFFF0ull ||
        arena_len > KWOK_JSON_ARENA_MAX)
        return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    drain(e);
    if (e->poisoned) return poisoned(e);
    if (n_host) *n_host = 0;
    if (!n) return 0;
    uint32_t nh = 0;
    int rc = json_decode(e, c, arena, arena_len, doc_off, doc_len, n, nullptr, nullptr, &nh);
    if (rc) return rc;
    std::vector<JsonPodSide> hs;
    std::vector<uint32_t> hl;
    if ((rc = json_complete(e, c, arena, arena_len, doc_off, doc_len, nh, nullptr, nullptr, &hs, &hl))) return rc;
    std::vector<JsonPodSide> side(n);
    HIPCHK(e, hipMemcpyAsync(ev, e->ing.d_ev, n * sizeof(kwok_pod_event), hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipMemcpyAsync(side.data(), e->json.side, n * sizeof(JsonPodSide), hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    for (size_t q = 0; q < hl.size(); q++) side[hl[q]] = hs[q];  // the host-decided documents
    int bad = 0;
    for (size_t i = 0; i < n; i++) {
        status[i] = side[i].status;
        bad += side[i].status != KWOK_OK;
        if (name_ns) {
            name_ns[2 * i] = kwok_str{side[i].name_off, side[i].name_len};
            name_ns[2 * i + 1] = kwok_str{side[i].ns_off, side[i].ns_len};
        }
        if (spec_key) spec_key[i] = side[i].spec_key;
    }
    if (n_host) *n_host = nh;
    return bad;
}

int kwok_ingest_pods_json(kwok_engine* e, const kwok_codec* c, const char* arena, size_t arena_len,
                          const uint64_t* doc_off, const uint32_t* doc_len, const uint8_t* op, const int32_t* handle,
                          size_t n, int32_t* out_handles, int32_t* out_status, uint32_t* out_released, size_t* n_host) {
    if (!e || !c || (n && (!doc_off || !doc_len || !op || !handle)) || (arena_len && !arena) || n > 0x7FFFFFF0ull ||
        arena_len > KWOK_JSON_ARENA_MAX)
        return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    drain(e);
    if (e->poisoned) return poisoned(e);
    if (n_host) *n_host = 0;
    if (!n) return 0;
    const auto t0 = clk::now();
    uint32_t nh = 0;
    int rc = json_decode(e, c, arena, arena_len, doc_off, doc_len, n, op, handle, &nh);
    if (rc) return rc;
    if ((rc = json_complete(e, c, arena, arena_len, doc_off, doc_len, nh, op, handle, nullptr, nullptr))) return rc;
    if (n_host) *n_host = nh;
    if (e->iprof)
        fprintf(stderr, "[kwok json] %zu pod documents decoded on the GPU (%u by the host): %.2f ms\n", n, nh,
                ms_between(t0, clk::now()));
    // the event switch over the decoded records, which stayed on the device
    return ingest_pods_impl(e, e->ing.d_ev, 0, n, nullptr, arena_len, out_handles, out_status, nullptr, out_released,
                            true);
}

// ---- watch streams (kwok_watch.h): framed on the device, ingested in place -----
namespace {
static int watch_reserve(kwok_engine* e, size_t len) {
    auto& Wt = e->watch;
    if (!Wt.counts) {
        if (int rc = dalloc(e, &Wt.counts, 2)) return rc;
        if (hipHostMalloc((void**)&Wt.counts_h.p, 2 * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess)
            return e->fail(KWOK_ENOMEM, "watch framer staging");
    }
    const size_t need = ((len + 15) & ~(size_t)15) + 16;  // (the readers take whole 16-byte windows)
    if (int rc = Wt.bytes.reserve(e, need)) return rc;
    return Wt.tiles.reserve(e, (len + KWOK_WATCH_TILE_BYTES - 1) / KWOK_WATCH_TILE_BYTES);
}
// a framed entry works on the frames of the last framing call only
static int stream_resident(kwok_engine* e, uint64_t stream_id) {
    if (!stream_id || stream_id != e->watch.id) return e->fail(KWOK_EINVAL, "stream_id is not the resident watch stream");
    return KWOK_OK;
}
// The checks of the by-uid framed entry `who` before it touches anything: the engine in step with the
// device, before and after the queued ticks are finished; the uid directory enabled; the stream resident.
static int framed_enter(kwok_engine* e, const char* who, uint64_t stream_id) {
    if (e->poisoned) return poisoned(e);
    drain(e);
    if (e->poisoned) return poisoned(e);
    if (!e->uid.on) return e->fail(KWOK_EINVAL, "%s: the uid directory is not enabled", who);
    return stream_resident(e, stream_id);
}
// the records of a framed batch from the host's copy of the frames: the object's
// span and the op of the frame type; a record that names no ingestible frame gets
// a span outside the stream, which the decode kernels answer with KWOK_EINVAL
// (k_json_pods / k_json_nodes: "a span outside the arena") and nothing applies
static int framed_records(kwok_engine* e, uint64_t stream_id, const uint32_t* frame_idx, size_t n, std::vector<uint64_t>& off,
                   std::vector<uint32_t>& len, std::vector<uint8_t>& op) {
    auto& Wt = e->watch;
    if (int rc = stream_resident(e, stream_id)) return rc;
    off.resize(n), len.resize(n), op.resize(n);
    for (size_t i = 0; i < n; i++) {
        const kwok_watch_frame* f = frame_idx[i] < Wt.frames_h.size() ? &Wt.frames_h[frame_idx[i]] : nullptr;
        const bool ok = f && f->status == KWOK_OK &&
                        (f->type == KWOK_WATCH_ADDED || f->type == KWOK_WATCH_MODIFIED || f->type == KWOK_WATCH_DELETED);
        off[i] = ok ? f->doc_off : ~0ull;
        len[i] = ok ? f->doc_len : 0u;
        op[i] = ok && f->type == KWOK_WATCH_DELETED ? KWOK_OP_DELETE : KWOK_OP_UPSERT;
    }
    return KWOK_OK;
}
}  // namespace

int kwok_frame_watch_gpu(kwok_engine* e, const char* stream, size_t len, kwok_watch_frame* frames, size_t cap,
                         size_t* n_frames, size_t* consumed, size_t* n_host, uint64_t* stream_id) {
    if (n_frames) *n_frames = 0;
    if (consumed) *consumed = 0;
    if (n_host) *n_host = 0;
    if (stream_id) *stream_id = 0;
    if (!e || !n_frames || !consumed || !stream_id || len > 0xFFFFFFF0ull || (len && !stream) || (cap && !frames))
        return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    auto& Wt = e->watch;
    hipStream_t st = e->st;
    Wt.id = 0;  // (a failed call leaves no stream resident)
    Wt.frames_h.clear();
    int rc = watch_reserve(e, len);
    if (rc) return rc;
    const uint32_t tiles = (uint32_t)((len + KWOK_WATCH_TILE_BYTES - 1) / KWOK_WATCH_TILE_BYTES);
    const size_t padded = ((len + 15) & ~(size_t)15) + 16;
    // KWOK_INGEST_PROF: device-side stamps - upload | count + scan | emit | parse
    const auto t0 = clk::now();
    ProfEvents<5> pe(e->iprof, e->st);
    auto stamp = [&](int k) { pe.stamp(k); };
    stamp(0);
    if (len) HIPCHK(e, hipMemcpyAsync(Wt.stream, stream, len, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemsetAsync(Wt.stream + len, 0, padded - len, st));
    Wt.stats[KWOK_WATCH_STAT_BYTES] += len;
    stamp(1);
    launch_frame_count(Wt.stream, len, tiles, Wt.tile_cnt, st);
    launch_frame_scan(Wt.tile_cnt, tiles, Wt.tile_base, Wt.counts, st);
    HIPCHK(e, hipGetLastError());
    stamp(2);
    HIPCHK(e, hipMemcpyAsync(Wt.counts_h, Wt.counts, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    const uint32_t n = Wt.counts_h[0];
    *n_frames = n;
    if (n > cap) return e->fail(KWOK_EINVAL, "kwok_frame_watch_gpu: cap smaller than the line count (%u)", n);
    if (!n) {  // (no newline: nothing consumed, no frame - but the call succeeded: an empty stream is resident)
        Wt.len = len, Wt.host = stream;
        *stream_id = Wt.id = Wt.next_id++;
        return 0;
    }
    if ((rc = Wt.lines.reserve(e, n))) return rc;
    const bool prof = pe.on();
    stamp(0);  // (re-used: the emit's start, after the host's wait for the count)
    launch_frame_emit(Wt.stream, len, tiles, Wt.tile_base, Wt.ends, n, st);
    stamp(3);
    HIPCHK(e, hipMemsetAsync(Wt.counts + 1, 0, 4, st));
    launch_frame_parse(Wt.stream, Wt.ends, n, Wt.frames, Wt.host_list, Wt.counts + 1, st);
    HIPCHK(e, hipGetLastError());
    stamp(4);
    Wt.frames_h.resize(n);
    HIPCHK(e, hipMemcpyAsync(Wt.frames_h.data(), Wt.frames, (size_t)n * sizeof(kwok_watch_frame), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(Wt.counts_h + 1, Wt.counts + 1, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(Wt.counts_h, Wt.ends + (n - 1), 4, hipMemcpyDeviceToHost, st));  // the last newline
    HIPCHK(e, hipStreamSynchronize(st));
    const uint32_t nh = Wt.counts_h[1];
    *consumed = (size_t)Wt.counts_h[0] + 1;
    if (nh) {  // the lines the device listed: the host framer over the caller's bytes
        std::vector<uint32_t> list(nh);
        HIPCHK(e, hipMemcpyAsync(list.data(), Wt.host_list, (size_t)nh * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipStreamSynchronize(st));
        for (uint32_t i : list) {
            if (i >= n) return e->fail(KWOK_EDEVICE, "watch framer: listed line %u of %u", i, n);
            const uint32_t lo = Wt.frames_h[i].line_off;
            const char* nl = (const char*)memchr(stream + lo, '\n', len - lo);
            if (!nl) return e->fail(KWOK_EDEVICE, "watch framer: listed line %u has no end", i);
            frame_line(stream, lo, (uint32_t)(nl - stream), &Wt.frames_h[i]);
            HIPCHK(e, hipMemcpyAsync(Wt.frames + i, &Wt.frames_h[i], sizeof(kwok_watch_frame), hipMemcpyHostToDevice, st));
        }
        HIPCHK(e, hipStreamSynchronize(st));
    }
    int bad = 0;
    for (uint32_t i = 0; i < n; i++) bad += Wt.frames_h[i].status != KWOK_OK;
    memcpy(frames, Wt.frames_h.data(), (size_t)n * sizeof(kwok_watch_frame));
    if (n_host) *n_host = nh;
    Wt.len = len, Wt.host = stream;
    Wt.stats[KWOK_WATCH_STAT_FRAMES] += n;
    Wt.stats[KWOK_WATCH_STAT_HOST_FRAMES] += nh;
    *stream_id = Wt.id = Wt.next_id++;
    if (prof) {
        const float cs = pe.elapsed(1, 2), em = pe.elapsed(0, 3), pa = pe.elapsed(3, 4);
        fprintf(stderr, "[kwok watch] %zu bytes, %u frames (%u by the host): k_frame_count + k_frame_scan %.3f ms, "
                        "k_frame_emit %.3f ms, k_frame_parse %.3f ms; the call %.2f ms\n", len, n, nh, cs, em, pa,
                ms_between(t0, clk::now()));
    }
    return bad;
}

int kwok_ingest_pods_framed(kwok_engine* e, const kwok_codec* c, uint64_t stream_id, const uint32_t* frame_idx,
                            const int32_t* handle, size_t n, int32_t* out_handles, int32_t* out_status,
                            uint32_t* out_released, size_t* n_host) {
    if (!e || !c || (n && (!frame_idx || !handle)) || n > 0x7FFFFFF0ull) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    drain(e);
    if (e->poisoned) return poisoned(e);
    if (n_host) *n_host = 0;
    auto& Wt = e->watch;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    std::vector<uint8_t> op;
    int rc = framed_records(e, stream_id, frame_idx, n, off, len, op);
    if (rc) return rc;
    Wt.stats[KWOK_WATCH_STAT_INGESTS]++;
    if (!n) return 0;
    uint32_t nh = 0;
    if ((rc = json_decode(e, c, Wt.host, Wt.len, off.data(), len.data(), n, op.data(), handle, &nh, Wt.stream))) return rc;
    if ((rc = json_complete(e, c, Wt.host, Wt.len, off.data(), len.data(), nh, op.data(), handle, nullptr, nullptr)))
        return rc;
    if (n_host) *n_host = nh;
    ScopedPtr<uint8_t> src(e->ing.arena_src, Wt.stream);  // the ingest kernels read the batch's strings from the resident stream
    return ingest_pods_impl(e, e->ing.d_ev, 0, n, nullptr, Wt.len, out_handles, out_status, nullptr, out_released, true);
}

int kwok_ingest_nodes_framed(kwok_engine* e, const kwok_codec* c, uint64_t stream_id, const uint32_t* frame_idx,
                             size_t n, int32_t* out_handles, int32_t* out_status, size_t* n_host) {
    if (!e || !c || (n && !frame_idx) || n > 0x7FFFFFF0ull) return KWOK_EINVAL;
    if (n_host) *n_host = 0;
    auto& Wt = e->watch;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    std::vector<uint8_t> op;
    int rc = framed_records(e, stream_id, frame_idx, n, off, len, op);
    if (rc) return rc;
    Wt.stats[KWOK_WATCH_STAT_INGESTS]++;
    // the node uid directory: the records' uid spans in the resident stream, for the note behind the apply pass
    auto& D = e->ndir;
    NodeUidNote un{};
    if (D.on && n) {  // (read from the resident frames by the uploaded indices: k_nd_frame_recs, not strict)
        if (e->poisoned) return poisoned(e);
        if ((rc = D.recs.reserve(e, n))) return rc;
        HIPCHK(e, hipMemcpyAsync(D.fidx, frame_idx, n * 4, hipMemcpyHostToDevice, e->st));
        launch_nd_frame_recs(Wt.frames, (uint32_t)Wt.frames_h.size(), Wt.len, D.fidx, (uint32_t)n, false, nullptr, nullptr, nullptr,
                             D.uoff, D.ulen, nullptr, e->st);
        HIPCHK(e, hipGetLastError());
        un = NodeUidNote{Wt.stream, Wt.len, D.uoff, D.ulen};
    }
    ScopedPtr<NodeUidNote> uids(D.note, D.on && n ? &un : nullptr);
    ScopedPtr<uint8_t> src(e->ing.arena_src, Wt.stream);  // the ingest kernels read the batch's strings from the resident stream
    return ingest_nodes_json_impl(e, c, Wt.host, Wt.len, off.data(), len.data(), op.data(), n, out_handles, out_status,
                                  n_host, Wt.stream);
}

int kwok_watch_stats(kwok_engine* e, uint64_t out[KWOK_WATCH_STAT_COUNT]) {
    if (!e || !out) return KWOK_EINVAL;
    for (int k = 0; k < KWOK_WATCH_STAT_COUNT; k++) out[k] = e->watch.stats[k];
    return KWOK_OK;
}

// ---- patch responses (kwok_watch.h): the caller's spans, one thread per document; the
// buffer and its frames become the resident stream, as a watch stream does ----
int kwok_frame_responses_gpu(kwok_engine* e, const char* buf, size_t len, const uint64_t* off, const uint32_t* dlen,
                             size_t n, kwok_watch_frame* frames, size_t* n_host, uint64_t* stream_id) {
    if (n_host) *n_host = 0;
    if (stream_id) *stream_id = 0;
    if (!e || !stream_id || len > 0xFFFFFFF0ull || (len && !buf) || (n && (!off || !dlen || !frames)) || n > 0x7FFFFFF0ull)
        return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    auto& Wt = e->watch;
    hipStream_t st = e->st;
    Wt.id = 0;  // (a failed call leaves no stream resident)
    Wt.frames_h.clear();
    int rc = watch_reserve(e, len);
    if (rc) return rc;
    const size_t padded = ((len + 15) & ~(size_t)15) + 16;
    const auto t0 = clk::now();
    ProfEvents<2> pe(e->iprof, e->st);
    if (len) HIPCHK(e, hipMemcpyAsync(Wt.stream, buf, len, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemsetAsync(Wt.stream + len, 0, padded - len, st));
    Wt.rstats[KWOK_RESP_STAT_BYTES] += len;
    uint32_t nh = 0;
    int bad = 0;
    if (n) {
        if ((rc = Wt.lines.reserve(e, n)) || (rc = Wt.rspans.reserve(e, n))) return rc;
        HIPCHK(e, hipMemcpyAsync(Wt.r_off, off, n * 8, hipMemcpyHostToDevice, st));
        HIPCHK(e, hipMemcpyAsync(Wt.r_len, dlen, n * 4, hipMemcpyHostToDevice, st));
        HIPCHK(e, hipMemsetAsync(Wt.counts + 1, 0, 4, st));
        pe.stamp(0);
        launch_resp_parse(Wt.stream, len, Wt.r_off, Wt.r_len, (uint32_t)n, Wt.frames, Wt.host_list, Wt.counts + 1, st);
        HIPCHK(e, hipGetLastError());
        pe.stamp(1);
        Wt.frames_h.resize(n);
        HIPCHK(e, hipMemcpyAsync(Wt.frames_h.data(), Wt.frames, n * sizeof(kwok_watch_frame), hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipMemcpyAsync(Wt.counts_h + 1, Wt.counts + 1, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipStreamSynchronize(st));
        nh = Wt.counts_h[1];
        if (nh > n) {
            Wt.frames_h.clear();
            return e->fail(KWOK_EDEVICE, "response framer: %u of %zu documents listed", nh, n);
        }
        if (nh) {  // the documents the device listed: the host framer over the caller's bytes
            std::vector<uint32_t> list(nh);
            HIPCHK(e, hipMemcpyAsync(list.data(), Wt.host_list, (size_t)nh * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(e, hipStreamSynchronize(st));
            for (uint32_t i : list) {
                if (i >= n || off[i] > len || dlen[i] > len - off[i]) {
                    Wt.frames_h.clear();
                    return e->fail(KWOK_EDEVICE, "response framer: listed document %u of %zu", i, n);
                }
                frame_response(buf, (uint32_t)off[i], (uint32_t)(off[i] + dlen[i]), &Wt.frames_h[i]);
                HIPCHK(e, hipMemcpyAsync(Wt.frames + i, &Wt.frames_h[i], sizeof(kwok_watch_frame), hipMemcpyHostToDevice, st));
            }
            HIPCHK(e, hipStreamSynchronize(st));
        }
        for (size_t i = 0; i < n; i++) bad += Wt.frames_h[i].status != KWOK_OK;
        memcpy(frames, Wt.frames_h.data(), n * sizeof(kwok_watch_frame));
    } else {
        HIPCHK(e, hipStreamSynchronize(st));
    }
    if (n_host) *n_host = nh;
    Wt.len = len, Wt.host = buf;
    Wt.rstats[KWOK_RESP_STAT_FRAMES] += n;
    Wt.rstats[KWOK_RESP_STAT_HOST_FRAMES] += nh;
    *stream_id = Wt.id = Wt.next_id++;
    if (pe.on())
        fprintf(stderr, "[kwok responses] %zu bytes, %zu documents (%u by the host): k_resp_parse %.3f ms; the call %.2f ms\n",
                len, n, nh, n ? pe.elapsed(0, 1) : 0.f, ms_between(t0, clk::now()));
    return bad;
}

int kwok_response_stats(kwok_engine* e, uint64_t out[KWOK_RESP_STAT_COUNT]) {
    if (!e || !out) return KWOK_EINVAL;
    for (int k = 0; k < KWOK_RESP_STAT_COUNT; k++) out[k] = e->watch.rstats[k];
    return KWOK_OK;
}

// ---- node status blobs canonicalised on the device (kwok_canon.h): the switch and its counters;
// the work is json_nodes_canon's, behind every device node decode ----
int kwok_canon_enable(kwok_engine* e, int on) {
    if (!e) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    e->canon.on = on != 0;  // (the buffers come with the first decode that needs them)
    return KWOK_OK;
}

int kwok_canon_stats(const kwok_engine* e, uint64_t out[KWOK_CANON_STAT_COUNT]) {
    if (!e || !out) return KWOK_EINVAL;
    for (int k = 0; k < KWOK_CANON_STAT_COUNT; k++) out[k] = e->canon.stats[k];
    return KWOK_OK;
}

// ---- List bodies (kwok_watch.h): split by bracket depth on the device, the items
// parsed there, the envelope by the host from the caller's bytes ----
namespace {
static int list_reserve(kwok_engine* e, size_t tiles) {
    auto& Wt = e->watch;
    if (!Wt.lc) {
        if (int rc = dalloc(e, &Wt.lc, (size_t)KWOK_LIST_COUNTERS)) return rc;
        if (hipHostMalloc((void**)&Wt.lc_h.p, KWOK_LIST_COUNTERS * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess)
            return e->fail(KWOK_ENOMEM, "list framer staging");
    }
    return Wt.ltiles.reserve(e, tiles);
}
}  // namespace

int kwok_frame_list_gpu(kwok_engine* e, const char* body, size_t len, kwok_watch_frame* frames, size_t cap,
                        size_t* n_frames, kwok_list_info* info, size_t* n_host, uint64_t* stream_id) {
    if (n_frames) *n_frames = 0;
    if (info) memset(info, 0, sizeof *info);
    if (n_host) *n_host = 0;
    if (stream_id) *stream_id = 0;
    if (!e || !n_frames || !info || !stream_id || len > 0xFFFFFFF0ull || (len && !body) || (cap && !frames))
        return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    auto& Wt = e->watch;
    hipStream_t st = e->st;
    Wt.id = 0;  // (a failed call leaves no stream resident)
    Wt.frames_h.clear();
    Wt.lstats[KWOK_LIST_STAT_BODIES]++;
    if (!len) return e->fail(KWOK_EINVAL, "kwok_frame_list_gpu: an empty body");
    const uint32_t tiles = (uint32_t)((len + KWOK_WATCH_TILE_BYTES - 1) / KWOK_WATCH_TILE_BYTES);
    int rc = 0;
    if ((rc = watch_reserve(e, len)) || (rc = list_reserve(e, tiles))) return rc;
    const size_t padded = ((len + 15) & ~(size_t)15) + 16;
    const size_t L = Wt.ltiles.cap;
    uint32_t *tq = Wt.ltile, *td0 = tq + L, *td1 = td0 + L, *qb = td1 + L, *db = qb + L, *ts = db + L, *te = ts + L;
    uint32_t *lc = Wt.lc, *lh = Wt.lc_h;
    // KWOK_INGEST_PROF: device-side stamps - upload | quotes + scans | count + scans | emit + range | parse
    const auto t0 = clk::now();
    ProfEvents<7> pe(e->iprof, e->st);
    auto stamp = [&](int k) { pe.stamp(k); };
    const bool prof = pe.on();
    float ms[4] = {0, 0, 0, 0};  // quotes, count, emit, parse
    uint32_t n = 0, nh = 0;
    auto report = [&](const char* how) {
        if (!prof) return;
        fprintf(stderr, "[kwok list] %zu bytes, %u items (%u by the host), %s: k_list_quotes + scans %.3f ms, "
                        "k_list_split<count> + scans %.3f ms, k_list_split<emit> + k_list_range %.3f ms, k_list_parse %.3f ms; "
                        "the call %.2f ms\n", len, n, nh, how, ms[0], ms[1], ms[2], ms[3], ms_between(t0, clk::now()));
    };
    stamp(0);
    HIPCHK(e, hipMemcpyAsync(Wt.stream, body, len, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemsetAsync(Wt.stream + len, 0, padded - len, st));
    Wt.lstats[KWOK_LIST_STAT_BYTES] += len;
    HIPCHK(e, hipMemsetAsync(lc, 0, KWOK_LIST_COUNTERS * sizeof(uint32_t), st));
    HIPCHK(e, hipMemsetAsync(lc + LC_OPEN_POS, 0xFF, sizeof(uint32_t), st));
    stamp(1);
    launch_list_quotes(Wt.stream, len, tiles, tq, td0, td1, st);
    launch_frame_scan(tq, tiles, qb, lc + LC_QUOTES, st);
    launch_list_pick(qb, td0, td1, tiles, st);
    launch_frame_scan(td0, tiles, db, lc + LC_DEPTH, st);
    stamp(2);
    launch_list_count(Wt.stream, len, tiles, qb, db, ts, te, lc, st);
    launch_frame_scan(ts, tiles, ts, lc + LC_STARTS, st);
    launch_frame_scan(te, tiles, te, lc + LC_ENDS, st);
    HIPCHK(e, hipGetLastError());
    stamp(3);
    HIPCHK(e, hipMemcpyAsync(lh, lc, KWOK_LIST_COUNTERS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    ms[0] = pe.elapsed(1, 2), ms[1] = pe.elapsed(2, 3);
    // a valid body ends outside every string and every bracket, and an array that its
    // root holds is closed once
    if ((lh[LC_QUOTES] & 1u) || lh[LC_DEPTH] != 0 || lh[LC_STARTS] != lh[LC_ENDS] || lh[LC_OPEN_N] != lh[LC_CLOSE_N] ||
        (lh[LC_OPEN_N] == 1 && lh[LC_OPEN_POS] >= lh[LC_CLOSE_POS])) {
        report("unbalanced");
        return e->fail(KWOK_EINVAL, "kwok_frame_list_gpu: the body is not a JSON object");
    }
    const uint32_t open = lh[LC_OPEN_POS], close = lh[LC_CLOSE_POS], S = lh[LC_STARTS];
    int env = 1;
    if (lh[LC_OPEN_N] == 1) {
        // the device's part goes on while the host reads the envelope
        if ((rc = Wt.lines.reserve(e, S)) || (rc = Wt.cands.reserve(e, S))) return rc;
        stamp(6);  // (the emit's start, after the host's wait for the counts)
        launch_list_emit(Wt.stream, len, tiles, qb, db, ts, te, Wt.starts, Wt.ends, S, st);
        launch_list_range(Wt.starts, S, open, close, lc, st);
        HIPCHK(e, hipGetLastError());
        stamp(4);
        HIPCHK(e, hipMemcpyAsync(lh + LC_R0, lc + LC_R0, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        env = list_envelope(body, len, open, close, info);
        HIPCHK(e, hipStreamSynchronize(st));
        ms[2] = pe.elapsed(6, 4);
        if (env < 0) {
            report("a bad envelope");
            return e->fail(KWOK_EINVAL, "kwok_frame_list_gpu: the body is not a JSON object");
        }
    }
    if (env == 1) {  // no single root array that is the first `items`: the host framer decides the whole body
        Wt.lstats[KWOK_LIST_STAT_HOST_BODIES]++;
        size_t nf = 0;
        std::vector<kwok_watch_frame> tmp(cap);
        rc = kwok_frame_list(body, len, tmp.data(), cap, &nf, info);
        *n_frames = nf;
        n = rc ? 0u : (uint32_t)nf;
        report("the body framed by the host");
        if (rc) return e->fail(KWOK_EINVAL, "kwok_frame_list_gpu: %s", kwok_codec_last_error());
        if ((rc = Wt.lines.reserve(e, nf))) return rc;
        Wt.frames_h.assign(tmp.begin(), tmp.begin() + nf);
        if (nf) {
            HIPCHK(e, hipMemcpyAsync(Wt.frames, Wt.frames_h.data(), nf * sizeof(kwok_watch_frame), hipMemcpyHostToDevice, st));
            HIPCHK(e, hipStreamSynchronize(st));
            memcpy(frames, Wt.frames_h.data(), nf * sizeof(kwok_watch_frame));
        }
        Wt.lstats[KWOK_LIST_STAT_ITEMS] += nf;
        Wt.len = len, Wt.host = body;
        *stream_id = Wt.id = Wt.next_id++;
        return KWOK_OK;
    }
    auto invalid = [&](const char* how) {
        memset(info, 0, sizeof *info);
        n = 0;
        report(how);
        return e->fail(KWOK_EINVAL, "kwok_frame_list_gpu: items is not an array of objects (%s)", how);
    };
    const uint32_t r0 = lh[LC_R0], r1 = lh[LC_R1];
    if (r0 > r1 || r1 > S) return e->fail(KWOK_EDEVICE, "list framer: items %u..%u of %u candidates", r0, r1, S);
    n = r1 - r0;
    if (!n) {  // [ ]: only whitespace between the brackets
        for (uint32_t p = open + 1; p < close; p++)
            if (body[p] != ' ' && body[p] != '\t' && body[p] != '\n' && body[p] != '\r') return invalid("a stray byte");
    }
    // (the device's frames are sized by the candidates, not by cap: the body is judged first, as the host does)
    launch_list_parse(Wt.stream, Wt.starts, Wt.ends, r0, n, open, close, Wt.frames, Wt.host_list, lc, st);
    HIPCHK(e, hipGetLastError());
    stamp(5);
    Wt.frames_h.resize(n);
    if (n) HIPCHK(e, hipMemcpyAsync(Wt.frames_h.data(), Wt.frames, (size_t)n * sizeof(kwok_watch_frame), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(lh + LC_BAD, lc + LC_BAD, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    if (n) ms[3] = pe.elapsed(4, 5);
    if (lh[LC_BAD]) {
        Wt.frames_h.clear();
        return invalid("an item or the text between items");
    }
    if (n > cap) {
        memset(info, 0, sizeof *info);
        Wt.frames_h.clear();
        *n_frames = n;
        return e->fail(KWOK_EINVAL, "kwok_frame_list_gpu: cap smaller than the item count (%u)", n);
    }
    nh = lh[LC_HOST];
    if (nh) {  // the items the device listed: the host framer over the caller's bytes
        std::vector<uint32_t> list(nh);
        HIPCHK(e, hipMemcpyAsync(list.data(), Wt.host_list, (size_t)nh * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipStreamSynchronize(st));
        for (uint32_t i : list) {
            if (i >= n) return e->fail(KWOK_EDEVICE, "list framer: listed item %u of %u", i, n);
            const uint32_t lo = Wt.frames_h[i].doc_off, hi = lo + Wt.frames_h[i].doc_len;
            if (hi > len || !frame_item(body, lo, hi, &Wt.frames_h[i]))
                return e->fail(KWOK_EDEVICE, "list framer: listed item %u does not parse on the host", i);
            HIPCHK(e, hipMemcpyAsync(Wt.frames + i, &Wt.frames_h[i], sizeof(kwok_watch_frame), hipMemcpyHostToDevice, st));
        }
        HIPCHK(e, hipStreamSynchronize(st));
    }
    if (n) memcpy(frames, Wt.frames_h.data(), (size_t)n * sizeof(kwok_watch_frame));
    *n_frames = n;
    if (n_host) *n_host = nh;
    Wt.len = len, Wt.host = body;
    Wt.lstats[KWOK_LIST_STAT_ITEMS] += n;
    Wt.lstats[KWOK_LIST_STAT_HOST_ITEMS] += nh;
    *stream_id = Wt.id = Wt.next_id++;
    report("split on the device");
    return KWOK_OK;
}

int kwok_list_stats(kwok_engine* e, uint64_t out[KWOK_LIST_STAT_COUNT]) {
    if (!e || !out) return KWOK_EINVAL;
    for (int k = 0; k < KWOK_LIST_STAT_COUNT; k++) out[k] = e->watch.lstats[k];
    return KWOK_OK;
}

// ---- relist with Replace (kwok_watch.h) ---------------------------
namespace {
bool resync_kind_ok(int kind) { return kind == KWOK_KIND_NODES || kind == KWOK_KIND_PODS; }
int resync_read_counters(kwok_engine* e) {
    auto& R = e->resync;
    HIPCHK(e, hipMemcpyAsync(R.ctr_h, R.ctr, sizeof(ResyncCounters), hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    return KWOK_OK;
}
}  // namespace

int kwok_resync_begin(kwok_engine* e, int kind) {
    if (!e || !resync_kind_ok(kind)) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    auto& R = e->resync;
    if (!R.ctr) {
        if (int rc = dalloc(e, &R.ctr, 1)) return rc;
        if (int rc = dalloc(e, &R.total, 1)) return rc;
        if (hipHostMalloc((void**)&R.ctr_h.p, sizeof(ResyncCounters), hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc((void**)&R.total_h.p, sizeof(uint32_t), hipHostMallocDefault) != hipSuccess)
            return e->fail(KWOK_ENOMEM, "resync staging");
        memset(R.ctr_h, 0, sizeof(ResyncCounters));
    }
    DevArr<uint8_t>& seen = kind == KWOK_KIND_PODS ? R.pod_seen : R.node_seen;
    const size_t bytes = kind == KWOK_KIND_PODS ? e->PLa : e->NLa;
    if (!seen) {  // (zeroed by the allocation)
        if (int rc = dalloc(e, &seen, bytes)) return rc;
    } else {
        HIPCHK(e, hipMemsetAsync(seen, 0, bytes, e->st));
    }
    R.open[kind] = true;
    R.stats[KWOK_RESYNC_STAT_SESSIONS]++;
    return KWOK_OK;
}

int kwok_resync_end(kwok_engine* e, int kind) {
    if (!e || !resync_kind_ok(kind)) return KWOK_EINVAL;
    e->resync.open[kind] = false;  // (the marks are cleared by the next begin)
    return KWOK_OK;
}

int kwok_resync_mark(kwok_engine* e, int kind, const int32_t* handles, size_t n, size_t* n_bad) {
    if (n_bad) *n_bad = 0;
    if (!e || !resync_kind_ok(kind) || (n && !handles) || n > 0x7FFFFFF0ull) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    auto& R = e->resync;
    if (!R.open[kind]) return e->fail(KWOK_EINVAL, "kwok_resync_mark: no session open");
    drain(e);  // (a handle is judged against the state after every submitted tick)
    if (e->poisoned) return poisoned(e);
    if (!n) return KWOK_OK;
    if (int rc = R.marks.reserve(e, n)) return rc;
    hipStream_t st = e->st;
    HIPCHK(e, hipMemcpyAsync(R.d_mark, handles, n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemsetAsync(&R.ctr->bad, 0, sizeof(R.ctr->bad), st));
    launch_seen_mark_handles(e->S, kind == KWOK_KIND_PODS, R.d_mark, (uint32_t)n, kind == KWOK_KIND_PODS ? R.pod_seen : R.node_seen,
                             R.ctr, st);
    HIPCHK(e, hipGetLastError());
    if (int rc = resync_read_counters(e)) return rc;
    if (n_bad) *n_bad = (size_t)R.ctr_h->bad;
    return KWOK_OK;
}

int kwok_resync_sweep(kwok_engine* e, int kind, int32_t* out_handles, size_t cap, size_t* n_swept, uint32_t* out_released,
                      int32_t* out_node) {
    if (n_swept) *n_swept = 0;
    if (!e || !resync_kind_ok(kind) || (cap && !out_handles)) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    if (e->multi) return e->fail(KWOK_EINVAL, "kwok_resync_sweep: single-rank engines only");
    auto& R = e->resync;
    if (!R.open[kind]) return e->fail(KWOK_EINVAL, "kwok_resync_sweep: no session open");
    drain(e);  // the device state reflects every submitted tick
    if (e->poisoned) return poisoned(e);
    const bool pods = kind == KWOK_KIND_PODS;
    const uint8_t* seen = pods ? R.pod_seen : R.node_seen;
    hipStream_t st = e->st;
    const auto t0 = clk::now();
    // KWOK_INGEST_PROF: device-side stamps around count + scan and around emit
    ProfEvents<4> pev(e->iprof, e->st);
    auto stamp = [&](int k) { pev.stamp(k); };
    // pass 1: the unmarked live objects per tile, their exclusive prefixes and the total
    const uint32_t tiles = sweep_tiles(e->S, pods);
    if (int rc = R.tiles.reserve(e, tiles)) return rc;
    stamp(0);
    launch_sweep_count(e->S, pods, seen, R.tile_cnt, st);
    launch_frame_scan(R.tile_cnt, tiles, R.tile_base, R.total, st);
    HIPCHK(e, hipGetLastError());
    stamp(1);
    HIPCHK(e, hipMemcpyAsync(R.total_h, R.total, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    const uint32_t n = *R.total_h;
    if (n_swept) *n_swept = n;
    if (n > cap) return e->fail(KWOK_EINVAL, "kwok_resync_sweep: %u objects to sweep, out_handles holds %zu", n, cap);
    R.open[kind] = false;  // the sweep closes the session (its DELETE records mark nothing)
    if (!n) {
        if (e->iprof) {
            const float cs = pev.elapsed(0, 1);
            fprintf(stderr, "[kwok resync] %s: %u tiles, 0 swept: k_sweep_count + k_frame_scan %.3f ms; the call %.3f ms\n",
                    pods ? "pods" : "nodes", tiles, cs, ms_between(t0, clk::now()));
        }
        return KWOK_OK;
    }
    if (int rc = R.swept.reserve(e, n)) return rc;
    // pass 2: the DELETE records into the ingest's own record buffer, in slot order; then the ingest's chain
    // over them, resident (no record or name crosses the link)
    int rc = pods ? ingest_reserve(e, n, 0) : node_reserve(e, n, 0);
    if (rc) return rc;
    stamp(2);
    launch_sweep_emit(e->S, pods, seen, R.tile_base, n, pods ? e->ing.d_ev : (void*)e->ing.d_nev, R.d_handles, R.d_nodes, st);
    HIPCHK(e, hipGetLastError());
    stamp(3);
    const auto t2 = clk::now();
    uint64_t released = 0;
    if (pods) {
        std::vector<uint32_t> rel_tmp(out_released ? 0 : n);
        uint32_t* rel = out_released ? out_released : rel_tmp.data();
        rc = ingest_pods_impl(e, e->ing.d_ev, 1, n, nullptr, 0, nullptr, nullptr, nullptr, rel, true);
        if (rc >= 0)
            for (uint32_t i = 0; i < n; i++) released += rel[i] != 0;
    } else {
        e->emit_hint = true;
        e->quiet = 0;
        e->state_changed();
        const std::unordered_map<uint32_t, uint32_t> hdoc;
        const std::vector<kwok_node_event> hrec;
        const std::vector<std::string> hbuf;
        const NodeJsonCtx ctx{nullptr, &hdoc, &hrec, &hbuf};
        ScopedPtr<uint8_t> names(e->ing.arena_src, e->S.node_name);  // the records' name spans index the directory's own names
        rc = ingest_nodes_impl(e, nullptr, n, nullptr, (size_t)e->NL * NAME_STRIDE, nullptr, nullptr, &ctx);
    }
    if (rc < 0) return rc;
    if (rc > 0) {  // (every record names a live object: none can be rejected)
        e->poisoned = true;
        return e->fail(KWOK_EDEVICE, "kwok_resync_sweep: %d of %u DELETE records rejected", rc, n);
    }
    HIPCHK(e, hipMemcpyAsync(out_handles, R.d_handles, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (pods && out_node) HIPCHK(e, hipMemcpyAsync(out_node, R.d_nodes, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    R.stats[pods ? KWOK_RESYNC_STAT_SWEPT_PODS : KWOK_RESYNC_STAT_SWEPT_NODES] += n;
    R.stats[KWOK_RESYNC_STAT_RELEASED] += released;
    if (e->iprof) {
        const float cs = pev.elapsed(0, 1), em = pev.elapsed(2, 3);
        fprintf(stderr, "[kwok resync] %s: %u tiles, %u swept (%llu addresses put back): k_sweep_count + k_frame_scan %.3f ms, "
                        "k_sweep_emit %.3f ms, apply chain + results %.3f ms; the call %.3f ms\n", pods ? "pods" : "nodes", tiles,
                n, (unsigned long long)released, cs, em, ms_between(t2, clk::now()), ms_between(t0, clk::now()));
    }
    return KWOK_OK;
}

int kwok_resync_stats(kwok_engine* e, uint64_t out[KWOK_RESYNC_STAT_COUNT]) {
    if (!e || !out) return KWOK_EINVAL;
    auto& R = e->resync;
    if (R.ctr && !e->poisoned)
        if (int rc = resync_read_counters(e)) return rc;
    for (int k = 0; k < KWOK_RESYNC_STAT_COUNT; k++) out[k] = R.stats[k];
    out[KWOK_RESYNC_STAT_MARKED] = R.ctr_h ? (uint64_t)R.ctr_h->marked : 0;
    return KWOK_OK;
}

// ---- the pod uid directory (kwok_watch.h, uid.hip) ---------------------------------
namespace {
int uid_read_counters(kwok_engine* e) {
    auto& U = e->uid;
    HIPCHK(e, hipMemcpyAsync(U.ctr_h, U.ctr, sizeof(UidCounters), hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    if (U.ctr_h->err) {
        e->poisoned = true;
        return e->fail(KWOK_EDEVICE, "uid directory: a probe wrapped the whole table");
    }
    return KWOK_OK;
}
// the table cleared and every live slot with a uid inserted again (k_uid_rebuild)
int uid_rebuild(kwok_engine* e) {
    auto& U = e->uid;
    hipStream_t st = e->st;
    HIPCHK(e, hipMemsetAsync(U.tab, 0, U.tab_cap * 8, st));
    HIPCHK(e, hipMemsetAsync(&U.ctr->entries, 0, sizeof(U.ctr->entries), st));
    launch_uid_rebuild(e->S, U.dir(), st);
    HIPCHK(e, hipGetLastError());
    if (int rc = uid_read_counters(e)) return rc;
    U.live = U.ctr_h->entries;
    U.inserted = 0;
    U.stats[KWOK_UID_STAT_REBUILDS]++;
    return KWOK_OK;
}
// before a launch that may insert `incoming` entries: the table sized for the pod slots (a growth
// outgrew it), stale entries dropped once live + inserted exceeds half of it
int uid_ensure(kwok_engine* e, size_t incoming) {
    auto& U = e->uid;
    auto want_cap = [&](uint64_t entries) {
        if (U.forced_log2) return (size_t)1 << U.forced_log2;
        size_t c = std::max<size_t>(U.tab_cap, 64);
        while (c < 2 * (uint64_t)e->PL || c < 2 * entries) c <<= 1;
        return c;
    };
    auto resize = [&](size_t cap) -> int {
        dfree(U.tab);
        U.tab_cap = 0;
        if (int rc = dalloc(e, &U.tab, cap)) return rc;
        U.tab_cap = cap;
        return uid_rebuild(e);
    };
    int rc = 0;
    if (want_cap(0) != U.tab_cap) {
        if ((rc = resize(want_cap(0)))) return rc;
    } else if (U.live + U.inserted + incoming > U.tab_cap / 2 && U.inserted) {
        if ((rc = uid_rebuild(e))) return rc;
    }
    if (U.live + incoming > U.tab_cap / 2) {
        if (!U.forced_log2) {
            if ((rc = resize(want_cap(U.live + incoming)))) return rc;
        } else if (U.live + incoming >= U.tab_cap) {  // (a forced table: filled past half, never to the last entry)
            return e->fail(KWOK_EFULL, "uid directory: %llu entries and %zu more in a table forced to %zu",
                           (unsigned long long)U.live, incoming, U.tab_cap);
        }
    }
    U.inserted += incoming;
    return KWOK_OK;
}
// kwok_uid_bind / kwok_uid_lookup: the spans and the caller's arena on the device
int uid_upload(kwok_engine* e, const int32_t* handles, const char* arena, const uint64_t* off, const uint32_t* len, size_t n,
               uint64_t* arena_len) {
    auto& U = e->uid;
    uint64_t al = 0;
    for (size_t i = 0; i < n; i++)  // (the bytes the spans name; a span past 2^40 is the caller's error)
        if (len[i] && len[i] <= KWOK_UID_MAX && off[i] < (1ull << 40)) al = std::max<uint64_t>(al, off[i] + len[i]);
    int rc = 0;
    if ((rc = U.spans.reserve(e, n)) || (rc = U.arena.reserve(e, al + 1, grown(al) + 1))) return rc;
    hipStream_t st = e->st;
    if (handles) HIPCHK(e, hipMemcpyAsync(U.q_h, handles, n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(U.q_off, off, n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(U.q_len, len, n * 4, hipMemcpyHostToDevice, st));
    if (al) HIPCHK(e, hipMemcpyAsync(U.q_arena, arena, al, hipMemcpyHostToDevice, st));
    *arena_len = al;
    return KWOK_OK;
}
}  // namespace

int kwok_uid_dir_enable(kwok_engine* e) {
    if (!e) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    if (e->multi) return e->fail(KWOK_EINVAL, "kwok_uid_dir_enable: single-rank engines only");
    auto& U = e->uid;
    if (U.on) return KWOK_OK;
    drain(e);
    if (e->poisoned) return poisoned(e);
    if (const char* v = getenv("KWOK_UID_TAB_LOG2")) {
        const int l = atoi(v);
        if (l < 4 || l > 31) return e->fail(KWOK_EINVAL, "KWOK_UID_TAB_LOG2 must be 4..31");
        U.forced_log2 = l;
    }
    int rc = 0;  // (dalloc zeroes: no uid known, an empty table)
    if (!U.ctr) {
        if ((rc = dalloc(e, &U.ctr, 1)) || (rc = dalloc(e, &U.run, 1))) return rc;
        if (hipHostMalloc((void**)&U.ctr_h.p, sizeof(UidCounters), hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc((void**)&U.run_h.p, sizeof(UidRun), hipHostMallocDefault) != hipSuccess)
            return e->fail(KWOK_ENOMEM, "uid directory staging");
        memset(U.ctr_h, 0, sizeof(UidCounters));
    }
    if (!U.pod_uid && (rc = dalloc(e, &U.pod_uid, e->PLa))) return rc;
    if (!U.pod_uid_len && (rc = dalloc(e, &U.pod_uid_len, e->PLa))) return rc;
    if (!U.tab) {
        size_t cap = 64;
        if (U.forced_log2) cap = (size_t)1 << U.forced_log2;
        else
            while (cap < 2 * (uint64_t)e->PL) cap <<= 1;
        if ((rc = dalloc(e, &U.tab, cap))) return rc;
        U.tab_cap = cap;
    }
    HIPCHK(e, hipStreamSynchronize(e->st));
    U.on = true;
    return KWOK_OK;
}

int kwok_uid_bind(kwok_engine* e, const int32_t* handles, const char* arena, const uint64_t* off, const uint32_t* len,
                  size_t n, size_t* n_bad) {
    if (n_bad) *n_bad = 0;
    if (!e || (n && (!handles || !off || !len)) || n > 0x7FFFFFF0ull) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    auto& U = e->uid;
    if (!U.on) return e->fail(KWOK_EINVAL, "kwok_uid_bind: the uid directory is not enabled");
    drain(e);  // (a handle is judged against the state after every submitted tick)
    if (e->poisoned) return poisoned(e);
    if (!n) return KWOK_OK;
    for (size_t i = 0; i < n; i++)
        if (len[i] && len[i] <= KWOK_UID_MAX && !arena) return KWOK_EINVAL;
    int rc = uid_ensure(e, n);
    if (rc) return rc;
    uint64_t al = 0;
    if ((rc = uid_upload(e, handles, arena, off, len, n, &al))) return rc;
    hipStream_t st = e->st;
    HIPCHK(e, hipMemsetAsync(&U.ctr->bad, 0, sizeof(U.ctr->bad), st));
    launch_uid_bind(e->S, U.dir(), U.q_h, U.q_arena, al, U.q_off, U.q_len, (uint32_t)n, st);
    HIPCHK(e, hipGetLastError());
    if ((rc = uid_read_counters(e))) return rc;
    if (n_bad) *n_bad = (size_t)U.ctr_h->bad;
    return KWOK_OK;
}

int kwok_uid_lookup(kwok_engine* e, const char* arena, const uint64_t* off, const uint32_t* len, size_t n,
                    int32_t* out_handles) {
    if (!e || (n && (!off || !len || !out_handles)) || n > 0x7FFFFFF0ull) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    auto& U = e->uid;
    if (!U.on) return e->fail(KWOK_EINVAL, "kwok_uid_lookup: the uid directory is not enabled");
    drain(e);
    if (e->poisoned) return poisoned(e);
    if (!n) return KWOK_OK;
    for (size_t i = 0; i < n; i++)
        if (len[i] && len[i] <= KWOK_UID_MAX && !arena) return KWOK_EINVAL;
    int rc = uid_ensure(e, 0);
    if (rc) return rc;
    uint64_t al = 0;
    if ((rc = uid_upload(e, nullptr, arena, off, len, n, &al))) return rc;
    hipStream_t st = e->st;
    launch_uid_lookup(e->S, U.dir(), U.q_arena, al, U.q_off, U.q_len, (uint32_t)n, U.q_h, st);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(out_handles, U.q_h, n * 4, hipMemcpyDeviceToHost, st));
    return uid_read_counters(e);
}

namespace {
// dev_idx: the frame indices are on the device (the echo entries' kept records; frame_idx null) and the
// results stay there (uid.res_h / res_st / res_rel): nothing is copied back, 0 is returned
int pods_framed_uid_impl(kwok_engine* e, const kwok_codec* c, uint64_t stream_id, const uint32_t* frame_idx,
                         const uint32_t* dev_idx, size_t n, int32_t* out_handles, int32_t* out_status, uint32_t* out_released,
                         size_t* n_host, size_t* n_runs);
}
int kwok_ingest_pods_framed_uid(kwok_engine* e, const kwok_codec* c, uint64_t stream_id, const uint32_t* frame_idx,
                                size_t n, int32_t* out_handles, int32_t* out_status, uint32_t* out_released,
                                size_t* n_host, size_t* n_runs) {
    if (n_host) *n_host = 0;
    if (n_runs) *n_runs = 0;
    if (!e || !c || (n && !frame_idx) || n > 0x7FFFFFF0ull) return KWOK_EINVAL;
    return pods_framed_uid_impl(e, c, stream_id, frame_idx, nullptr, n, out_handles, out_status, out_released, n_host, n_runs);
}
namespace {
int pods_framed_uid_impl(kwok_engine* e, const kwok_codec* c, uint64_t stream_id, const uint32_t* frame_idx,
                         const uint32_t* dev_idx, size_t n, int32_t* out_handles, int32_t* out_status, uint32_t* out_released,
                         size_t* n_host, size_t* n_runs) {
    if (int rc = framed_enter(e, "kwok_ingest_pods_framed_uid", stream_id)) return rc;
    auto& U = e->uid;
    auto& Wt = e->watch;
    auto& J = e->json;
    auto& G = e->ing;
    if (!n) return 0;
    hipStream_t st = e->st;
    const auto t0 = clk::now();
    int rc = 0;
    // the per-record buffers of the call, the decode's and the ingest's sized for the whole batch
    // (a run is a prefix of a range: no later reserve moves them)
    if ((rc = U.recs.reserve(e, n)) || (rc = U.claims.reserve(e, claim_size(n), claim_size(n)))) return rc;
    if ((rc = ingest_reserve(e, n, 0)) || (rc = json_reserve(e, n))) return rc;
    if (dev_idx) HIPCHK(e, hipMemcpyAsync(U.fidx, dev_idx, n * 4, hipMemcpyDeviceToDevice, st));
    else HIPCHK(e, hipMemcpyAsync(U.fidx, frame_idx, n * 4, hipMemcpyHostToDevice, st));
    std::vector<uint32_t> idx_h;  // (dev_idx: fetched for the documents the host completes)
    // KWOK_INGEST_PROF: device-side stamps around k_uid_resolve and around k_uid_claim + k_uid_cut
    ProfEvents<3> pev(e->iprof, e->st);
    float ms_resolve = 0, ms_cut = 0, ms_note = 0;
    UidBatch B{};
    B.stream = Wt.stream;
    B.stream_len = Wt.len;
    B.frames = Wt.frames;
    B.n_frames = (uint32_t)Wt.frames_h.size();
    B.n = (uint32_t)n;
    B.frame_idx = U.fidx;
    B.uoff = U.uoff, B.ulen = U.ulen, B.hash = U.hash, B.cls = U.cls;
    B.doc_off = J.off, B.doc_len = J.len, B.op = J.op, B.handle = J.handle;
    B.claim = U.claim;
    B.run = U.run;
    B.err = &U.ctr->err;
    size_t runs = 0, cuts = 0, host_docs = 0;
    for (size_t lo = 0; lo < n;) {
        const size_t range = n - lo;
        if ((rc = uid_ensure(e, 0))) return rc;  // (the table sized for the slots before it is probed)
        const size_t cm = claim_size(range);
        B.lo = (uint32_t)lo;
        B.claim_mask = (uint32_t)(cm - 1);
        U.run_h->first_cut = ~0u, U.run_h->n_sent = 0, U.run_h->n_new = 0, U.run_h->pad = 0;
        HIPCHK(e, hipMemcpyAsync(U.run, U.run_h, sizeof(UidRun), hipMemcpyHostToDevice, st));
        HIPCHK(e, hipMemsetAsync(U.claim, 0xFF, cm * 4, st));
        pev.stamp(0);
        launch_uid_resolve(e->S, U.dir(), B, st);
        pev.stamp(1);
        launch_uid_cut(B, st);
        pev.stamp(2);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipMemcpyAsync(U.run_h, U.run, sizeof(UidRun), hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipStreamSynchronize(st));
        ms_resolve += pev.elapsed(0, 1), ms_cut += pev.elapsed(1, 2);
        const size_t cut = std::min<size_t>(U.run_h->first_cut, n);
        if (cut <= lo) return e->fail(KWOK_EDEVICE, "uid directory: a run of no records at %zu", lo);
        const size_t m = cut - lo;
        // (a cut run holds the create that caused the cut; an uncut one is the whole range, whose count this is)
        const bool sends = cut < n || U.run_h->n_sent;
        if (cut < n) cuts++;
        const int32_t *rh = nullptr, *rs = nullptr;
        const uint32_t* rr = nullptr;
        if (sends) {
            runs++;
            Wt.stats[KWOK_WATCH_STAT_INGESTS]++;
            // (room for the run's creates: the range's count, which bounds a cut run's)
            if ((rc = uid_ensure(e, std::min<size_t>(m, U.run_h->n_new)))) return rc;
            uint32_t nh = 0;
            if ((rc = json_decode(e, c, Wt.host, Wt.len, nullptr, nullptr, m, nullptr, nullptr, &nh, Wt.stream, true))) return rc;
            if (nh) {  // the documents the scanner listed for the host codec: their spans, ops and the run's handles
                std::vector<uint64_t> off;
                std::vector<uint32_t> len;
                std::vector<uint8_t> op;
                std::vector<int32_t> hv(m);
                if (dev_idx && idx_h.empty()) {
                    idx_h.resize(n);
                    HIPCHK(e, hipMemcpyAsync(idx_h.data(), U.fidx, n * 4, hipMemcpyDeviceToHost, st));
                    HIPCHK(e, hipStreamSynchronize(st));
                }
                if ((rc = framed_records(e, stream_id, (dev_idx ? idx_h.data() : frame_idx) + lo, m, off, len, op))) return rc;
                HIPCHK(e, hipMemcpyAsync(hv.data(), J.handle, m * 4, hipMemcpyDeviceToHost, st));
                HIPCHK(e, hipStreamSynchronize(st));
                if ((rc = json_complete(e, c, Wt.host, Wt.len, off.data(), len.data(), nh, op.data(), hv.data(), nullptr, nullptr)))
                    return rc;
                host_docs += nh;
            }
            const UidNote N{Wt.stream, U.uoff + lo, U.ulen + lo, U.hash + lo, U.cls + lo};
            ScopedPtr<UidNote> note(e->uid.note, &N);  // the ingest notes the run's creates with their uids
            const RefNote RN{Wt.stream, Wt.len, Wt.frames, B.n_frames, U.fidx + lo, U.cls + lo};
            ScopedPtr<RefNote> ref_note(e->refs.note, &RN);  // ... and, with the reference directory, with their names
            ScopedPtr<uint8_t> src(e->ing.arena_src, Wt.stream);
            rc = ingest_pods_impl(e, G.d_ev, 0, m, nullptr, Wt.len, nullptr, nullptr, nullptr, nullptr, true);
            for (size_t q = 0; q + 1 < U.note_ev.size(); q += 2) {  // (the batch is synchronised, or failed)
                float ms = 0;
                if (rc >= 0 && hipEventElapsedTime(&ms, U.note_ev[q], U.note_ev[q + 1]) == hipSuccess) ms_note += ms;
                (void)hipEventDestroy(U.note_ev[q]);
                (void)hipEventDestroy(U.note_ev[q + 1]);
            }
            U.note_ev.clear();
            if (rc < 0) return rc;
            rh = G.out_handle, rs = G.out_status, rr = G.out_released;
        }
        // (a run that sends nothing holds withheld records only: k_uid_fix reads no result of the ingest for them)
        launch_uid_fix(B, (uint32_t)m, rh ? rh : U.res_h, rs ? rs : U.res_st, rr ? rr : U.res_rel, U.res_h, U.res_st, U.res_rel, st);
        HIPCHK(e, hipGetLastError());
        lo = cut;
    }
    if (dev_idx) {
        if ((rc = uid_read_counters(e))) return rc;
        U.stats[KWOK_UID_STAT_RUNS] += runs;
        U.stats[KWOK_UID_STAT_CUTS] += cuts;
        if (n_host) *n_host = host_docs;
        if (n_runs) *n_runs = runs;
        return 0;
    }
    if (out_handles) HIPCHK(e, hipMemcpyAsync(out_handles, U.res_h, n * 4, hipMemcpyDeviceToHost, st));
    if (out_released) HIPCHK(e, hipMemcpyAsync(out_released, U.res_rel, n * 4, hipMemcpyDeviceToHost, st));
    std::vector<int32_t> st_tmp(out_status ? 0 : n);
    int32_t* sts = out_status ? out_status : st_tmp.data();
    HIPCHK(e, hipMemcpyAsync(sts, U.res_st, n * 4, hipMemcpyDeviceToHost, st));
    if ((rc = uid_read_counters(e))) return rc;
    int rejected = 0;
    for (size_t i = 0; i < n; i++) rejected += sts[i] != KWOK_OK && sts[i] != KWOK_NOT_SENT;
    U.stats[KWOK_UID_STAT_RUNS] += runs;
    U.stats[KWOK_UID_STAT_CUTS] += cuts;
    if (n_host) *n_host = host_docs;
    if (n_runs) *n_runs = runs;
    if (e->iprof)
        fprintf(stderr, "[kwok uid] %zu frames, %zu run%s (%zu by the host): k_uid_resolve %.3f ms, k_uid_claim + k_uid_cut %.3f ms, "
                        "k_uid_note %.3f ms; the call %.2f ms\n", n, runs, runs == 1 ? "" : "s", host_docs, ms_resolve, ms_cut,
                ms_note, ms_between(t0, clk::now()));
    return rejected;
}
}  // namespace

int kwok_uid_stats(kwok_engine* e, uint64_t out[KWOK_UID_STAT_COUNT]) {
    if (!e || !out) return KWOK_EINVAL;
    auto& U = e->uid;
    if (U.ctr && !e->poisoned)
        if (int rc = uid_read_counters(e)) return rc;
    for (int k = 0; k < KWOK_UID_STAT_COUNT; k++) out[k] = U.stats[k];
    if (U.ctr_h) {
        out[KWOK_UID_STAT_LOOKUPS] = U.ctr_h->lookups;
        out[KWOK_UID_STAT_HITS] = U.ctr_h->hits;
        out[KWOK_UID_STAT_BINDS] = U.ctr_h->binds;
        out[KWOK_UID_STAT_UNBOUND] = U.ctr_h->unbound;
        out[KWOK_UID_STAT_TABLE_ENTRIES] = U.ctr_h->entries;
    }
    return KWOK_OK;
}

// ---- the echo ledger (kwok_watch.h, echo.hip) ----------------------------------------
namespace {
int echo_read(kwok_engine* e, bool call) {
    auto& E = e->echo;
    if (call) HIPCHK(e, hipMemcpyAsync(E.call_h, E.call, sizeof(EchoCall), hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipMemcpyAsync(E.ctr_h, E.ctr, sizeof(EchoCounters), hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    if (E.ctr_h->err || (call && E.call_h->err)) {
        e->poisoned = true;
        return e->fail(KWOK_EDEVICE, "echo ledger: a probe wrapped a whole table (ledger %u, call %u)", E.ctr_h->err,
                       call ? E.call_h->err : 0u);
    }
    return KWOK_OK;
}
// every entry that holds a note into a fresh pool and table of tab_cap entries (k_echo_rebuild)
int echo_rebuild(kwok_engine* e, size_t tab_cap) {
    auto& E = e->echo;
    hipStream_t st = e->st;
    const EchoLedger from = E.ledger();
    const uint32_t used = E.ctr_h->used;
    uint32_t* tab = nullptr;
    EchoEntry* pool = nullptr;
    const size_t pool_cap = E.forced_log2 ? tab_cap - 1 : tab_cap / 2;
    int rc = 0;
    if ((rc = dalloc(e, &tab, tab_cap))) return rc;
    if ((rc = dalloc(e, &pool, pool_cap))) {
        dfree(tab);
        return rc;
    }
    const EchoLedger to{tab, (uint32_t)(tab_cap - 1), pool, (uint32_t)pool_cap, E.ctr};
    HIPCHK(e, hipMemsetAsync(&E.ctr->used, 0, sizeof(uint32_t), st));
    launch_echo_rebuild(from, to, used, st);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(st));
    E.tab.reset(tab), E.pool.reset(pool);
    E.tab_cap = tab_cap, E.pool_cap = pool_cap;
    E.rebuilds++;
    if ((rc = echo_read(e, false))) return rc;
    if (E.ctr_h->used != E.ctr_h->live) {
        e->poisoned = true;
        return e->fail(KWOK_EDEVICE, "echo ledger: %u entries rebuilt, %llu uids hold a note", E.ctr_h->used,
                       (unsigned long long)E.ctr_h->live);
    }
    return KWOK_OK;
}
// before a launch that may insert `incoming` entries: room in the pool, the table at most half full
// (a forced table: never to its last entry); emptied entries are compacted away first
int echo_ensure(kwok_engine* e, size_t incoming) {
    auto& E = e->echo;
    const uint64_t used = E.ctr_h->used, live = E.ctr_h->live;
    if (used + incoming <= E.pool_cap) return KWOK_OK;
    if (E.forced_log2) {
        if (live + incoming > E.pool_cap)
            return e->fail(KWOK_EFULL, "echo ledger: %llu uids and %zu more in a table forced to %zu", (unsigned long long)live,
                           incoming, E.tab_cap);
        return echo_rebuild(e, E.tab_cap);
    }
    size_t cap = 64;
    while (cap < 2 * (live + incoming)) cap <<= 1;
    if (cap > ((size_t)1 << 31)) return e->fail(KWOK_EFULL, "echo ledger: %llu uids", (unsigned long long)(live + incoming));
    return echo_rebuild(e, std::max(cap, E.tab_cap));
}
// the per-record buffers of a call of n records, cleared for it
int echo_reserve(kwok_engine* e, size_t n) {
    auto& E = e->echo;
    int rc = 0;
    const size_t ccap = claim_size(n);
    if ((rc = E.recs.reserve(e, n)) || (rc = E.claims.reserve(e, ccap, ccap))) return rc;
    hipStream_t st = e->st;
    HIPCHK(e, hipMemsetAsync(E.claim, 0xFF, ccap * 4, st));
    HIPCHK(e, hipMemsetAsync(E.cnt, 0, n * 4, st));
    HIPCHK(e, hipMemsetAsync(E.fill, 0, n * 4, st));
    HIPCHK(e, hipMemsetAsync(E.call, 0, sizeof(EchoCall), st));
    return KWOK_OK;
}
EchoBatch echo_batch(kwok_engine* e, const uint8_t* base, uint64_t base_len, size_t n) {
    auto& E = e->echo;
    EchoBatch B{};
    B.base = base, B.base_len = base_len, B.n = (uint32_t)n;
    B.uoff = E.uoff, B.roff = E.roff, B.ulen = E.ulen, B.rlen = E.rlen, B.hash = E.hash, B.kind = E.kind, B.res = E.res;
    B.claim = E.claim, B.claim_mask = (uint32_t)(claim_size(n) - 1);
    B.own = E.own, B.cnt = E.cnt, B.fill = E.fill, B.lbase = E.lbase, B.list = E.list;
    B.call = E.call;
    return B;
}
// the typed front end's spans and the bytes they name on the device (the arena's used prefix: *arena_len)
int echo_upload(kwok_engine* e, const uint8_t* op, const char* arena, const uint64_t* uid_off, const uint32_t* uid_len,
                const uint64_t* rv_off, const uint32_t* rv_len, size_t n, uint64_t* arena_len, EchoSpans* P) {
    auto& E = e->echo;
    uint64_t al = 0;
    for (size_t i = 0; i < n; i++) {  // (a span past 2^32 names no byte of the upload: the device refuses it)
        if (uid_len[i] && uid_len[i] <= KWOK_UID_MAX && uid_off[i] < 0xFFFFFF00ull) al = std::max<uint64_t>(al, uid_off[i] + uid_len[i]);
        if (rv_len[i] && rv_len[i] <= KWOK_RV_MAX && rv_off[i] < 0xFFFFFF00ull) al = std::max<uint64_t>(al, rv_off[i] + rv_len[i]);
    }
    if (al && !arena) return KWOK_EINVAL;
    int rc = 0;
    if ((rc = E.spans.reserve(e, n)) || (rc = E.bytes.reserve(e, al + 1, grown(al) + 1))) return rc;
    hipStream_t st = e->st;
    HIPCHK(e, hipMemcpyAsync(E.s_uoff, uid_off, n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(E.s_roff, rv_off, n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(E.s_ulen, uid_len, n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(E.s_rlen, rv_len, n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(E.s_op, op, n, hipMemcpyHostToDevice, st));
    if (al) HIPCHK(e, hipMemcpyAsync(E.arena, arena, al, hipMemcpyHostToDevice, st));
    *arena_len = al;
    *P = EchoSpans{E.s_uoff, E.s_roff, E.s_ulen, E.s_rlen, E.s_op};
    return KWOK_OK;
}
// the checks every echo entry makes before it touches anything
int echo_enter(kwok_engine* e, const char* who) {
    if (e->poisoned) return poisoned(e);
    if (!e->echo.on) return e->fail(KWOK_EINVAL, "%s: the echo ledger is not enabled", who);
    drain(e);
    if (e->poisoned) return poisoned(e);
    return KWOK_OK;
}
// the filter over all frames of a batch; on return the call's counts are on the host, the kept
// records' frame indices (E.kidx, E.call_h->n_keep of them) and each record's answer on the device
int echo_filter_frames(kwok_engine* e, const uint32_t* frame_idx, size_t n, EchoBatch* Bo, EchoFrames* Fo, EchoKeep* Ko) {
    auto& E = e->echo;
    auto& Wt = e->watch;
    hipStream_t st = e->st;
    int rc = echo_reserve(e, n);
    if (rc) return rc;
    HIPCHK(e, hipMemcpyAsync(E.fidx, frame_idx, n * 4, hipMemcpyHostToDevice, st));
    const EchoBatch B = echo_batch(e, Wt.stream, Wt.len, n);
    const EchoFrames F{Wt.frames, (uint32_t)Wt.frames_h.size(), E.fidx};
    const EchoKeep K{E.bsum, E.kidx, E.kpos, E.q_off, E.q_len};
    ProfEvents<2> pev(e->iprof, e->st);
    pev.stamp(0);
    launch_echo_key_frames(B, F, st);
    launch_echo_group(B, st);
    launch_echo_decide(E.ledger(), B, st);
    launch_echo_keep(B, F, K, st);
    pev.stamp(1);
    HIPCHK(e, hipGetLastError());
    if ((rc = echo_read(e, true))) return rc;
    if (pev.on())
        fprintf(stderr, "[kwok echo] %zu frames, %u echoes, %u repeats: the echo kernels %.3f ms\n", n, E.call_h->n_drop,
                E.call_h->n_rep, pev.elapsed(0, 1));
    if (E.call_h->n_keep > n) return e->fail(KWOK_EDEVICE, "echo ledger: %u of %zu records kept", E.call_h->n_keep, n);
    *Bo = B, *Fo = F, *Ko = K;
    return KWOK_OK;
}
}  // namespace

int kwok_echo_enable(kwok_engine* e) {
    if (!e) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    if (e->multi) return e->fail(KWOK_EINVAL, "kwok_echo_enable: single-rank engines only");
    auto& E = e->echo;
    if (E.on) return KWOK_OK;
    if (const char* v = getenv("KWOK_ECHO_TAB_LOG2")) {
        const int l = atoi(v);
        if (l < 4 || l > 31) return e->fail(KWOK_EINVAL, "KWOK_ECHO_TAB_LOG2 must be 4..31");
        E.forced_log2 = l;
    }
    int rc = 0;  // (dalloc zeroes: an empty table, no note)
    if (!E.ctr) {
        if ((rc = dalloc(e, &E.ctr, 1)) || (rc = dalloc(e, &E.call, 1))) return rc;
        if (hipHostMalloc((void**)&E.ctr_h.p, sizeof(EchoCounters), hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc((void**)&E.call_h.p, sizeof(EchoCall), hipHostMallocDefault) != hipSuccess)
            return e->fail(KWOK_ENOMEM, "echo ledger staging");
        memset(E.ctr_h, 0, sizeof(EchoCounters));
        memset(E.call_h, 0, sizeof(EchoCall));
    }
    if (!E.tab) {
        const size_t cap = E.forced_log2 ? (size_t)1 << E.forced_log2 : 64;
        const size_t pcap = E.forced_log2 ? cap - 1 : cap / 2;
        if ((rc = dalloc(e, &E.tab, cap))) return rc;
        if ((rc = dalloc(e, &E.pool, pcap))) return rc;
        E.tab_cap = cap, E.pool_cap = pcap;
    }
    HIPCHK(e, hipStreamSynchronize(e->st));
    E.on = true;
    return KWOK_OK;
}

int kwok_echo_update(kwok_engine* e, const uint8_t* op, const char* arena, const uint64_t* uid_off,
                     const uint32_t* uid_len, const uint64_t* rv_off, const uint32_t* rv_len, size_t n,
                     int32_t* out_status) {
    if (!e || (n && (!op || !uid_off || !uid_len || !rv_off || !rv_len)) || n > 0x7FFFFFF0ull) return KWOK_EINVAL;
    int rc = echo_enter(e, "kwok_echo_update");
    if (rc) return rc;
    if (!n) return 0;
    auto& E = e->echo;
    uint64_t al = 0;
    EchoSpans P{};
    if ((rc = echo_upload(e, op, arena, uid_off, uid_len, rv_off, rv_len, n, &al, &P))) return rc;
    if ((rc = echo_reserve(e, n))) return rc;
    hipStream_t st = e->st;
    const EchoBatch B = echo_batch(e, E.arena, al, n);
    launch_echo_key_update(B, P, E.s_status, st);
    launch_echo_group(B, st);
    launch_echo_need(E.ledger(), B, st);
    HIPCHK(e, hipGetLastError());
    // the room the call needs, before anything is stored: compacted, grown or refused here
    if ((rc = echo_read(e, true)) || (rc = echo_ensure(e, E.call_h->n_new))) return rc;
    launch_echo_update(E.ledger(), B, st);
    HIPCHK(e, hipGetLastError());
    if (out_status) HIPCHK(e, hipMemcpyAsync(out_status, E.s_status, n * 4, hipMemcpyDeviceToHost, st));
    if ((rc = echo_read(e, true))) return rc;
    return (int)E.call_h->n_bad;
}

// kwok_echo_update's notes with the pairs read from the resident frames (kwok_response.h): only the keying
// front end differs, the grouping, the room check and the apply are kwok_echo_update's
int kwok_echo_note_framed(kwok_engine* e, uint64_t stream_id, const uint32_t* frame_idx, size_t n, int32_t* out_status) {
    if (!e || (n && !frame_idx) || n > 0x7FFFFFF0ull) return KWOK_EINVAL;
    int rc = echo_enter(e, "kwok_echo_note_framed");
    if (rc) return rc;
    if ((rc = stream_resident(e, stream_id))) return rc;
    auto& E = e->echo;
    auto& Wt = e->watch;
    Wt.rstats[KWOK_RESP_STAT_NOTE_CALLS]++;
    if (!n) return 0;
    if ((rc = echo_reserve(e, n))) return rc;
    hipStream_t st = e->st;
    HIPCHK(e, hipMemcpyAsync(E.fidx, frame_idx, n * 4, hipMemcpyHostToDevice, st));
    const EchoBatch B = echo_batch(e, Wt.stream, Wt.len, n);
    const EchoFrames F{Wt.frames, (uint32_t)Wt.frames_h.size(), E.fidx};
    launch_echo_key_note_frames(B, F, E.res_st, st);
    launch_echo_group(B, st);
    launch_echo_need(E.ledger(), B, st);
    HIPCHK(e, hipGetLastError());
    // the room the call needs, before anything is stored: compacted, grown or refused here
    if ((rc = echo_read(e, true)) || (rc = echo_ensure(e, E.call_h->n_new))) return rc;
    launch_echo_update(E.ledger(), B, st);
    HIPCHK(e, hipGetLastError());
    if (out_status) HIPCHK(e, hipMemcpyAsync(out_status, E.res_st, n * 4, hipMemcpyDeviceToHost, st));
    if ((rc = echo_read(e, true))) return rc;
    Wt.rstats[KWOK_RESP_STAT_NOTES] += E.call_h->n_note;
    return (int)E.call_h->n_bad;
}

int kwok_echo_match(kwok_engine* e, const char* arena, const uint64_t* uid_off, const uint32_t* uid_len,
                    const uint64_t* rv_off, const uint32_t* rv_len, const uint8_t* deleted, size_t n,
                    uint8_t* out_drop) {
    if (!e || (n && (!uid_off || !uid_len || !rv_off || !rv_len || !deleted || !out_drop)) || n > 0x7FFFFFF0ull)
        return KWOK_EINVAL;
    int rc = echo_enter(e, "kwok_echo_match");
    if (rc) return rc;
    if (!n) return KWOK_OK;
    auto& E = e->echo;
    uint64_t al = 0;
    EchoSpans P{};
    if ((rc = echo_upload(e, deleted, arena, uid_off, uid_len, rv_off, rv_len, n, &al, &P))) return rc;
    if ((rc = echo_reserve(e, n))) return rc;
    hipStream_t st = e->st;
    const EchoBatch B = echo_batch(e, E.arena, al, n);
    launch_echo_key_typed(B, P, st);
    launch_echo_group(B, st);
    launch_echo_decide(E.ledger(), B, st);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(out_drop, E.res, n, hipMemcpyDeviceToHost, st));  // (ER_KEEP 0, ER_DROP 1)
    return echo_read(e, true);
}

int kwok_ingest_pods_framed_echo(kwok_engine* e, const kwok_codec* c, uint64_t stream_id, const uint32_t* frame_idx,
                                 size_t n, int32_t* out_handles, int32_t* out_status, uint32_t* out_released,
                                 size_t* n_host, size_t* n_runs, size_t* n_echoes) {
    if (n_host) *n_host = 0;
    if (n_runs) *n_runs = 0;
    if (n_echoes) *n_echoes = 0;
    if (!e || !c || (n && !frame_idx) || n > 0x7FFFFFF0ull) return KWOK_EINVAL;
    int rc = echo_enter(e, "kwok_ingest_pods_framed_echo");
    if (rc) return rc;
    auto& E = e->echo;
    auto& U = e->uid;
    auto& Wt = e->watch;
    if (!U.on) return e->fail(KWOK_EINVAL, "kwok_ingest_pods_framed_echo: the uid directory is not enabled");
    if ((rc = stream_resident(e, stream_id))) return rc;
    if (!n) return 0;
    hipStream_t st = e->st;
    EchoBatch B{};
    EchoFrames F{};
    EchoKeep K{};
    if ((rc = echo_filter_frames(e, frame_idx, n, &B, &F, &K))) return rc;
    const size_t nk = E.call_h->n_keep, nd = E.call_h->n_drop;
    if (nd) {  // the echoes' live handles, before the kept records change anything
        if ((rc = uid_ensure(e, 0))) return rc;
        launch_uid_lookup(e->S, U.dir(), Wt.stream, Wt.len, K.q_off, K.q_len, (uint32_t)n, E.hdrop, st);
        HIPCHK(e, hipGetLastError());
    }
    if (nk && (rc = pods_framed_uid_impl(e, c, stream_id, nullptr, E.kidx, nk, nullptr, nullptr, nullptr, n_host, n_runs)) < 0)
        return rc;
    // (no kept record: k_echo_fix reads no result of the ingest)
    launch_echo_fix(B, K, E.hdrop, nk ? U.res_h : E.res_h, nk ? U.res_st : E.res_st, nk ? U.res_rel : E.res_rel, E.res_h, E.res_st,
                    E.res_rel, st);
    HIPCHK(e, hipGetLastError());
    if (out_handles) HIPCHK(e, hipMemcpyAsync(out_handles, E.res_h, n * 4, hipMemcpyDeviceToHost, st));
    if (out_released) HIPCHK(e, hipMemcpyAsync(out_released, E.res_rel, n * 4, hipMemcpyDeviceToHost, st));
    std::vector<int32_t> st_tmp(out_status ? 0 : n);
    int32_t* sts = out_status ? out_status : st_tmp.data();
    HIPCHK(e, hipMemcpyAsync(sts, E.res_st, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    int rejected = 0;
    for (size_t i = 0; i < n; i++) rejected += sts[i] != KWOK_OK && sts[i] != KWOK_NOT_SENT && sts[i] != KWOK_ECHO;
    if (n_echoes) *n_echoes = nd;
    return rejected;
}

namespace {
// The device-input form of kwok_ingest_nodes_framed (the node directory on): record k is frame didx[k] of the
// resident stream, didx a device-resident list that names ingestible frames only (the echo filter's kept records).
// k_nd_frame_recs writes the decode's inputs and the uid spans, k_json_nodes runs over the resident stream in one
// piece, the documents it lists for the host are completed as kwok_ingest_nodes_json completes them (their indices
// and the list fetched only when there are any; their spans from Wt.frames_h), ingest_nodes_impl applies the
// records where they are, the note follows.  Nothing per record comes back: the apply's handles and statuses stay
// in ing.out_handle / out_status, the decode's in json.nstat, for k_nd_echo_fix.  The caller drained and checked
// the stream.  Returns the apply's rejected count (not the call's), or an error.
int nodes_framed_dev_impl(kwok_engine* e, const kwok_codec* c, const uint32_t* didx, size_t n, size_t* n_host) {
    auto& Wt = e->watch;
    auto& G = e->ing;
    auto& J = e->json;
    auto& D = e->ndir;
    hipStream_t st = e->st;
    e->emit_hint = true;
    e->quiet = 0;
    e->state_changed();
    Wt.stats[KWOK_WATCH_STAT_INGESTS]++;
    int rc = 0;
    if ((rc = node_reserve(e, n, 0)) || (rc = json_reserve(e, n)) || (rc = J.node_docs.reserve(e, n)) || (rc = D.recs.reserve(e, n)))
        return rc;
    auto& C = e->canon;
    C.doc_h.clear();
    if (C.on && (rc = canon_reserve(e, n))) return rc;
    if ((rc = codec_export(c, J.cfg_h))) {  // (selectors beyond the device tables: every document to the host)
        if (rc != KWOK_EDOMAIN) return e->fail(rc, "%s", kwok_codec_last_error());
        memset(J.cfg_h, 0, sizeof(JsonCfg));
        J.cfg_h->all_host = 1;
    }
    HIPCHK(e, hipMemcpyAsync(J.cfg, J.cfg_h, sizeof(JsonCfg), hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemsetAsync(J.n_host, 0, 4, st));
    HIPCHK(e, hipMemsetAsync(&D.call->err, 0, sizeof(D.call->err), st));
    launch_nd_frame_recs(Wt.frames, (uint32_t)Wt.frames_h.size(), Wt.len, didx, (uint32_t)n, true, J.off, J.len, J.op, D.uoff, D.ulen,
                         &D.call->err, st);
    HIPCHK(e, hipGetLastError());
    JsonNodeArgs A{};
    A.arena = Wt.stream;
    A.arena_len = Wt.len;
    A.doc_off = J.off, A.doc_len = J.len, A.op = J.op;
    A.n = (uint32_t)n;
    A.cfg = J.cfg;
    A.ev = G.d_nev;
    A.status = J.nstat;
    A.host_list = J.host_list;
    A.n_host = J.n_host;
    A.base = 0;
    A.canon_list = C.on ? C.list.p : nullptr;
    A.canon_ctr = C.ctr;
    launch_json_nodes(A, st);
    HIPCHK(e, hipGetLastError());
    if (C.on && (rc = json_nodes_canon(e, Wt.stream))) return rc;
    HIPCHK(e, hipMemcpyAsync(J.n_host_h, J.n_host, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(D.call_h, D.call, sizeof(*D.call_h.p), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    if (D.call_h->err) {  // (an engine bug: the echo filter kept an index that names no ingestible frame)
        e->poisoned = true;
        return e->fail(KWOK_EDEVICE, "device-input node ingest: a kept index names no ingestible frame");
    }
    const uint32_t nh = *J.n_host_h;
    if (nh > n) return e->fail(KWOK_EDEVICE, "device-input node ingest: %u of %zu documents listed", nh, n);
    std::unordered_map<uint32_t, uint32_t> hdoc;
    std::vector<kwok_node_event> hrec;
    std::vector<std::string> hbuf;
    if (nh) {
        std::vector<uint32_t> list, kidx(n);
        std::vector<int32_t> hstat;
        HIPCHK(e, hipMemcpyAsync(kidx.data(), didx, n * 4, hipMemcpyDeviceToHost, st));
        if ((rc = json_nodes_listed(e, nh, list))) return rc;  // (synchronises: kidx is here too)
        if (!listed_in_range(list, kidx, Wt.frames_h.size())) return e->fail(KWOK_EDEVICE, "device-input node ingest: a listed document out of range");
        if ((rc = nodes_complete_listed(e, c, Wt.host, list, [&](uint32_t i, uint64_t* o, uint32_t* l, uint8_t* p) {
                const kwok_watch_frame& f = Wt.frames_h[kidx[i]];
                *o = f.doc_off, *l = f.doc_len, *p = f.type == KWOK_WATCH_DELETED ? KWOK_OP_DELETE : KWOK_OP_UPSERT;
            }, hstat, hdoc, hrec, hbuf)))
            return rc;
        // the host codec's statuses of those documents, beside the device's in json.nstat
        HIPCHK(e, hipMemcpyAsync(D.hstat, hstat.data(), (size_t)nh * 4, hipMemcpyHostToDevice, st));
        launch_nd_stat_scatter(J.nstat, J.host_list, D.hstat, nh, st);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipStreamSynchronize(st));  // (hstat is read by the copy above)
    }
    if (n_host) *n_host = nh;
    const NodeUidNote un{Wt.stream, Wt.len, D.uoff, D.ulen};
    ScopedPtr<NodeUidNote> uids(D.note, &un);
    ScopedPtr<uint8_t> src(G.arena_src, Wt.stream);  // the ingest kernels read the batch's strings from the resident stream
    NodeJsonCtx ctx{Wt.host, &hdoc, &hrec, &hbuf, e->canon.on ? &e->canon : nullptr};
    return ingest_nodes_impl(e, nullptr, n, Wt.host, Wt.len, nullptr, nullptr, &ctx);
}
}  // namespace

int kwok_ingest_nodes_framed_echo(kwok_engine* e, const kwok_codec* c, uint64_t stream_id, const uint32_t* frame_idx,
                                  size_t n, int32_t* out_handles, int32_t* out_status, size_t* n_host,
                                  size_t* n_echoes) {
    if (n_host) *n_host = 0;
    if (n_echoes) *n_echoes = 0;
    if (!e || !c || (n && !frame_idx) || n > 0x7FFFFFF0ull) return KWOK_EINVAL;
    int rc = echo_enter(e, "kwok_ingest_nodes_framed_echo");
    if (rc) return rc;
    auto& E = e->echo;
    if ((rc = stream_resident(e, stream_id))) return rc;
    if (!n) return 0;
    hipStream_t st = e->st;
    EchoBatch B{};
    EchoFrames F{};
    EchoKeep K{};
    if ((rc = echo_filter_frames(e, frame_idx, n, &B, &F, &K))) return rc;
    const size_t nk = E.call_h->n_keep, nd = E.call_h->n_drop;
    if (e->ndir.on) {
        // the node directory on: the kept records are ingested from the resident frames by the device-resident
        // index list, every answer is merged on the device, two arrays and one word come back
        auto& D = e->ndir;
        auto& G = e->ing;
        const auto t0 = clk::now();
        ProfEvents<2> pev(e->iprof, st);  // KWOK_INGEST_PROF: everything of the call behind the echo filter
        pev.stamp(0);
        if (nd) {
            launch_nd_lookup_frames(e->S, D.dir(), B, F, E.hdrop, st);
            HIPCHK(e, hipGetLastError());
        }
        if (nk && (rc = nodes_framed_dev_impl(e, c, E.kidx, nk, n_host)) < 0) return rc;
        HIPCHK(e, hipMemsetAsync(&D.call->rejected, 0, sizeof(D.call->rejected), st));
        launch_nd_echo_fix(B, K, (uint32_t)nk, E.hdrop, G.out_handle, G.out_status, e->json.nstat, E.res_h, E.res_st,
                           &D.call->rejected, st);
        HIPCHK(e, hipGetLastError());
        pev.stamp(1);
        if (out_handles) HIPCHK(e, hipMemcpyAsync(out_handles, E.res_h, n * 4, hipMemcpyDeviceToHost, st));
        if (out_status) HIPCHK(e, hipMemcpyAsync(out_status, E.res_st, n * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipMemcpyAsync(D.call_h, D.call, sizeof(*D.call_h.p), hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipStreamSynchronize(st));
        if (pev.on())
            fprintf(stderr, "[kwok nodes] %zu frames, %zu kept, %zu echoes: lookup + device-input ingest + merge %.3f ms on the device "
                            "(host waits of the ingest included), %.3f ms wall; 8 bytes per record back\n", n, nk, nd, pev.elapsed(0, 1),
                    ms_between(t0, clk::now()));
        if (n_echoes) *n_echoes = nd;
        return (int)D.call_h->rejected;
    }
    // the node ingest takes its records from the host: the kept indices come back (4 bytes per kept
    // record), with every record's answer (1 byte) and, if any, the echoes' handles
    std::vector<uint32_t> kidx(nk), kpos(n);
    std::vector<uint8_t> res(n);
    std::vector<int32_t> hdrop(nd ? n : 0);
    if (nd) {
        launch_echo_node_handles(e->S, B, F, E.hdrop, st);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipMemcpyAsync(hdrop.data(), E.hdrop, n * 4, hipMemcpyDeviceToHost, st));
    }
    if (nk) HIPCHK(e, hipMemcpyAsync(kidx.data(), E.kidx, nk * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(kpos.data(), E.kpos, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(res.data(), E.res, n, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    std::vector<int32_t> kh(nk), ks(nk);
    if (nk && (rc = kwok_ingest_nodes_framed(e, c, stream_id, kidx.data(), nk, kh.data(), ks.data(), n_host)) < 0) return rc;
    int rejected = 0;
    for (size_t i = 0; i < n; i++) {
        int32_t h = -1, s = KWOK_EINVAL;
        if (res[i] == ER_KEEP && kpos[i] < nk) h = kh[kpos[i]], s = ks[kpos[i]];
        else if (res[i] == ER_DROP) h = hdrop[i], s = KWOK_ECHO;
        else if (res[i] == ER_EDOMAIN) s = KWOK_EDOMAIN;
        if (out_handles) out_handles[i] = h;
        if (out_status) out_status[i] = s;
        rejected += s != KWOK_OK && s != KWOK_ECHO;
    }
    if (n_echoes) *n_echoes = nd;
    return rejected;
}

int kwok_echo_stats(kwok_engine* e, uint64_t out[KWOK_ECHO_STAT_COUNT]) {
    if (!e || !out) return KWOK_EINVAL;
    auto& E = e->echo;
    for (int k = 0; k < KWOK_ECHO_STAT_COUNT; k++) out[k] = 0;
    if (!E.ctr_h) return KWOK_OK;
    out[KWOK_ECHO_STAT_NOTES] = E.ctr_h->notes;
    out[KWOK_ECHO_STAT_FORGETS] = E.ctr_h->forgets;
    out[KWOK_ECHO_STAT_EVICTIONS] = E.ctr_h->evictions;
    out[KWOK_ECHO_STAT_MATCHED] = E.ctr_h->matched;
    out[KWOK_ECHO_STAT_DROPPED] = E.ctr_h->dropped;
    out[KWOK_ECHO_STAT_KEPT_MATCHED] = E.ctr_h->kept_matched;
    out[KWOK_ECHO_STAT_REBUILDS] = E.rebuilds;
    out[KWOK_ECHO_STAT_LIVE_UIDS] = E.ctr_h->live;
    out[KWOK_ECHO_STAT_TABLE_ENTRIES] = E.ctr_h->used;
    return KWOK_OK;
}

// ---- the pod and node reference directory (kwok_watch.h, refs.hip) -------------------
namespace {
int refs_read_counters(kwok_engine* e) {
    auto& R = e->refs;
    HIPCHK(e, hipMemcpyAsync(R.ctr_h, R.ctr, sizeof(RefCounters), hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    return KWOK_OK;
}
// items [first, first + n) of the device handle list `handles`: sizes, scan, gather, then refs[] and the blob to
// the caller (on the engine stream: behind every ingest and every submitted tick)
int refs_query(kwok_engine* e, const char* who, const int32_t* handles, size_t first, size_t n, bool pods, bool any_slot,
               kwok_ref* refs, char* blob, size_t blob_cap, size_t* blob_used) {
    auto& R = e->refs;
    hipStream_t st = e->st;
    if (!n) return KWOK_OK;
    int rc = 0;
    if ((rc = R.items.reserve(e, n))) return rc;
    const size_t tmp = refs_scan_bytes((uint32_t)n);
    if (tmp > R.tmp_bytes) {
        R.q_tmp.release(), R.tmp_bytes = 0;
        const size_t want = tmp + tmp / 4 + 256;
        if (hipMalloc(&R.q_tmp.p, want) != hipSuccess) return e->fail(KWOK_ENOMEM, "%s: scan storage", who);
        R.tmp_bytes = want;
    }
    RefQuery Q{};
    Q.handles = handles;
    Q.first = (uint32_t)first, Q.n = (uint32_t)n;
    Q.pods = pods ? 1u : 0u, Q.any_slot = any_slot ? 1u : 0u;
    Q.len = R.q_len, Q.off = R.q_off, Q.refs = R.q_refs;
    // KWOK_INGEST_PROF: device-side stamps around k_refs_size, the scan and k_refs_gather
    const auto t0 = clk::now();
    ProfEvents<5> pev(e->iprof, e->st);
    pev.stamp(0);
    const bool nd = !pods && e->ndir.on;  // node queries with the node uid directory on: the uid behind the name
    if (nd) launch_refs_size_nd(e->S, e->ref_dir(), e->ndir.dir(), Q, R.q_slot, st);
    else launch_refs_size(e->S, e->ref_dir(), Q, R.q_slot, st);
    pev.stamp(1);
    HIPCHK(e, hipGetLastError());
    if (launch_refs_scan(Q, R.q_tmp, R.tmp_bytes, st)) return e->fail(KWOK_EDEVICE, "%s: scan", who);
    pev.stamp(2);
    uint64_t tail[2] = {0, 0};  // the last item's offset and size: the total
    HIPCHK(e, hipMemcpyAsync(&tail[0], R.q_off + (n - 1), 8, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(&tail[1], R.q_len + (n - 1), 8, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    const uint64_t total = tail[0] + tail[1];
    if (blob_used) *blob_used = (size_t)total;
    if (total > blob_cap || (total && !blob))
        return e->fail(KWOK_EINVAL, "%s: blob_cap %zu < %llu", who, blob_cap, (unsigned long long)total);
    if ((rc = R.blob.reserve(e, total))) return rc;
    Q.blob = R.q_blob;
    pev.stamp(3);
    if (nd) launch_refs_gather_nd(e->S, e->ndir.dir(), Q, R.q_slot, st);
    else launch_refs_gather(e->S, e->ref_dir(), Q, R.q_slot, st);
    pev.stamp(4);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(refs, R.q_refs, n * sizeof(kwok_ref), hipMemcpyDeviceToHost, st));
    if (total) HIPCHK(e, hipMemcpyAsync(blob, R.q_blob, total, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    if (pev.on()) {
        const float ms_size = pev.elapsed(0, 1), ms_scan = pev.elapsed(1, 2), ms_gather = pev.elapsed(3, 4);
        fprintf(stderr, "[kwok refs] %s: %zu %s, %llu blob bytes: k_refs_size %.3f ms, scan %.3f ms, k_refs_gather %.3f ms; "
                        "the call %.2f ms\n", who, n, pods ? "pods" : "nodes", (unsigned long long)total, ms_size, ms_scan, ms_gather,
                ms_between(t0, clk::now()));
    }
    return KWOK_OK;
}
}  // namespace

int kwok_refs_enable(kwok_engine* e) {
    if (!e) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    if (e->multi) return e->fail(KWOK_EINVAL, "kwok_refs_enable: single-rank engines only");
    auto& R = e->refs;
    if (R.on) return KWOK_OK;
    int rc = kwok_uid_dir_enable(e);  // (drains; the references ride on its run cuts)
    if (rc) return rc;
    if (!R.ctr) {
        if ((rc = dalloc(e, &R.ctr, 1))) return rc;
        if (hipHostMalloc((void**)&R.ctr_h.p, sizeof(RefCounters), hipHostMallocDefault) != hipSuccess)
            return e->fail(KWOK_ENOMEM, "reference directory staging");
        memset(R.ctr_h, 0, sizeof(RefCounters));
    }
    // (dalloc zeroes: no pod has a name)
    if (!R.pod_ref && (rc = dalloc(e, &R.pod_ref, e->PLa))) return rc;
    if (!R.pod_ref_len && (rc = dalloc(e, &R.pod_ref_len, e->PLa))) return rc;
    HIPCHK(e, hipStreamSynchronize(e->st));
    R.on = true;
    return KWOK_OK;
}

int kwok_refs_bind(kwok_engine* e, const int32_t* handles, const char* arena, const uint64_t* ns_off,
                   const uint32_t* ns_len, const uint64_t* name_off, const uint32_t* name_len, size_t n, size_t* n_bad) {
    if (n_bad) *n_bad = 0;
    if (!e || (n && (!handles || !ns_off || !ns_len || !name_off || !name_len)) || n > 0x0FFFFFF0ull) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    auto& R = e->refs;
    if (!R.on) return e->fail(KWOK_EINVAL, "kwok_refs_bind: the reference directory is not enabled");
    drain(e);  // (a handle is judged against the state after every submitted tick)
    if (e->poisoned) return poisoned(e);
    if (!n) return KWOK_OK;
    R.gen[KWOK_KIND_PODS]++;
    uint64_t al = 0;  // (the bytes the valid spans name; a span past 2^40 is the caller's error)
    for (size_t i = 0; i < n; i++) {
        if (!name_len[i] || name_len[i] > KWOK_REF_NAME_MAX || ns_len[i] > KWOK_REF_NS_MAX) continue;
        if (name_off[i] < (1ull << 40)) al = std::max<uint64_t>(al, name_off[i] + name_len[i]);
        if (ns_len[i] && ns_off[i] < (1ull << 40)) al = std::max<uint64_t>(al, ns_off[i] + ns_len[i]);
    }
    if (al && !arena) return KWOK_EINVAL;
    int rc = 0;
    if ((rc = R.spans.reserve(e, n)) || (rc = R.arena.reserve(e, al + 1, grown(al) + 1))) return rc;
    hipStream_t st = e->st;
    HIPCHK(e, hipMemcpyAsync(R.q_h, handles, n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(R.b_off, ns_off, n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(R.b_off + n, name_off, n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(R.b_len, ns_len, n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(R.b_len + n, name_len, n * 4, hipMemcpyHostToDevice, st));
    if (al) HIPCHK(e, hipMemcpyAsync(R.b_arena, arena, al, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemsetAsync(&R.ctr->bad, 0, sizeof(R.ctr->bad), st));
    launch_refs_bind(e->S, e->ref_dir(), R.q_h, R.b_arena, al, R.b_off, R.b_len, R.b_off + n, R.b_len + n, (uint32_t)n, st);
    HIPCHK(e, hipGetLastError());
    if ((rc = refs_read_counters(e))) return rc;
    if (n_bad) *n_bad = (size_t)R.ctr_h->bad;
    return KWOK_OK;
}

int kwok_refs_lookup(kwok_engine* e, int kind, const int32_t* handles, size_t n, uint32_t flags, kwok_ref* refs,
                     char* blob, size_t blob_cap, size_t* blob_used) {
    if (blob_used) *blob_used = 0;
    if (!e || (n && (!handles || !refs)) || n > 0x0FFFFFF0ull) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    auto& R = e->refs;
    if (!R.on) return e->fail(KWOK_EINVAL, "kwok_refs_lookup: the reference directory is not enabled");
    if (kind != KWOK_KIND_PODS && kind != KWOK_KIND_NODES) return e->fail(KWOK_EINVAL, "kwok_refs_lookup: kind %d", kind);
    if (flags & ~(uint32_t)KWOK_REFS_ANY_SLOT) return e->fail(KWOK_EINVAL, "kwok_refs_lookup: flags %u", flags);
    drain(e);
    if (e->poisoned) return poisoned(e);
    if (!n) return KWOK_OK;
    if (int rc = R.spans.reserve(e, n)) return rc;  // (q_h is sized with the bind's buffers)
    HIPCHK(e, hipMemcpyAsync(R.q_h, handles, n * 4, hipMemcpyHostToDevice, e->st));
    return refs_query(e, "kwok_refs_lookup", R.q_h, 0, n, kind == KWOK_KIND_PODS, (flags & KWOK_REFS_ANY_SLOT) != 0, refs, blob,
                      blob_cap, blob_used);
}

int kwok_read_refs(kwok_engine* e, int which, size_t first, size_t count, kwok_ref* refs, char* blob, size_t blob_cap,
                   size_t* blob_used) {
    if (blob_used) *blob_used = 0;
    if (!e || (count && !refs)) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    auto& R = e->refs;
    if (!R.on) return e->fail(KWOK_EINVAL, "kwok_read_refs: the reference directory is not enabled");
    if (which < 0 || which >= KWOK_REFS_LIST_COUNT) return e->fail(KWOK_EINVAL, "kwok_read_refs: list %d", which);
    if (e->cur < 0) return e->fail(KWOK_EINVAL, "no collected tick (or its slot was reused by a submit)");
    const kwok_engine::TickSlot& T = e->slots[e->cur];
    const TickHdr& H = *T.hdr_h;
    const int kind = which == KWOK_REFS_HEARTBEAT || which == KWOK_REFS_NODE_INIT ? KWOK_KIND_NODES : KWOK_KIND_PODS;
    // the stale guard: an ingest since the tick's submit may have created into a slot the list names
    if (R.gen[kind] != T.ref_gen[kind])
        return e->fail(KWOK_EINVAL, "kwok_read_refs: stale: %s were ingested or bound since the collected tick's submit",
                       kind == KWOK_KIND_PODS ? "pods" : "nodes");
    const int32_t* list = which == KWOK_REFS_HEARTBEAT ? T.hb_nodes : which == KWOK_REFS_NODE_INIT ? T.init_nodes :
                          which == KWOK_REFS_POD_PATCH ? T.pp_pods : T.del_pods;
    const size_t total = which == KWOK_REFS_HEARTBEAT ? H.n_hb : which == KWOK_REFS_NODE_INIT ? H.n_init :
                         which == KWOK_REFS_POD_PATCH ? H.n_pp : H.n_del;
    if (first > total || count > total - first)
        return e->fail(KWOK_EINVAL, "kwok_read_refs: range [%zu, +%zu) outside the list's %zu items", first, count, total);
    // (the tick named these objects; it, or a tick queued behind it, may have freed them since: their bytes stay)
    return refs_query(e, "kwok_read_refs", list, first, count, kind == KWOK_KIND_PODS, true, refs, blob, blob_cap, blob_used);
}

int kwok_refs_stats(kwok_engine* e, uint64_t out[KWOK_REFS_STAT_COUNT]) {
    if (!e || !out) return KWOK_EINVAL;
    auto& R = e->refs;
    for (int k = 0; k < KWOK_REFS_STAT_COUNT; k++) out[k] = 0;
    if (!R.ctr) return KWOK_OK;
    if (!e->poisoned)
        if (int rc = refs_read_counters(e)) return rc;
    out[KWOK_REFS_STAT_BINDS] = R.ctr_h->binds;
    out[KWOK_REFS_STAT_NOTES] = R.ctr_h->notes;
    out[KWOK_REFS_STAT_UNNAMED] = R.ctr_h->unnamed;
    out[KWOK_REFS_STAT_READS] = R.ctr_h->reads;
    out[KWOK_REFS_STAT_NOT_FOUND] = R.ctr_h->not_found;
    out[KWOK_REFS_STAT_BYTES] = (uint64_t)e->PLa * (KWOK_REF_STRIDE + sizeof(uint16_t)) + sizeof(RefCounters) +
                                (uint64_t)R.items.cap * (8 + 8 + 4 + sizeof(kwok_ref)) + R.tmp_bytes + R.blob.cap +
                                (uint64_t)R.spans.cap * (2 * 8 + 2 * 4 + 4) + R.arena.cap;
    return KWOK_OK;
}

// ---- the node uid directory (kwok_watch.h, nodes.hip) ----------------------------------
namespace {
int ndir_read_counters(kwok_engine* e) {
    auto& D = e->ndir;
    HIPCHK(e, hipMemcpyAsync(D.ctr_h, D.ctr, sizeof(NodeDirCounters), hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    return KWOK_OK;
}
// kwok_node_lookup / kwok_node_bind: the spans whose length is 1..max_len and the caller's bytes they name, on the device
int ndir_upload(kwok_engine* e, const int32_t* handles, const char* arena, const uint64_t* off, const uint32_t* len, size_t n,
                uint32_t max_len, uint64_t* arena_len) {
    auto& D = e->ndir;
    uint64_t al = 0;
    for (size_t i = 0; i < n; i++)  // (a span past 2^40 is the caller's error: it names no byte here and answers as a miss)
        if (len[i] && len[i] <= max_len && off[i] < (1ull << 40)) al = std::max<uint64_t>(al, off[i] + len[i]);
    if (al && !arena) return KWOK_EINVAL;
    int rc = 0;
    if ((rc = D.spans.reserve(e, n)) || (rc = D.arena.reserve(e, al + 1, grown(al) + 1))) return rc;
    hipStream_t st = e->st;
    if (handles) HIPCHK(e, hipMemcpyAsync(D.q_h, handles, n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(D.q_off, off, n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(D.q_len, len, n * 4, hipMemcpyHostToDevice, st));
    if (al) HIPCHK(e, hipMemcpyAsync(D.q_arena, arena, al, hipMemcpyHostToDevice, st));
    *arena_len = al;
    return KWOK_OK;
}
}  // namespace

int kwok_node_dir_enable(kwok_engine* e) {
    if (!e) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    if (e->multi) return e->fail(KWOK_EINVAL, "kwok_node_dir_enable: single-rank engines only");
    auto& D = e->ndir;
    if (D.on) return KWOK_OK;
    drain(e);
    if (e->poisoned) return poisoned(e);
    int rc = 0;  // (dalloc zeroes: no node has a uid)
    // (each piece on its own: a call that failed half way is finished by the next one)
    if (!D.ctr && (rc = dalloc(e, &D.ctr, 1))) return rc;
    if (!D.call && (rc = dalloc(e, &D.call, 1))) return rc;
    if (!D.ctr_h) {
        if (hipHostMalloc((void**)&D.ctr_h.p, sizeof(NodeDirCounters), hipHostMallocDefault) != hipSuccess)
            return e->fail(KWOK_ENOMEM, "node directory staging");
        memset(D.ctr_h, 0, sizeof(NodeDirCounters));
    }
    if (!D.call_h) {
        if (hipHostMalloc((void**)&D.call_h.p, sizeof(*D.call_h.p), hipHostMallocDefault) != hipSuccess)
            return e->fail(KWOK_ENOMEM, "node directory staging");
        memset(D.call_h, 0, sizeof(*D.call_h.p));
    }
    if (!D.node_uid && (rc = dalloc(e, &D.node_uid, e->NL))) return rc;
    if (!D.node_uid_key && (rc = dalloc(e, &D.node_uid_key, e->NL))) return rc;
    if (!D.node_uid_len && (rc = dalloc(e, &D.node_uid_len, (size_t)e->NL + 4))) return rc;
    HIPCHK(e, hipStreamSynchronize(e->st));
    D.on = true;
    return KWOK_OK;
}

int kwok_node_lookup(kwok_engine* e, const char* arena, const uint64_t* off, const uint32_t* len, size_t n,
                     int32_t* out_handles) {
    if (!e || (n && (!off || !len || !out_handles)) || n > 0x07FFFFF0ull) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    drain(e);  // (a name is judged against the state after every submitted tick)
    if (e->poisoned) return poisoned(e);
    if (!n) return KWOK_OK;
    auto& D = e->ndir;
    uint64_t al = 0;
    int rc = ndir_upload(e, nullptr, arena, off, len, n, NODE_NAME_MAX, &al);
    if (rc) return rc;
    hipStream_t st = e->st;
    launch_nd_lookup(e->S, D.on ? D.ctr.p : nullptr, D.q_arena, al, D.q_off, D.q_len, (uint32_t)n, D.q_h, st);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(out_handles, D.q_h, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    return KWOK_OK;
}

int kwok_node_bind(kwok_engine* e, const int32_t* handles, const char* arena, const uint64_t* off, const uint32_t* len,
                   size_t n, size_t* n_bad) {
    if (n_bad) *n_bad = 0;
    if (!e || (n && (!handles || !off || !len)) || n > 0x0FFFFFF0ull) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    auto& D = e->ndir;
    if (!D.on) return e->fail(KWOK_EINVAL, "kwok_node_bind: the node directory is not enabled");
    drain(e);  // (a handle is judged against the state after every submitted tick)
    if (e->poisoned) return poisoned(e);
    if (!n) return KWOK_OK;
    uint64_t al = 0;
    int rc = ndir_upload(e, handles, arena, off, len, n, KWOK_UID_MAX, &al);
    if (rc) return rc;
    if (e->refs.on) e->refs.gen[KWOK_KIND_NODES]++;  // (kwok_read_refs' stale guard: a node's answer changes)
    hipStream_t st = e->st;
    HIPCHK(e, hipMemsetAsync(&D.ctr->bad, 0, sizeof(D.ctr->bad), st));
    launch_nd_uid_bind(e->S, D.dir(), D.q_h, D.q_arena, al, D.q_off, D.q_len, (uint32_t)n, st);
    HIPCHK(e, hipGetLastError());
    if ((rc = ndir_read_counters(e))) return rc;
    if (n_bad) *n_bad = (size_t)D.ctr_h->bad;
    return KWOK_OK;
}

int kwok_node_dir_stats(kwok_engine* e, uint64_t out[KWOK_NODE_DIR_STAT_COUNT]) {
    if (!e || !out) return KWOK_EINVAL;
    auto& D = e->ndir;
    for (int k = 0; k < KWOK_NODE_DIR_STAT_COUNT; k++) out[k] = 0;
    if (!D.on) return KWOK_OK;
    if (!e->poisoned)
        if (int rc = ndir_read_counters(e)) return rc;
    out[KWOK_NODE_DIR_STAT_LOOKUPS] = D.ctr_h->lookups;
    out[KWOK_NODE_DIR_STAT_HITS] = D.ctr_h->hits;
    out[KWOK_NODE_DIR_STAT_NOTES] = D.ctr_h->notes;
    out[KWOK_NODE_DIR_STAT_BINDS] = D.ctr_h->binds;
    out[KWOK_NODE_DIR_STAT_UNBOUND] = D.ctr_h->unbound;
    out[KWOK_NODE_DIR_STAT_BYTES] = (uint64_t)e->NL * (KWOK_UID_MAX + 1 + 8) + 4 + sizeof(NodeDirCounters) + sizeof(*D.call_h.p) +
                                    (uint64_t)D.spans.cap * (4 + 8 + 4) + D.arena.cap + (uint64_t)D.recs.cap * (4 + 4 + 1 + 4);
    return KWOK_OK;
}

int kwok_pack_pod_events(const kwok_pod_event* ev, size_t n, const char* arena, size_t arena_len, kwok_pod_rec* out,
                         int32_t* status) {
    if ((n && (!ev || !out)) || (arena_len && !arena)) return KWOK_EINVAL;
    int bad = 0;
    auto ip_of = [&](kwok_str s, uint32_t* ip) {  // "" -> 0; otherwise a canonical, non-zero dotted quad
        *ip = 0;
        if (!s.len) return true;
        if ((uint64_t)s.off + s.len > arena_len) return false;
        return parse_ipv4(arena + s.off, s.len, ip) && *ip != 0;
    };
    for (size_t i = 0; i < n; i++) {
        const kwok_pod_event& x = ev[i];
        kwok_pod_rec r{};
        int st = KWOK_OK;
        const bool create = x.op == KWOK_OP_UPSERT && x.handle < 0;
        r.op = (uint8_t)(x.op | (create ? KWOK_REC_NEW : 0u));
        r.flags = (uint8_t)((x.flags & 31u) | ((x.phase & 7u) << KWOK_REC_PHASE_SHIFT));
        r.spec_id = x.op == KWOK_OP_UPSERT ? (uint16_t)x.spec_id : (uint16_t)0;
        r.target = create ? x.node_handle : x.handle;
        if (x.op != KWOK_OP_UPSERT && x.op != KWOK_OP_DELETE) st = KWOK_EINVAL;
        else if (create && x.node_handle < 0) st = KWOK_EINVAL;  // by spec.nodeName: the full form only
        else if (x.phase > KWOK_PHASE_UNKNOWN) st = KWOK_EINVAL;  // (a pod phase: the device prep's bound)
        else if (x.op == KWOK_OP_UPSERT && (x.spec_id < 0 || x.spec_id > 0xFFFF)) st = KWOK_EINVAL;
        else if (x.op == KWOK_OP_UPSERT && (x.creation_unix < 0 || x.creation_unix > 0xFFFFFFFFll)) st = KWOK_EDOMAIN;
        else if (x.op == KWOK_OP_UPSERT && (!ip_of(x.host_ip, &r.host_ip) || !ip_of(x.pod_ip, &r.pod_ip)))
            st = KWOK_EDOMAIN;
        else if (x.op == KWOK_OP_DELETE && !ip_of(x.pod_ip, &r.pod_ip)) r.pod_ip = 0;  // not released (as unparsed)
        r.creation = x.op == KWOK_OP_UPSERT && st == KWOK_OK ? (uint32_t)x.creation_unix : 0u;
        if (status) status[i] = st;
        if (st == KWOK_OK) out[i] = r;
        bad += st != KWOK_OK;
    }
    return bad;
}

int kwok_cni_pending(kwok_engine* e, int32_t* out, size_t cap, size_t* n_out) {
    if (!e || !n_out || (cap && !out)) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    if (!e->S.cni) return e->fail(KWOK_EINVAL, "kwok_cni_pending: the engine was created without enable_cni");
    drain(e);
    if (e->poisoned) return poisoned(e);
    // scratch: the exchange list buffer (multi-rank ticks only, none in flight) and its counter
    HIPCHK(e, hipMemsetAsync(e->S.list_counts, 0, 4, e->st));
    launch_cni_pending(e->S, (int32_t*)e->S.use_list, e->S.list_counts, e->st);
    HIPCHK(e, hipGetLastError());
    uint32_t cnt = 0;
    if (int rc = release_for_host(e)) return rc;
    HIPCHK(e, hipMemcpyAsync(&cnt, e->S.list_counts, 4, hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    std::vector<int32_t> h(cnt);
    if (cnt) {
        HIPCHK(e, hipMemcpyAsync(h.data(), e->S.use_list, (size_t)cnt * 4, hipMemcpyDeviceToHost, e->st));
        HIPCHK(e, hipStreamSynchronize(e->st));
    }
    (void)hipMemsetAsync(e->S.list_counts, 0, 8, e->st);
    std::sort(h.begin(), h.end());  // canonical order
    *n_out = cnt;
    if (cap < cnt) return e->fail(KWOK_EINVAL, "kwok_cni_pending: %u pods pending, buffer holds %zu", cnt, cap);
    if (cnt) memcpy(out, h.data(), (size_t)cnt * 4);
    return KWOK_OK;
}

int kwok_cni_assign(kwok_engine* e, const int32_t* handles, const uint32_t* ips, size_t n, int32_t* out_status) {
    if (!e || (n && (!handles || !ips)) || n > 0x7FFFFFF0ull) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    if (!e->S.cni) return e->fail(KWOK_EINVAL, "kwok_cni_assign: the engine was created without enable_cni");
    drain(e);
    if (e->poisoned) return poisoned(e);
    if (!n) return 0;
    e->quiet = 0;
    e->state_changed();
    // a handle assigned twice keeps its last valid IP (configurePod runs once per tick)
    std::vector<uint8_t> wr(n, 0);
    {
        std::unordered_map<int32_t, size_t> last;
        for (size_t i = 0; i < n; i++)
            if (ips[i]) last[handles[i]] = i;
        for (const auto& kv : last) wr[kv.second] = 1;
    }
    int rc = ingest_reserve(e, n, 0);
    if (rc) return rc;
    auto& G = e->ing;
    hipStream_t st = e->st;
    // scratch: the ingest buffers (handles, IPs, write flags, statuses)
    HIPCHK(e, hipMemsetAsync(G.sum, 0, sizeof(IngSummary), st));
    HIPCHK(e, hipMemcpyAsync(G.keys, handles, n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(G.keys_sorted, ips, n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(G.idx_sorted, wr.data(), n, hipMemcpyHostToDevice, st));
    launch_cni_assign(e->S, (const int32_t*)G.keys.p, G.keys_sorted, (const uint8_t*)G.idx_sorted.p, (uint32_t)n,
                      G.out_status, &G.sum->rejected, st);
    HIPCHK(e, hipGetLastError());
    if ((rc = read_summary(e))) return rc;
    if (out_status) {
        HIPCHK(e, hipMemcpyAsync(out_status, G.out_status, n * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(e, hipStreamSynchronize(st));
    }
    return (int)G.sum_h->rejected;
}

int kwok_pool_put(kwok_engine* e, const uint32_t* ips, size_t n) {
    if (!e || (n && !ips)) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    drain(e);  // the host mirrors reflect every submitted tick
    if (e->poisoned) return poisoned(e);
    e->puts.insert(e->puts.end(), ips, ips + n);
    e->quiet = 0;
    e->state_changed();
    e->foreign_ips = true;  // releases of another rank's pods (multi rank)
    return flush_ops(e);
}

int kwok_read_outputs(kwok_engine* e, kwok_outputs* o) {
    if (!e || !o) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    if (e->cur < 0) return e->fail(KWOK_EINVAL, "no collected tick (or its slot was reused by a submit)");
    const kwok_engine::TickSlot& S = e->slots[e->cur];  // outputs of the last collected tick
    const TickHdr& H = *S.hdr_h;
    // the copies run on their own stream once the tick is done, so they overlap a
    // tick already queued behind it (kwok_tick_submit before kwok_read_outputs);
    // the fence event there writes the kernels' L2 lines back for the copy engine
    hipStream_t st = e->rst;
    HIPCHK(e, hipStreamWaitEvent(st, S.done, 0));
    HIPCHK(e, hipEventRecord(e->fence, st));
    auto cp = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
        if (!dst || !bytes) return hipSuccess;
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
    };
    o->heartbeat_off = H.hb_base;
    HIPCHK(e, cp(o->heartbeat_nodes, S.hb_nodes, (size_t)H.n_hb * 4));
    HIPCHK(e, cp(o->node_init_nodes, S.init_nodes, (size_t)H.n_init * 4));
    HIPCHK(e, cp(o->node_init_off, S.init_off, (size_t)H.n_init * 8));
    HIPCHK(e, cp(o->node_init_len, S.init_len, (size_t)H.n_init * 4));
    HIPCHK(e, cp(o->pod_patch_pods, S.pp_pods, (size_t)H.n_pp * 4));
    HIPCHK(e, cp(o->pod_patch_off, S.pp_off, (size_t)H.n_pp * 8));
    HIPCHK(e, cp(o->pod_patch_len, S.pp_len, (size_t)H.n_pp * 4));
    HIPCHK(e, cp(o->delete_pods, S.del_pods, (size_t)H.n_del * 4));
    HIPCHK(e, cp(o->delete_has_finalizers, S.del_fin, (size_t)H.n_del));
    o->arena_shift = 0;
    o->arena_copied = 0;
    if (o->arena) {
        if (o->flags & KWOK_READ_HEARTBEAT_ONCE) {
            // one heartbeat body, then the node-init / pod patch region (init_base..)
            const uint64_t hb = H.n_hb ? (uint64_t)e->hb_stride : 0, patches = H.arena_bytes - H.init_base;
            if (o->arena_cap < hb + patches)
                return e->fail(KWOK_EINVAL, "arena_cap < %llu", (unsigned long long)(hb + patches));
            HIPCHK(e, cp(o->arena, S.arena, hb));
            HIPCHK(e, cp(o->arena + hb, S.arena + H.init_base, patches));
            o->arena_shift = H.init_base - hb;
            o->arena_copied = hb + patches;
        } else {
            if (o->arena_cap < H.arena_bytes)
                return e->fail(KWOK_EINVAL, "arena_cap < %llu", (unsigned long long)H.arena_bytes);
            HIPCHK(e, cp(o->arena, S.arena, H.arena_bytes));
            o->arena_copied = H.arena_bytes;
        }
    }
    HIPCHK(e, hipStreamSynchronize(st));
    return KWOK_OK;
}

// Page-locked batch buffers: 2 MiB-aligned anonymous memory on transparent huge
// pages where the kernel grants them, registered (and mapped) with the runtime
// (the GPU walks 512x fewer page translations than over 4 KiB pages);
// KWOK_HOST_ALLOC=hip: hipHostMalloc instead.  Both are in the registry, with
// their device addresses: kwok_ingest_pods reads a batch in such a buffer in
// place (host_mapped).
void* kwok_host_alloc(size_t bytes) {
    bytes = bytes ? bytes : 1;
    const char* how = getenv("KWOK_HOST_ALLOC");
    if (!(how && strcmp(how, "hip") == 0)) {
        const size_t huge = (size_t)2 << 20, len = (bytes + huge - 1) & ~(huge - 1);
        void* p = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p != MAP_FAILED) {
            const char* thp = getenv("KWOK_HOST_THP");
            if (!(thp && thp[0] == '0')) (void)madvise(p, len, MADV_HUGEPAGE);
            memset(p, 0, len);  // first touch: the pages exist (huge where granted) before pinning
            if (hipHostRegister(p, len, hipHostRegisterMapped) == hipSuccess) {
                void* dev = nullptr;
                if (hipHostGetDevicePointer(&dev, p, 0) != hipSuccess) dev = nullptr;
                std::lock_guard<std::mutex> l(g_host_mu);
                g_host_reg[(uintptr_t)p] = HostReg{len, (uint8_t*)dev, true};
                return p;
            }
            munmap(p, len);
        }
    }
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    void* dev = nullptr;
    if (hipHostGetDevicePointer(&dev, p, 0) != hipSuccess) dev = nullptr;
    std::lock_guard<std::mutex> l(g_host_mu);
    g_host_reg[(uintptr_t)p] = HostReg{bytes, (uint8_t*)dev, false};
    return p;
}

void kwok_host_free(void* p) {
    if (!p) return;
    HostReg r{0, nullptr, false};
    bool found = false;
    {
        std::lock_guard<std::mutex> l(g_host_mu);
        auto it = g_host_reg.find((uintptr_t)p);
        if (it != g_host_reg.end()) r = it->second, found = true, g_host_reg.erase(it);
    }
    if (found && r.mmapped) {
        (void)hipHostUnregister(p);
        munmap(p, r.len);
    } else {
        (void)hipHostFree(p);
    }
}

// dst <- src (len bytes) on the read stream (after its fence), a large read in
// parts over the extra read streams, joined back on the read stream
int read_copy(kwok_engine* e, void* dst, const uint8_t* src, uint64_t len) {
    const int ns = len >= (16ull << 20) ? std::max(1, std::min(e->read_streams, 4)) : 1;
    if (ns > 1) {
        if (!e->rd_go) HIPCHK(e, hipEventCreateWithFlags(&e->rd_go, hipEventDisableTiming));
        for (int i = 0; i < ns - 1; i++) {
            if (!e->rsx[i]) HIPCHK(e, hipStreamCreateWithFlags(&e->rsx[i], hipStreamNonBlocking));
            if (!e->rd_part[i]) HIPCHK(e, hipEventCreateWithFlags(&e->rd_part[i], hipEventDisableTiming));
        }
        HIPCHK(e, hipEventRecord(e->rd_go, e->rst));
    }
    const uint64_t step = ((len + ns - 1) / ns + 4095) & ~4095ull;
    for (int i = ns - 1; i >= 0; i--) {
        const uint64_t lo = std::min<uint64_t>(len, step * i), hi = std::min<uint64_t>(len, step * (i + 1));
        if (hi <= lo) continue;
        hipStream_t s = i ? e->rsx[i - 1] : e->rst;
        if (i) HIPCHK(e, hipStreamWaitEvent(s, e->rd_go, 0));
        HIPCHK(e, hipMemcpyAsync(static_cast<uint8_t*>(dst) + lo, src + lo, hi - lo, hipMemcpyDeviceToHost, s));
        if (i) {
            HIPCHK(e, hipEventRecord(e->rd_part[i - 1], s));
            HIPCHK(e, hipStreamWaitEvent(e->rst, e->rd_part[i - 1], 0));
        }
    }
    return KWOK_OK;
}

int kwok_read_arena(kwok_engine* e, uint64_t off, uint64_t len, void* dst) {
    if (!e || (len && !dst)) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    if (e->cur < 0) return e->fail(KWOK_EINVAL, "no collected tick (or its slot was reused by a submit)");
    const kwok_engine::TickSlot& S = e->slots[e->cur];
    const uint64_t total = S.hdr_h->arena_bytes;
    if (off > total || len > total - off)
        return e->fail(KWOK_EINVAL, "arena range [%llu, +%llu) outside the tick's %llu bytes", (unsigned long long)off,
                       (unsigned long long)len, (unsigned long long)total);
    if (!len) return KWOK_OK;
    hipStream_t st = e->rst;  // beside a tick queued behind the collected one (as kwok_read_outputs)
    HIPCHK(e, hipStreamWaitEvent(st, S.done, 0));
    HIPCHK(e, hipEventRecord(e->fence, st));
    if (int rc = read_copy(e, dst, S.arena + off, len)) return rc;
    HIPCHK(e, hipStreamSynchronize(st));
    return KWOK_OK;
}

// kwok_read_arena queued without waiting: dst should be kwok_host_alloc memory (the
// copy engine writes it while the caller goes on: the next batch's ingest, the
// next tick); kwok_read_wait waits for every read queued so far.  The slot stays
// the caller's until the next submit that takes it, which waits for the reads on
// the device (or, when the arena must grow, on the host)
int kwok_read_arena_async(kwok_engine* e, uint64_t off, uint64_t len, void* dst) {
    if (!e || (len && !dst)) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    if (e->cur < 0) return e->fail(KWOK_EINVAL, "no collected tick (or its slot was reused by a submit)");
    kwok_engine::TickSlot& S = e->slots[e->cur];
    const uint64_t total = S.hdr_h->arena_bytes;
    if (off > total || len > total - off)
        return e->fail(KWOK_EINVAL, "arena range [%llu, +%llu) outside the tick's %llu bytes", (unsigned long long)off,
                       (unsigned long long)len, (unsigned long long)total);
    if (!len) return KWOK_OK;
    hipStream_t st = e->rst;
    if (!S.rd && hipEventCreateWithFlags(&S.rd, hipEventDisableTiming) != hipSuccess)
        return e->fail(KWOK_EDEVICE, "event create");
    HIPCHK(e, hipStreamWaitEvent(st, S.done, 0));
    HIPCHK(e, hipEventRecord(e->fence, st));
    if (int rc = read_copy(e, dst, S.arena + off, len)) return rc;
    HIPCHK(e, hipEventRecord(S.rd, st));
    S.rd_pending = true;
    return KWOK_OK;
}

int kwok_read_wait(kwok_engine* e) {
    if (!e) return KWOK_EINVAL;
    HIPCHK(e, hipStreamSynchronize(e->rst));
    for (auto& T : e->slots) T.rd_pending = false;
    return KWOK_OK;
}

int kwok_device_outputs(kwok_engine* e, kwok_device_view* v) {
    if (!e || !v) return KWOK_EINVAL;
    if (e->cur < 0) return e->fail(KWOK_EINVAL, "no collected tick (or its slot was reused by a submit)");
    const kwok_engine::TickSlot& T = e->slots[e->cur];
    v->arena = T.arena;
    v->heartbeat_nodes = T.hb_nodes;
    v->pod_patch_pods = T.pp_pods;
    v->pod_patch_off = T.pp_off;
    v->pod_patch_len = T.pp_len;
    v->stream = e->st;
    return KWOK_OK;
}

int kwok_profile_enable(kwok_engine* e, int on) {
    if (!e) return KWOK_EINVAL;
    drain(e);
    for (auto& T : e->slots)
        for (auto& ev : T.pev)
            if (T.alloc && !ev) HIPCHK(e, hipEventCreate(&ev));
    e->prof = on != 0;
    memset(e->prof_ms, 0, sizeof e->prof_ms);
    e->prof_ticks = 0;
    return KWOK_OK;
}

int kwok_profile_read(kwok_engine* e, double ms_sum[KWOK_T_COUNT], uint64_t* ticks) {
    if (!e) return KWOK_EINVAL;
    if (ms_sum) memcpy(ms_sum, e->prof_ms, sizeof e->prof_ms);
    if (ticks) *ticks = e->prof_ticks;
    return KWOK_OK;
}

int kwok_profile_host(kwok_engine* e, int reset, double ms_sum[KWOK_H_COUNT], uint64_t* ticks) {
    if (!e) return KWOK_EINVAL;
    if (ms_sum) memcpy(ms_sum, e->host_ms, sizeof e->host_ms);
    if (ticks) *ticks = e->host_ticks;
    if (reset) {
        memset(e->host_ms, 0, sizeof e->host_ms);
        e->host_ticks = 0;
    }
    return KWOK_OK;
}

int kwok_node_has(kwok_engine* e, const char* name, size_t len) {
    // nodesSets.Has (node_controller.go:140-143): the device directory's entry is managed
    if (!e || !name || !len || len > NODE_NAME_MAX || e->poisoned) return 0;
    if (ensure_pinned(e, NAME_STRIDE + 64)) return 0;
    uint8_t* h = static_cast<uint8_t*>(e->pinned);
    uint8_t* d = static_cast<uint8_t*>(e->d_ops);
    memcpy(h, name, len);
    const uint32_t n32 = (uint32_t)len;
    memcpy(h + NAME_STRIDE, &n32, 4);
    uint32_t res = 0;
    if (hipMemcpyAsync(d, h, NAME_STRIDE + 4, hipMemcpyHostToDevice, e->st) != hipSuccess) return 0;
    launch_node_lookup(e->S, d, reinterpret_cast<const uint32_t*>(d + NAME_STRIDE), 1,
                       reinterpret_cast<uint32_t*>(d + NAME_STRIDE + 16), e->st);
    if (hipGetLastError() != hipSuccess || release_for_host(e) ||
        hipMemcpyAsync(h + NAME_STRIDE + 16, d + NAME_STRIDE + 16, 4, hipMemcpyDeviceToHost, e->st) != hipSuccess ||
        hipStreamSynchronize(e->st) != hipSuccess)
        return 0;
    memcpy(&res, h + NAME_STRIDE + 16, 4);
    return (res & NS_MANAGED) != 0;
}

uint64_t kwok_node_size(kwok_engine* e) { return e ? e->n_managed : 0; }

int kwok_dump_pods(kwok_engine* e, int32_t first, uint32_t count, uint8_t* used, uint8_t* phase, uint32_t* host_ip,
                   uint32_t* pod_ip) {
    if (!e) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    drain(e);
    // through the engine's page-locked dump buffer: a device-to-host copy into
    // pageable memory made later copies of the ingest path stall (measured: every
    // other 2M-record churn batch paid 6-20 ms before its first device operation)
    const size_t PL = e->PL, need = PL * 10;
    if (need > e->dump_cap) {
        if (e->dump_h) (void)hipHostFree(e->dump_h);
        e->dump_h = nullptr;
        e->dump_cap = 0;
        if (hipHostMalloc((void**)&e->dump_h, need, hipHostMallocDefault) != hipSuccess)
            return e->fail(KWOK_ENOMEM, "dump buffer %zu", need);
        e->dump_cap = need;
    }
    uint32_t* hh = reinterpret_cast<uint32_t*>(e->dump_h);
    uint32_t* ph = hh + PL;
    const uint16_t* sth = reinterpret_cast<const uint16_t*>(ph + PL);
    if (int rc = release_for_host(e)) return rc;
    HIPCHK(e, hipMemcpyAsync((void*)sth, e->S.pod_state, PL * 2, hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipMemcpyAsync(hh, e->S.host_ip, PL * 4, hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipMemcpyAsync(ph, e->S.pod_ip, PL * 4, hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    for (uint32_t i = 0; i < count; i++) {
        uint32_t l = 0;
        bool ok = e->pod_slot((int64_t)first + i, &l) == KWOK_OK && (sth[l] & PS_USED);
        if (used) used[i] = ok;
        if (phase) phase[i] = ok ? (uint8_t)((sth[(size_t)l] & PS_PHASE_MASK) >> PS_PHASE_SHIFT) : 0;
        if (host_ip) host_ip[i] = ok && (sth[(size_t)l] & PS_HAS_HOST_IP) ? hh[(size_t)l] : 0;
        if (pod_ip) pod_ip[i] = ok ? ph[(size_t)l] : 0;
    }
    return KWOK_OK;
}

}  // extern "C"
