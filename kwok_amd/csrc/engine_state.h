// engine_state.h - internal to the host runtime: the engine's state (struct kwok_engine with the sub-structs of
// every subsystem), the device allocation helpers, and the helpers one engine*.cpp file defines and another
// calls.  Included by every engine*.cpp and by nothing else; engine_impl.h has the owning scratch types it
// builds on.  Everything here stays out of the dynamic symbol table.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>
#include <string.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/kwok_engine.h"
#include "../../include/kwok_canon.h"
#include "codec.h"
#include "device.h"
#include "gotemplate.h"
#include "kernels.h"
#include "echo.h"
#include "templates.h"
#include "engine_impl.h"

using namespace kwok;

#pragma GCC visibility push(hidden)

namespace kwok {

using clk = std::chrono::steady_clock;
inline double ms_between(clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
};

// Persistent host worker threads for the ingest partitions (started on first
// use): run(n, f) calls f(0) on the caller and f(1..n-1) on the workers, and
// returns when all are done.
class WorkPool {
  public:
    ~WorkPool() {
        {
            std::lock_guard<std::mutex> l(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    void run(int n, const std::function<void(int)>& f) {
        while ((int)th_.size() < n - 1) {
            const int id = (int)th_.size() + 1;
            th_.emplace_back([this, id] { loop(id); });
        }
        {
            std::lock_guard<std::mutex> l(m_);
            job_ = &f;
            width_ = n;
            left_ = n - 1;
            gen_++;
        }
        cv_.notify_all();
        f(0);
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [&] { return left_ == 0; });
        job_ = nullptr;
    }

  private:
    void loop(int id) {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> l(m_);
        for (;;) {
            cv_.wait(l, [&] { return stop_ || gen_ != seen; });
            if (stop_) return;
            seen = gen_;
            if (id >= width_) continue;  // this run uses fewer workers
            const std::function<void(int)>* f = job_;
            l.unlock();
            (*f)(id);
            l.lock();
            if (--left_ == 0) done_.notify_one();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(int)>* job_ = nullptr;
    uint64_t gen_ = 0;
    int width_ = 0, left_ = 0;
    bool stop_ = false;
};

}  // namespace kwok

#pragma GCC visibility pop

struct kwok_engine {
    kwok_config cfg{};
    std::string err;
    int W = 1, rank = 0, dev = 0;
    int XW = 1;  // exchange messages per tick: W, or KWOK_EMULATE_RANKS on a one-rank multi engine (diagnostics)
    bool multi = false;  // the FRONT / exchange / BACK tick (W > 1, or KWOK_FORCE_MULTI with one rank)
    uint32_t B = 0, Cn = 0, Cp = 0, b_lo = 0, b_hi = 0, nb = 0, NL = 0, PL = 0;
    uint32_t Hs = 0;  // pod handle stride: handle = bucket * Hs + slot in the bucket; Cp grows up to it
    PoolGeom pool{};
    uint32_t node_ip = 0;
    std::string node_ip_s;
    int64_t start = 0;
    hipStream_t st = nullptr;   // tick pipeline
    hipEvent_t fence = nullptr; // recorded (system-scope release) before device -> host copies of kernel output
    hipStream_t rst = nullptr;  // kwok_read_outputs: copies of a collected tick, beside the next tick's kernels
    // large arena reads split over more copy streams (KWOK_READ_STREAMS, default 1: two or
    // four streams measured no faster than one, ~44 GB/s device-to-host either way)
    int read_streams = 1;
    hipStream_t rsx[3] = {};
    hipEvent_t rd_go = nullptr, rd_part[3] = {};
    DevState S{};

    // ---- nodes: the directory (names -> slots), occupancy, managed / zombie counts
    // live on the device (ingest.hip); the host keeps the managed-set size ----
    uint64_t n_managed = 0;
    bool hb_pre_dirty = true;                        // the per-chain-block heartbeat bases need k_hb_pre
    uint32_t hb_epoch = 0;                           // kwok_tick_result.heartbeat_epoch: bumped when the managed set changes
    uint32_t* d_hb_pre = nullptr;
    uint32_t* d_hb_bpre = nullptr;                   // [nb + 1] per-bucket bases (k_once)
    // pods: no host mirror.  The device's pod_state (USED = slot occupancy),
    // pod_node and node_state (NS_SLOT) are the state the GPU ingest pass
    // (ingest.hip) applies batches to; pod_fill is its per-bucket fill mark.
    uint16_t* d_pod_fill = nullptr;

    // ---- host work of node batches: the status strings of UPSERT records with a
    // non-empty status (string checks, blob interning, custom node templates), on up
    // to n_part host threads ----
    int n_part = 1;
    std::vector<uint32_t> puts;  // kwok_pool_put (other ranks' ingest-time releases), staged for flush_ops
    void* pinned = nullptr;
    size_t pinned_cap = 0;
    void* d_ops = nullptr;
    size_t d_ops_cap = 0;

    // ---- GPU pod ingest (ingest.hip) ----
    struct KWOK_LOCAL Ingest {
        size_t sort_bytes = 0;
        DevArr<void> d_ev;       // [recs.cap] kwok_pod_event, or the packed forms
        DevArr<uint8_t> d_arena;
        DevArr<PodRec> rec;
        DevArr<uint32_t> keys, keys_sorted, idx_sorted;
        DevArr<int32_t> out_handle, out_status;
        DevArr<int8_t> out_status8;  // kwok_ingest_pods_packed: the statuses as bytes
        DevArr<uint32_t> out_released;
        DevArr<void> sort_tmp;   // [sort_bytes]
        // kwok_ingest_pods_packed12: NEW records per 256-record tile, the tiles' prefixes,
        // the creates' handles in create order
        DevArr<uint32_t> tile_new, tile_pre;
        DevArr<int32_t> new_handle;
        static size_t ev_bytes(size_t cap) { return cap * sizeof(kwok_pod_event); }
        static size_t sort_need(size_t cap) { return ingest_sort_bytes((uint32_t)cap, 32); }
        // the per-record buffers (recs.cap: the records they hold) and the batch's strings
        DevGroup recs{4096, {{d_ev, ev_bytes}, rec, keys, keys_sorted, idx_sorted, out_handle, out_status, out_released,
                             out_status8, {tile_new, per_tile256}, {tile_pre, per_tile256}, new_handle, {sort_tmp, sort_need}}};
        DevGroup arena{1 << 16, {d_arena}};
        // per bucket (allocated once)
        uint32_t *beg = nullptr, *end = nullptr;
        uint32_t* abort = nullptr;          // [1] a chunk of the batch needs growth (speculative apply passes)
        IngSummary* sums = nullptr;         // [nsums] one per chunk of a batch
        IngSummary* sums_h = nullptr;       // pinned
        size_t nsums = 0;
        IngSummary* sum = nullptr;
        // node batches (kwok_ingest_nodes): records, names, prepared records, host list
        DevArr<kwok_node_event> d_nev;
        DevArr<uint8_t> d_nnames;  // [nodes.cap * NAME_STRIDE]
        DevArr<NodeRec> nrec;
        DevArr<uint32_t> host_idx;
        DevArr<NodeFix> d_nfix;
        static size_t name_bytes(size_t cap) { return cap * NAME_STRIDE; }
        DevGroup nodes{4096, {d_nev, {d_nnames, name_bytes}, nrec, host_idx, d_nfix}};
        NodeSummary* nsum = nullptr;
        NodeSummary* nsum_h = nullptr;  // pinned
        Pinned<int32_t> res_h;          // [2 * nodes.cap]: handles, statuses
        IngSummary* sum_h = nullptr;  // pinned
        // a batch runs in chunks (KWOK_INGEST_CHUNK records): chunk k+1's prep reads its
        // records over the link on `pst` while chunk k is applied and its results copied
        // back on the engine stream
        IngSummary* sum1 = nullptr;
        hipStream_t pst = nullptr, dst = nullptr;  // prep (H2D + k_ing_prep) / results (D2H)
        hipEvent_t tev[8] = {};  // KWOK_INGEST_PROF: device-side phase stamps of a two-chunk batch
        hipEvent_t go = nullptr, prepped[2] = {nullptr, nullptr}, used[2] = {nullptr, nullptr};
        hipEvent_t idone = nullptr;  // a pod batch's last operation (the host spins on it: KWOK_SYNC)
        hipEvent_t rdone = nullptr;  // the results stream's work of a batch (kwok_pod_rec12: before the summaries)
        size_t chunk = 1048576;
        // the framed ingests (kwok_watch.h): the records' strings are in the resident watch
        // stream, not in d_arena (null: d_arena)
        const uint8_t* arena_src = nullptr;
    } ing;

    // ---- the watch stream framer (json.hip k_frame_*): the resident stream, its
    // frames on the device and on the host, the caller's bytes (listed lines and
    // documents are completed from them) ----
    struct KWOK_LOCAL Watch {
        DevArr<uint8_t> stream;        // [bytes.cap] the stream, padded to whole 16-byte windows
        DevGroup bytes{1 << 16, {stream}};
        uint64_t len = 0;
        const char* host = nullptr;    // the caller's buffer (valid until the next framing call)
        DevArr<uint32_t> tile_cnt, tile_base;
        DevGroup tiles{1024, {tile_cnt, tile_base}};
        DevArr<uint32_t> ends;         // [lines.cap] newline offsets
        DevArr<kwok_watch_frame> frames;  // [lines.cap]
        DevArr<uint32_t> host_list;    // [lines.cap]
        DevGroup lines{4096, {ends, frames, host_list}};
        DevArr<uint32_t> counts;       // [2]: newlines, listed lines
        Pinned<uint32_t> counts_h;     // [2]
        std::vector<kwok_watch_frame> frames_h;
        uint64_t id = 0, next_id = 1;  // id 0: no stream resident
        uint64_t stats[KWOK_WATCH_STAT_COUNT] = {};
        // the List body framer (json.hip k_list_*): eight arrays of per-tile words,
        // the candidates' `{` offsets (their `}` go to ends), its counters
        DevArr<uint32_t> ltile;        // [8][ltiles.cap]
        static size_t eight(size_t cap) { return 8 * cap; }
        DevGroup ltiles{1024, {{ltile, eight}}};
        DevArr<uint32_t> starts;       // [cands.cap]
        DevGroup cands{4096, {starts}};
        DevArr<uint32_t> lc;           // [KWOK_LIST_COUNTERS]
        Pinned<uint32_t> lc_h;         // [KWOK_LIST_COUNTERS]
        uint64_t lstats[KWOK_LIST_STAT_COUNT] = {};
        // the response framer (json.hip k_resp_parse): the documents' spans (nothing is
        // allocated before the first kwok_frame_responses_gpu)
        DevArr<uint64_t> r_off;        // [rspans.cap]
        DevArr<uint32_t> r_len;        // [rspans.cap]
        DevGroup rspans{4096, {r_off, r_len}};
        uint64_t rstats[KWOK_RESP_STAT_COUNT] = {};
    } watch;

    // ---- relist with Replace (resync.hip, kwok_watch.h): a `seen` byte per slot of each
    // kind (allocated at the kind's first begin), the sweep's tile counts and outputs ----
    struct KWOK_LOCAL Resync {
        DevArr<uint8_t> pod_seen;      // [PLa] re-laid out with the pod arrays (grow_pods)
        DevArr<uint8_t> node_seen;     // [NLa]
        bool open[2] = {false, false}; // KWOK_KIND_*: a session is open (the ingests mark)
        DevArr<ResyncCounters> ctr;
        Pinned<ResyncCounters> ctr_h;
        DevArr<uint32_t> tile_cnt, tile_base;
        DevGroup tiles{1024, {tile_cnt, tile_base}};
        DevArr<uint32_t> total;        // [1]
        Pinned<uint32_t> total_h;      // [1]
        DevArr<int32_t> d_handles, d_nodes;  // [swept.cap] the swept handles / their nodes, emit order
        DevGroup swept{4096, {d_handles, d_nodes}};
        DevArr<int32_t> d_mark;        // [marks.cap] kwok_resync_mark's handles
        DevGroup marks{4096, {d_mark}};
        uint64_t stats[KWOK_RESYNC_STAT_COUNT] = {};
    } resync;

    // ---- the pod uid directory (uid.hip, kwok_watch.h): a uid per pod slot, the table
    // of hints, the per-call buffers of a by-uid framed batch and of bind / lookup ----
    struct KWOK_LOCAL Uid {
        struct Bytes {
            uint8_t b[KWOK_UID_MAX];
        };
        bool on = false;
        DevArr<Bytes> pod_uid;           // [PLa] re-laid out with the pod arrays (grow_pods)
        DevArr<uint8_t> pod_uid_len;     // [PLa]
        DevArr<unsigned long long> tab;
        size_t tab_cap = 0;              // entries (a power of two)
        int forced_log2 = 0;             // KWOK_UID_TAB_LOG2 (tests)
        uint64_t live = 0, inserted = 0; // entries at the last rebuild; an upper bound of the inserts since
        DevArr<UidCounters> ctr;
        Pinned<UidCounters> ctr_h;
        DevArr<UidRun> run;
        Pinned<UidRun> run_h;
        // per record of a by-uid batch
        DevArr<uint32_t> fidx, uoff, res_rel;
        DevArr<uint8_t> ulen, cls;
        DevArr<uint64_t> hash;
        DevArr<int32_t> res_h, res_st;
        DevGroup recs{4096, {fidx, uoff, res_rel, ulen, cls, hash, res_h, res_st}};
        DevArr<uint32_t> claim;
        DevGroup claims{0, {claim}};     // (sized by claim_size: no headroom)
        // bind / lookup: handles or results, spans, the caller's arena
        DevArr<int32_t> q_h;
        DevArr<uint64_t> q_off;
        DevArr<uint32_t> q_len;
        DevGroup spans{4096, {q_h, q_off, q_len}};
        DevArr<uint8_t> q_arena;
        DevGroup arena{1 << 16, {q_arena}};
        // the by-uid batch whose records the ingest is applying (null: an entry that carries no uid)
        const UidNote* note = nullptr;
        std::vector<hipEvent_t> note_ev;  // KWOK_INGEST_PROF: stamps around each k_uid_note of a by-uid batch, in pairs
        uint64_t stats[KWOK_UID_STAT_COUNT] = {};
        UidDir dir() const { return UidDir{reinterpret_cast<uint8_t*>(pod_uid.p), pod_uid_len, tab, (uint32_t)(tab_cap - 1), ctr}; }
    } uid;

    // ---- the echo ledger (echo.hip, kwok_watch.h): the pool of noted uids behind its table,
    // the per-call buffers of a filtered batch ----
    struct KWOK_LOCAL Echo {
        bool on = false;
        DevArr<uint32_t> tab;
        size_t tab_cap = 0;           // entries (a power of two)
        DevArr<EchoEntry> pool;
        size_t pool_cap = 0;
        int forced_log2 = 0;          // KWOK_ECHO_TAB_LOG2 (tests)
        DevArr<EchoCounters> ctr;
        Pinned<EchoCounters> ctr_h;   // the counters after the last call
        DevArr<EchoCall> call;
        Pinned<EchoCall> call_h;
        uint64_t rebuilds = 0;
        // per record of a call
        DevArr<uint32_t> uoff, roff, own, cnt, fill, lbase, list, fidx, bsum, kidx, kpos, q_len, res_rel;
        DevArr<uint8_t> ulen, rlen, kind, res;
        DevArr<uint64_t> hash, q_off;
        DevArr<int32_t> hdrop, res_h, res_st;
        DevGroup recs{4096, {uoff, roff, own, cnt, fill, lbase, list, fidx, {bsum, per_tile256}, kidx, kpos, q_len, res_rel,
                             ulen, rlen, kind, res, hash, q_off, hdrop, res_h, res_st}};
        DevArr<uint32_t> claim;
        DevGroup claims{0, {claim}};  // (sized by claim_size: no headroom)
        // the typed front end: spans, ops, statuses and the caller's arena
        DevArr<uint64_t> s_uoff, s_roff;
        DevArr<uint32_t> s_ulen, s_rlen;
        DevArr<uint8_t> s_op;
        DevArr<int32_t> s_status;
        DevGroup spans{4096, {s_uoff, s_roff, s_ulen, s_rlen, s_op, s_status}};
        DevArr<uint8_t> arena;
        DevGroup bytes{1 << 16, {arena}};
        EchoLedger ledger() const { return EchoLedger{tab, (uint32_t)(tab_cap - 1), pool, (uint32_t)pool_cap, ctr}; }
    } echo;

    // ---- the pod and node reference directory (refs.hip, kwok_watch.h): namespace and name per pod
    // slot, the per-call buffers of bind / lookup / read ----
    struct KWOK_LOCAL Refs {
        struct Bytes {
            uint8_t b[KWOK_REF_STRIDE];
        };
        bool on = false;
        DevArr<Bytes> pod_ref;            // [PLa] re-laid out with the pod arrays (grow_pods)
        DevArr<uint16_t> pod_ref_len;     // [PLa]
        DevArr<RefCounters> ctr;
        Pinned<RefCounters> ctr_h;
        // the stale guard: per kind (KWOK_KIND_*), bumped by every call that can create an object of it
        uint64_t gen[2] = {0, 0};
        // lookup / read: handles, sizes, offsets, slots, references, the scan's storage, the blob
        DevArr<uint64_t> q_len, q_off;
        DevArr<uint32_t> q_slot;
        DevArr<kwok_ref> q_refs;
        DevGroup items{4096, {q_len, q_off, q_slot, q_refs}};
        DevArr<void> q_tmp;               // [tmp_bytes] (not zero-filled)
        size_t tmp_bytes = 0;
        DevArr<uint8_t> q_blob;
        DevGroup blob{1 << 16, {q_blob}};
        // bind: the spans (namespaces, then names), the handles (lookup's too) and the caller's arena
        DevArr<uint64_t> b_off;
        DevArr<uint32_t> b_len;
        DevArr<int32_t> q_h;
        DevGroup spans{4096, {{b_off, twice}, {b_len, twice}, q_h}};
        DevArr<uint8_t> b_arena;
        DevGroup arena{1 << 16, {b_arena}};
        // the by-uid batch whose records the ingest is applying (null: an entry that carries no name)
        const RefNote* note = nullptr;
    } refs;
    RefDir ref_dir() const {
        return RefDir{reinterpret_cast<uint8_t*>(refs.pod_ref.p), refs.pod_ref_len, reinterpret_cast<const uint8_t*>(uid.pod_uid.p),
                      uid.pod_uid_len, refs.ctr};
    }

    // ---- the node uid directory (nodes.hip, kwok_watch.h): a uid per node slot (NL is fixed at create:
    // nothing re-lays out node slots), the per-call buffers of lookup / bind and of a framed batch's uid spans ----
    struct KWOK_LOCAL NodeDir {
        struct Bytes {
            uint8_t b[KWOK_UID_MAX];
        };
        bool on = false;
        DevArr<Bytes> node_uid;           // [NL]
        DevArr<uint8_t> node_uid_len;     // [NL + 4] (read by aligned words)
        DevArr<uint64_t> node_uid_key;    // [NL]
        DevArr<NodeDirCounters> ctr;
        Pinned<NodeDirCounters> ctr_h;
        // the device-input ingest's words of a call: the error word (a bad kept index), the rejected records
        struct CallWords {
            unsigned long long rejected;
            uint32_t err, pad;
        };
        DevArr<CallWords> call;
        Pinned<CallWords> call_h;
        // lookup / bind: handles or results, spans, the caller's arena (kwok_node_lookup: also with the directory off)
        DevArr<int32_t> q_h;
        DevArr<uint64_t> q_off;
        DevArr<uint32_t> q_len;
        DevGroup spans{4096, {q_h, q_off, q_len}};
        DevArr<uint8_t> q_arena;
        DevGroup arena{1 << 16, {q_arena}};
        // a framed node batch: its frame indices (an upload of the caller's), its records' uid spans in the resident
        // stream, the host codec's statuses of the documents it decided
        DevArr<uint32_t> fidx, uoff;
        DevArr<uint8_t> ulen;
        DevArr<int32_t> hstat;
        DevGroup recs{4096, {fidx, uoff, ulen, hstat}};
        // the framed batch whose records the node ingest is applying (null: an entry that carries no uid)
        const NodeUidNote* note = nullptr;
        NodeDirX dir() const { return NodeDirX{reinterpret_cast<uint8_t*>(node_uid.p), node_uid_len, node_uid_key, ctr}; }
    } ndir;

    // ---- the pod codec on the GPU (json.hip): per-document buffers, the codec's
    // selectors, the spec table (kwok_spec_key -> spec id) ----
    struct KWOK_LOCAL Json {
        DevArr<uint64_t> off;
        DevArr<uint32_t> len;
        DevArr<uint8_t> op;
        DevArr<int32_t> handle;
        DevArr<JsonPodSide> side;
        DevArr<uint32_t> host_list;
        DevArr<kwok_pod_event> fix_ev;     // the listed documents' records (gathered, completed, scattered)
        DevArr<JsonPodSide> fix_side;
        DevGroup docs{4096, {off, len, op, handle, side, host_list, fix_ev, fix_side}};
        DevArr<uint32_t> n_host;           // [1]
        Pinned<uint32_t> n_host_h;         // [1]
        DevArr<JsonCfg> cfg;
        Pinned<JsonCfg> cfg_h;             // staging
        DevArr<uint64_t> tab_key;
        DevArr<int32_t> tab_id;
        DevArr<int32_t> nstat;             // node documents: the device decode's status per document
        DevArr<kwok_node_event> nev_fix;   // node records gathered for / scattered from the host
        DevGroup node_docs{4096, {nstat, nev_fix}};
        DevArr<uint2> tab_canon;           // per slot: offset / length of its spec's canonical string in canon
        DevArr<uint8_t> canon;             // the registered specs' canonical strings (json_spec_canon)
        DevGroup canon_bytes{4096, {canon}};
        uint32_t tab_mask = 0;
        bool tab_dirty = true;
    } json;

    // ---- node status blobs canonicalised on the device (json.hip k_canon, kwok_canon.h): nothing is
    // allocated before the first node decode with the switch on ----
    struct KWOK_LOCAL Canon {
        bool on = false;
        DevArr<CanonCounters> ctr;         // [1] the scan's: listed documents, their raw blob bytes
        Pinned<CanonCounters> ctr_h;
        DevArr<uint32_t> list;             // [docs.cap] the canon list (batch indices, in the order the scan appended them)
        DevArr<uint64_t> len, off;         // [docs.cap] raw blob bytes per listed document, their exclusive scan
        DevArr<CanonDoc> doc;              // [docs.cap] per listed document: its three (offset, length) pairs
        DevGroup docs{4096, {list, len, off, doc}};
        DevArr<uint8_t> bytes;             // the compact canonical bytes of the call
        DevGroup out{1 << 16, {bytes}};
        DevArr<void> tmp;                  // [tmp_bytes] the scan's storage (not zero-filled)
        size_t tmp_bytes = 0;
        // the last decode's result on the host: the listed documents sorted by batch index, and the bytes
        std::vector<CanonDoc> doc_h;
        std::vector<char> bytes_h;
        uint64_t stats[KWOK_CANON_STAT_COUNT] = {};
        // the clean document i of the last decode, or null
        const CanonDoc* find(uint32_t i) const {
            auto it = std::lower_bound(doc_h.begin(), doc_h.end(), i, [](const CanonDoc& d, uint32_t v) { return d.doc < v; });
            return it != doc_h.end() && it->doc == i && !it->host ? &*it : nullptr;
        }
    } canon;
    std::unordered_map<uint64_t, int32_t> spec_keys;  // kwok_spec_key -> spec id (-2: two specs share the key)
    std::unordered_map<uint64_t, std::string> spec_canon;  // kwok_spec_key -> the canonical string of its spec

    // ---- specs / blobs ----
    std::unordered_map<std::string, int32_t> spec_ids;
    uint32_t hb_len = HB_LEN, hb_stride = HB_STRIDE;  // heartbeat patch bytes / arena stride (16-aligned)
    HeartbeatTemplate hb_tpl;     // the heartbeat template (default or compiled from Config.NodeHeartbeatTemplate)
    bool custom_hb = false;
    std::string hb_tpl_text;
    bool custom_pod = false;      // Config.PodStatusTemplate in use (compiled per spec)
    bool custom_node = false;     // Config.NodeInitializationTemplate in use (compiled per node status)
    std::string pod_tpl, node_tpl, start_s;  // their texts; StartTime() (RFC3339 of start_time_unix)
    std::unordered_map<std::string, uint64_t> node_tpl_blobs;  // node status fields -> compiled blob
    std::vector<SpecDesc> specs_h;
    std::string spec_bytes_h;
    DevBuf<SpecDesc> d_specs;
    DevBuf<uint8_t> d_spec_bytes;
    std::vector<uint16_t> spec_nxt_h;  // timestamp lookups of every spec (build_ts_lookup)
    DevBuf<uint16_t> d_spec_nxt;
    DevBuf<uint8_t> d_unit_tab;      // k_emit's unit tables (16 bytes per unit), appended per spec
    DevBuf<uint16_t> d_unit_desc;
    uint32_t tab_units = 0;
    uint32_t max_pod_len = 0;
    std::unordered_map<std::string, uint64_t> blob_ids;
    uint64_t empty_blob = 0;      // the blob of a node with an empty status (every status field absent)
    std::atomic<bool> has_empty_blob{false};
    std::string blob_h;
    size_t blob_up_lo = SIZE_MAX;  // blob_h bytes from here on are not on the device yet (upload_blobs)
    DevBuf<uint8_t> d_blob;
    uint32_t max_init_len = 0;

    // ---- tick ----
    // A tick's outputs (header, lists, arena) live in one of two slots, so tick N+1
    // can be queued while tick N is collected (kwok_tick_submit / _collect).  Slot 1
    // is allocated on the first submit that finds slot 0 busy.
    struct TickSlot {
        TickHdr* hdr_h = nullptr;  // pinned: k_tick publishes the field totals here
        uint8_t* arena = nullptr;
        uint64_t arena_cap = 0;
        int32_t *hb_nodes = nullptr, *init_nodes = nullptr, *pp_pods = nullptr, *del_pods = nullptr;
        uint64_t *init_off = nullptr, *pp_off = nullptr;
        uint32_t *init_len = nullptr, *pp_len = nullptr;
        uint8_t* del_fin = nullptr;
        DevState* d_S = nullptr;    // S with this slot's outputs, in device memory (out-of-line kernel phases)
        DevState* S_pin = nullptr;  // pinned staging for its upload
        DevState S_up{};            // the copy last uploaded
        hipEvent_t done = nullptr;  // recorded after the tick's launches
        hipEvent_t pev[8] = {};     // profiling: FRONT(+BACK) launch start/stop, BACK launch start/stop, k_emit,
                                    // k_pod_jobs
        uint4* pp_job = nullptr;    // k_tick -> k_emit job records
        uint64_t* init_job = nullptr;
        uint32_t* emit_n = nullptr;
        bool emit_queued = false;   // k_emit was enqueued behind the tick's launches
        bool split = false;         // TICK_SPLIT: k_pod_jobs builds the pod jobs after the tick's launches
        bool fuse = false;          // ... and writes their patch bytes itself (DevState::fuse_pods)
        bool inits_folded = false;  // ... and the node inits' too (no k_emit launch: KWOK_FOLD_INITS)
        bool quiet = false;         // only pods with an event are Use-checked (kwok_engine::quiet)
        bool once = false;          // launched as k_once / k_once_stream (a tick expected to have nothing to emit)
        bool once_stream = false;   // ... as k_once_stream: the engine writes every heartbeat body
        bool once_use = false;      // ... reading the per-bucket summaries (counted when it retires as a once tick)
        hipEvent_t rd = nullptr;    // kwok_read_arena_async: the last read queued from this slot's arena
        bool rd_pending = false;    //   (a submit or an arena growth that takes the slot waits for it)
        bool no_once = false;       // k_once found work: the tick runs again with k_tick
        bool alloc = false;
        // What the heartbeat region [0, n x stride) of `arena` provably holds: n complete
        // bodies of the template generation `gen` at `clock`.  Written by retire alone,
        // for a tick that completed without error, was not skipped on the device or
        // requeued, was not redone after k_once_stream found work and ran its stream; cleared by everything that
        // replaces, poisons or is about to overwrite the arena (grow_arena, alloc_slot,
        // every enqueue, so also a failed tick and the debug layout-fault tick) and by a
        // template change.  A tick whose layout matches it exactly writes only the lines
        // that differ from these bodies (hb_prev).
        struct HbValid {
            bool ok = false;
            const uint8_t* arena = nullptr;
            uint32_t n = 0, stride = 0, units = 0, gen = 0;
            uint64_t clock = 0;
        } hb_valid;
        uint64_t hb_prev = 0;       // this tick's stream is a delta against the bodies of this clock (0: all bytes)
        uint32_t hb_n = 0;          // bodies this tick's stream lays out
        bool hb_record = false;     // retire may record this tick's bodies (not requeued, no layout fault, streamed)
        // What `hb_nodes` provably holds: the n handles of a count of state generation gen.
        // Follows HbValid: written by retire of a clean k_once_stream tick in this slot
        // (counted, or reused: the list it found), cleared by every enqueue into the slot
        // and by alloc_slot (the lists are allocated once).  A reused tick needs an exact match.
        struct ListValid {
            bool ok = false;
            const int32_t* list = nullptr;
            uint32_t n = 0;
            uint64_t gen = 0;
        } list_valid;
        bool count_reused = false;  // launched as k_hb_stream: the count is the engine's clean-count record
        bool requeued = false;      // the launch in flight is a requeue (the first one skipped, or the tick was redone)
        uint64_t state_gen = 0;     // the engine's state generation at the tick's enqueue
        // the tick in the slot
        int state = 0;  // SLOT_FREE, SLOT_QUEUED (enqueued), SLOT_DONE (finished on the host, not collected)
        uint64_t now = 0, target = 0;
        uint32_t tag = 0;
        uint32_t epoch = 0;         // heartbeat_epoch of the tick
        uint64_t ref_gen[2] = {0, 0};  // the reference directory's counters at the tick's submit (kwok_read_refs)
        int rc = 0;
        std::string err;
        kwok_tick_result res{};
    };
    TickSlot slots[2];
    int queue[2] = {-1, -1};  // queued / done slots in submission order
    int nq = 0;
    int cur = -1;             // slot of the last collected tick (kwok_read_outputs)
    size_t NLa = 0, PLa = 0;  // output list capacities
    uint64_t arena_need = 0;  // worst-case output bytes of one tick
    ListDesc* d_ld = nullptr;  // [W] or scratch
    ncclComm_t comm = nullptr;
    XMsg* d_xall = nullptr;
    XMsg* h_xall = nullptr;  // pinned
    uint32_t* d_xsend = nullptr;
    uint32_t* d_xrecv = nullptr;
    size_t xlist_cap = 0;
    // TICK_XSPEC: after a tick whose lists were too long to be inline, the next
    // ticks send their lists in a second allgather right behind the messages (no
    // host round trip) with capacities from that tick's longest lists; every rank
    // takes the same decisions (from the same gathered messages, in lockstep)
    uint32_t xspec_u = 0, xspec_r = 0;  // capacities per rank (0: off)
    uint32_t xspec_ttl = 0;             // ticks left
    uint32_t xspec_alloc = 0;           // entries allocated per rank in d_ssend / d_srecv
    uint32_t* d_ssend = nullptr;
    uint32_t* d_srecv = nullptr;
    int xspec_env = -1;                 // KWOK_XSPEC: 0 off, N: ticks kept on after a long-list tick (default 256)
    uint64_t xspec_miss = 0;  // diagnostics: speculative ticks whose lists did not fit
    uint32_t n_stream = 0;      // k_tick heartbeat streamer blocks (the chain blocks: S.n_chain)
    uint32_t n_once_stream = 0; // k_once_stream's streamer blocks (512 threads each; KWOK_ONCE_STREAMERS), 0: by size
    uint32_t emit_grid = 0;     // k_emit blocks
    bool emit_hint = true;      // events were ingested since the last submit: the tick likely emits patches
    bool sync_spin = true;      // spin on a tick's completion event (KWOK_SYNC=spin, the default)
    bool chain_prio = false;    // KWOK_TICK_PRIO=1: s_setprio 3 on the chain blocks
    bool no_stream = false;     // KWOK_TICK_NO_STREAM=1: diagnostics - heartbeat bodies not written
    bool split_jobs = true;     // KWOK_SPLIT=0: pod jobs of event ticks in the chain blocks (A/B)
    int fuse_emit = -1;         // KWOK_FUSE_EMIT: 1 always / 0 never fuse the pod bytes into k_pod_jobs; -1 dense ticks
    bool sparse_jobs = true;    // unfused split ticks: k_sparse_jobs over FRONT's group records (KWOK_SPARSE_JOBS=0: off)
    bool fold_inits = true;     // KWOK_FOLD_INITS=0: a fused tick's node inits by k_emit (A/B)
    uint64_t pod_records_since_tick = 0;  // pod records ingested since the last tick was enqueued (fused emission)
    uint32_t n_untabled = 0;    // registered specs without unit tables (no fused emission while any)
    // Quiet ticks.  A tick's Use(podIP) of an evaluated pod (pod_controller.go:
    // 378-382) is a no-op when the address is already in `used`.  Only a Put clears
    // a bit, and Puts come from ingest (Deleted events), kwok_pool_put, and the
    // deletions a tick makes of the pods marked at the ingest before it.  So after
    // two submits with nothing in between, the previous tick Use-checked every
    // evaluated pod and released nothing: this tick need only Use-check pods with
    // an event (single rank; KWOK_QUIET=0 checks every pod).
    // Also, while every in-CIDR podIP a live pod holds was assigned to it by this
    // engine (no pod was created or updated with a podIP of its own, and no Deleted
    // event released an address its pod did not hold: the GPU apply pass flags
    // those, IngSummary::foreign), every such address has exactly one holder and
    // stays in `used` until that holder is deleted: then no Use changes anything
    // and the Use checks of pods without an event are skipped in every tick.
    uint32_t quiet = 0;         // submits since the last ingest / pool_put / cni_assign
    bool foreign_ips = false;   // sticky: a podIP not assigned by this engine entered the pool
    bool global_foreign = false;  // multi rank, sticky: some rank's exchange message carried its foreign_ips
    bool quiet_ok = true;
    bool once_ok = true;        // KWOK_ONCE=0: quiet ticks always run k_tick (A/B)
    bool once_stream_ok = true; // KWOK_ONCE_STREAM=0: ... those of engines that write every body (A/B; k_once stays)
    // the last retired tick patched pods that took no address in it (created with an empty
    // status: patched without IPs, their Gets follow in the next tick): that tick is not
    // quiet, whatever the events say.  k_once_stream's prediction only: a redone tick
    // writes its whole stream again, k_tick here writes the changed lines
    bool pp_followup = false;
    // k_once's per-bucket summaries (DevState::once_sum): valid while nothing has changed a
    // pod state since the BUILD tick of generation sum_gen was enqueued (every ingest, CNI
    // assignment, pool Put, zombie sweep and k_tick launch clears sum_valid)
    bool once_sum_ok = true;    // KWOK_ONCE_SUM=0: every k_once tick reads the pod rows (A/B)
    bool sum_valid = false;
    uint32_t sum_gen = 0;
    // Count reuse.  k_once_stream's count (handle list, totals) reads
    // node and pod state words, pod_fill, hb_bpre and the managed count, never `now`: a
    // quiet tick that follows a cleanly counted one with none of those changed in between
    // would count the same again, so it launches the streamers alone (k_hb_stream) and
    // retire fills its header from the record.  state_gen is bumped wherever sum_valid is
    // cleared (every ingest, CNI assignment, pool Put, zombie sweep, redo and k_tick launch)
    // and by every node / pod batch, pod capacity growth and template upload besides;
    // resync sweeps change state through the ingest paths.  A tick records the generation
    // it was enqueued under; a reused tick has no net that finds unexpected work, so the
    // generation alone decides.
    bool count_reuse_ok = true;  // KWOK_COUNT_REUSE=0: every quiet tick counts (A/B, tests)
    uint64_t state_gen = 1;
    void state_changed() {
        sum_valid = false;
        state_gen++;
    }
    // the last clean count: written by retire alone, for a k_once_stream tick that counted
    // and completed without error, redo, device skip or requeue; tot is the device-written
    // part of its header (before derive_header), gen the generation it was enqueued under
    struct CleanCount {
        bool ok = false;
        uint64_t gen = 0;
        uint64_t tot[16] = {};
    } clean_count;
    uint64_t stats[KWOK_STAT_COUNT] = {};  // kwok_engine_stats
    uint8_t* dump_h = nullptr;  // kwok_dump_pods' page-locked staging
    size_t dump_cap = 0;
    bool ingest_zc = true;      // KWOK_INGEST_ZC=0: pod batches in kwok_host_alloc memory copied to HBM first
    bool results_stream = true;   // KWOK_INGEST_RS=0: a chunked batch's results copied on the engine stream
    bool results_kernel = false;  // KWOK_INGEST_RESULTS_KERNEL=1: pod batch results written into mapped host arrays by a kernel
    double last_chunk_cut = 0.4;  // KWOK_INGEST_LAST_CUT: a chunked batch's last chunk is (1 - this) of the others
    bool new_mapped = true;       // KWOK_INGEST_NEW_MAPPED=0: kwok_pod_rec12 create handles copied back, not written in place
    bool hb_delta = true;       // KWOK_HB_DELTA=0: every tick writes the whole heartbeat stream (A/B, tests)
    uint32_t hb_gen = 0;        // heartbeat template generation (bumped by every upload of the template or `start`)
    int nt_env = -1;            // KWOK_HB_NT (0 / 1: heartbeat stores plain / non-temporal), else automatic
    int keep_env = -1;          // KWOK_HB_KEEP (0..64 of every 64 groups of a non-temporal delta stream stored plain), else
                                // automatic: HB_KEEP_BUDGET's share on the quiet ticks of a region past the Infinity Cache
    int share_env = -1;         // KWOK_TICK_STREAM_SHARE (/1024 of the stream to the streamer blocks), else automatic
    uint32_t tick_tag = 0;      // nonzero id of the last FRONT launch
    uint64_t front_launches = 0;  // FRONT launches since the cross-block state was last zeroed
    // diagnostics
    bool prof = false;
    double prof_ms[KWOK_T_COUNT] = {};
    uint64_t prof_ticks = 0;
    double host_ms[KWOK_H_COUNT] = {};
    // KWOK_TICK_TRACE=1: per-block phase stamps, summarised on stderr at destroy
    std::vector<uint64_t> trace_h;
    double trace_sum[TRACE_SLOTS + 2][3] = {};  // chain stamps, streamer entry / exit
    uint64_t trace_ticks = 0, trace_seen = 0;
    uint64_t host_ticks = 0;
    // a failed tick leaves device and host state out of step: every later call
    // fails with KWOK_EDEVICE (destroy and recreate the engine, re-ingest by List)
    bool poisoned = false;
    bool iprof = false;
    WorkPool workers;  // host threads of the ingest partitions  // KWOK_INGEST_PROF=1: host ingest / retire phase times on stderr
    uint32_t debug_fail_chunk = 0;  // KWOK_DEBUG_INGEST_FAIL_CHUNK=N: chunk N of a pod batch fails before its apply (tests)
    uint32_t debug_fail_apply = 0;  // KWOK_DEBUG_INGEST_FAIL_APPLY=N: chunk N fails after its first apply pass (tests)
    // the pod batch in progress changed the state (placeholder nodes, capacity, the
    // apply pass): a failure from then on leaves the batch partly applied (poison)
    bool ing_mutated = false;
    uint32_t ing_chunk = 0;     // the chunk ingest_chunk works on (debug injection)
    uint64_t debug_fault_tick = 0;  // KWOK_DEBUG_LAYOUT_FAULT_TICK=N: tick N gets a wrong heartbeat layout (tests)

    int fail(int code, const char* fmt, ...) {
        char b[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(b, sizeof b, fmt, ap);
        va_end(ap);
        err = b;
        return code;
    }
    bool owns(uint32_t bucket) const { return bucket >= b_lo && bucket < b_hi; }
    // pod handle <-> local slot (bucket_local * Cp + index)
    int32_t pod_handle(uint32_t slot) const { return (int32_t)((b_lo + slot / Cp) * Hs + slot % Cp); }
    // KWOK_OK (slot set), KWOK_ENOTMINE (another rank's bucket) or KWOK_ENOTFOUND
    int pod_slot(int64_t h, uint32_t* slot) const {
        if (h < 0 || h / Hs >= B) return KWOK_ENOTFOUND;
        const uint32_t b = (uint32_t)(h / Hs), i = (uint32_t)(h % Hs);
        if (!owns(b)) return KWOK_ENOTMINE;
        if (i >= Cp) return KWOK_ENOTFOUND;
        *slot = (b - b_lo) * Cp + i;
        return KWOK_OK;
    }
};

#define HIPCHK(e, x)                                                                              \
    do {                                                                                          \
        hipError_t _r = (x);                                                                      \
        if (_r != hipSuccess) return (e)->fail(KWOK_EDEVICE, "%s: %s", #x, hipGetErrorString(_r)); \
    } while (0)

#pragma GCC visibility push(hidden)

namespace kwok {

template <class T>
int dalloc(kwok_engine* e, T** p, size_t n) {
    size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    hipError_t r = hipMalloc((void**)p, bytes);
    if (r != hipSuccess) return e->fail(KWOK_ENOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(r));
    r = hipMemsetAsync(*p, 0, bytes, e->st);
    if (r != hipSuccess) return e->fail(KWOK_EDEVICE, "hipMemset: %s", hipGetErrorString(r));
    return KWOK_OK;
}
template <class T>
void dfree(T*& p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}

// grow a device buffer to hold `bytes` (keeps contents)
template <class T>
int dgrow(kwok_engine* e, DevBuf<T>& b, size_t n) {
    if (n <= b.n) return KWOK_OK;
    size_t cap = std::max<size_t>(n, b.n * 2 + 64);
    T* p = nullptr;
    if (hipMalloc((void**)&p, cap * sizeof(T)) != hipSuccess) return e->fail(KWOK_ENOMEM, "grow %zu", cap * sizeof(T));
    if (b.p) {
        HIPCHK(e, hipMemcpyAsync(p, b.p, b.n * sizeof(T), hipMemcpyDeviceToDevice, e->st));
        HIPCHK(e, hipStreamSynchronize(e->st));
        (void)hipFree(b.p);
    }
    b.p = p;
    b.n = cap;
    return KWOK_OK;
}

template <class T>
int dalloc(kwok_engine* e, DevArr<T>* a, size_t n) {
    return dalloc(e, &a->p, n);
}
template <class T>
void dfree(DevArr<T>& a) {
    a.release();
}

enum { SLOT_FREE = 0, SLOT_QUEUED = 1, SLOT_DONE = 2 };

// ---- helpers defined in one engine*.cpp and called from another --------------------
// engine.cpp
int poisoned(kwok_engine* e);
int exchange(kwok_engine* e, void* send, size_t bytes, void* recv);
// engine_tick.cpp
int size_arena(kwok_engine* e);
int grow_arena(kwok_engine* e, kwok_engine::TickSlot& T);
int alloc_slot(kwok_engine* e, int k);
void free_slot(kwok_engine::TickSlot& T);
int release_for_host(kwok_engine* e);
int enqueue_tick(kwok_engine* e, int k, bool requeue);
int drain(kwok_engine* e);  // finish every queued tick on the host
int tick_submit_check(kwok_engine* e, int64_t now_unix);  // kwok_tick_submit's checks / the rest
int tick_submit_impl(kwok_engine* e, int64_t now_unix);

}  // namespace kwok

#pragma GCC visibility pop
