// engine_tick.cpp - the tick queue: the output slots and their arena, enqueue / retire, submit / collect
// (kernels.hip k_tick, k_once, k_once_stream, k_hb_stream, k_emit) behind include/kwok_engine.h:
// kwok_tick_submit / _collect, kwok_tick, kwok_engine_stats.  What a tick calls on every enqueue and
// retire is defined here, so that it inlines.
//
// Reference interfaces replaced (hezhizhen/kwok, pkg/kwok/controllers):
//   KeepNodeHeartbeat, LockNodes, LockPods, DeletePods    node_controller.go:175-204,301-354, pod_controller.go:155-250
#include "engine_state.h"

namespace kwok {

// the output arena must hold the worst case of one tick.  It changes when the
// capacity, the specs or the node blobs do (ingest, registration), and is
// reserved then for the slots the next submit may take (a free slot whose outputs
// the caller is not reading), not inside that tick: the 1M x 10M fleet's first
// tick would otherwise reallocate ~8 GB (~0.7 ms of its enqueue).  A slot still
// queued grows at its next submit.
int size_arena(kwok_engine* e) {
    e->arena_need = (uint64_t)e->NL * e->hb_stride + (uint64_t)e->NL * ((e->max_init_len + 15u) & ~15u) +
                    (uint64_t)e->PL * e->max_pod_len + 256;
    for (int i = 0; i < 2; i++) {
        kwok_engine::TickSlot& T = e->slots[i];
        if (T.alloc && T.state == SLOT_FREE && i != e->cur)
            if (int rc = grow_arena(e, T)) return rc;
    }
    return KWOK_OK;
}
int grow_arena(kwok_engine* e, kwok_engine::TickSlot& T) {  // T holds no queued tick
    if (e->arena_need <= T.arena_cap) return KWOK_OK;
    if (T.rd_pending) {  // (an asynchronous read of the old arena still in flight)
        if (hipEventSynchronize(T.rd) != hipSuccess) return e->fail(KWOK_EDEVICE, "kwok_read_arena_async");
        T.rd_pending = false;
    }
    const uint64_t need = std::max<uint64_t>(e->arena_need, T.arena_cap + T.arena_cap / 2);
    if (T.arena) (void)hipFree(T.arena);
    T.arena = nullptr;
    T.arena_cap = 0;
    T.hb_valid.ok = false;  // a new (possibly poisoned) arena holds no bodies
    if (hipMalloc((void**)&T.arena, need) != hipSuccess) return e->fail(KWOK_ENOMEM, "arena %llu", (unsigned long long)need);
    T.arena_cap = need;
    if (getenv("KWOK_DEBUG_POISON"))  // diagnostics: bytes no kernel writes read as 0xEE, not as stale data
        HIPCHK(e, hipMemsetAsync(T.arena, 0xEE, need, e->st));
    return KWOK_OK;
}
int alloc_slot(kwok_engine* e, int k) {
    kwok_engine::TickSlot& T = e->slots[k];
    int rc = 0;
    T.hb_valid.ok = false;
    T.list_valid.ok = false;
    if ((rc = dalloc(e, &T.hb_nodes, e->NLa)) || (rc = dalloc(e, &T.init_nodes, e->NLa)) ||
        (rc = dalloc(e, &T.init_off, e->NLa)) || (rc = dalloc(e, &T.init_len, e->NLa)) ||
        (rc = dalloc(e, &T.pp_pods, e->PLa)) || (rc = dalloc(e, &T.pp_off, e->PLa)) || (rc = dalloc(e, &T.pp_len, e->PLa)) ||
        (rc = dalloc(e, &T.del_pods, e->PLa)) || (rc = dalloc(e, &T.del_fin, e->PLa)) || (rc = dalloc(e, &T.d_S, 1)) ||
        (rc = dalloc(e, &T.pp_job, e->PLa)) || (rc = dalloc(e, &T.init_job, e->NLa)) || (rc = dalloc(e, &T.emit_n, 2)))
        return rc;
    // the header is coherent host memory written with system-scope stores, so the
    // completion event needs no system-scope release (measured ~1.7 us per tick)
    if (hipHostMalloc((void**)&T.hdr_h, sizeof(TickHdr), hipHostMallocCoherent) != hipSuccess ||
        hipHostMalloc((void**)&T.S_pin, sizeof(DevState), hipHostMallocDefault) != hipSuccess)
        return e->fail(KWOK_ENOMEM, "pinned tick header");
    memset(T.hdr_h, 0, sizeof(TickHdr));
    if (hipEventCreateWithFlags(&T.done, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess)
        return e->fail(KWOK_EDEVICE, "event create");
    for (auto& ev : T.pev)
        if (e->prof && !ev) HIPCHK(e, hipEventCreate(&ev));
    T.alloc = true;
    return KWOK_OK;
}
void free_slot(kwok_engine::TickSlot& T) {
    void* ptrs[] = {T.arena, T.hb_nodes, T.init_nodes, T.init_off, T.init_len, T.pp_pods,
                    T.pp_off, T.pp_len, T.del_pods, T.del_fin, T.d_S, T.pp_job, T.init_job, T.emit_n};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (T.hdr_h) (void)hipHostFree(T.hdr_h);
    if (T.S_pin) (void)hipHostFree(T.S_pin);
    if (T.done) (void)hipEventDestroy(T.done);
    if (T.rd) (void)hipEventDestroy(T.rd);
    for (auto& ev : T.pev)
        if (ev) (void)hipEventDestroy(ev);
}
}  // namespace kwok

namespace {
// this slot's outputs into S (what launches read), uploaded to the slot's device copy if changed
int bind_slot(kwok_engine* e, int k) {
    kwok_engine::TickSlot& T = e->slots[k];
    DevState& S = e->S;
    S.arena = T.arena;
    S.arena_cap = T.arena_cap;
    S.hb_nodes = T.hb_nodes;
    S.init_nodes = T.init_nodes;
    S.init_off = T.init_off;
    S.init_len = T.init_len;
    S.pp_pods = T.pp_pods;
    S.pp_off = T.pp_off;
    S.pp_len = T.pp_len;
    S.del_pods = T.del_pods;
    S.del_fin = T.del_fin;
    S.hdr_host = T.hdr_h;
    S.self = T.d_S;
    S.pp_job = T.pp_job;
    S.init_job = T.init_job;
    S.emit_n = T.emit_n;
    if (memcmp(&T.S_up, &S, sizeof(DevState)) != 0) {  // pointers / sizes changed since the last upload
        *T.S_pin = S;  // the slot's previous upload has completed (its tick was collected)
        HIPCHK(e, hipMemcpyAsync(T.d_S, T.S_pin, sizeof(DevState), hipMemcpyHostToDevice, e->st));
        T.S_up = S;
    }
    return KWOK_OK;
}
}  // namespace

namespace kwok {
// Tick completion events skip the system-scope release (the tick header is
// written with system-scope stores), so before a copy engine reads what the
// kernels wrote, record an event that performs it: the kernels' dirty L2 lines
// (per XCD, not coherent with the copy engine) are written back first.
int release_for_host(kwok_engine* e) {
    HIPCHK(e, hipEventRecord(e->fence, e->st));
    return KWOK_OK;
}
}  // namespace kwok

namespace {

// k_emit for slot k's tick (S bound to slot k), behind its k_tick launch(es)
int enqueue_emit(kwok_engine* e, int k) {
    kwok_engine::TickSlot& T = e->slots[k];
    if (e->prof) HIPCHK(e, hipEventRecord(T.pev[4], e->st));
    launch_emit(e->S, e->emit_grid, T.now, (uint64_t)e->start, e->st);
    HIPCHK(e, hipGetLastError());
    if (e->prof) HIPCHK(e, hipEventRecord(T.pev[5], e->st));
    T.emit_queued = true;
    return KWOK_OK;
}

}  // namespace

namespace kwok {
// Enqueue one tick on e->st into slot k.  Single rank: ONE persistent k_tick
// launch (no host synchronisation, no graph needed).  Multi-rank: k_tick FRONT
// (classify, bases, exchange message) -> allgather -> k_tick BACK (fold
// messages, lists, pool, emission).  requeue: the slot's tick was skipped on
// the device (queued behind a tick that needed finish_long_lists) and runs
// again with its own tag and arrival target.
int enqueue_tick(kwok_engine* e, int k, bool requeue) {
    DevState& S = e->S;
    kwok_engine::TickSlot& T = e->slots[k];
    hipStream_t st = e->st;
    // KWOK_INGEST_PROF: the host time to each launch of the tick (us after entry)
    const auto q0 = clk::now();
    double qs[4] = {-1, -1, -1, -1};  // hb_pre queued, slot bound, k_tick / k_once queued, k_pod_jobs queued
    auto qstamp = [&](int i) { if (e->iprof) qs[i] = ms_between(q0, clk::now()) * 1e3; };
    hipEvent_t* ev = e->prof ? T.pev : nullptr;
    uint32_t nhb = (uint32_t)e->n_managed;  // = the device's count of managed local node slots
    const bool fault_tick = e->debug_fault_tick && e->front_launches + 1 == e->debug_fault_tick && !requeue;
    if (fault_tick) nhb++;  // tests: TICK_ERR_LAYOUT
    // the delta stream: only when the slot's record says its arena holds exactly this
    // tick's layout of bodies.  Multi-rank and heartbeat-once engines always write
    // everything, and so does a requeued tick (its slot's first launch was skipped)
    {
        const kwok_engine::TickSlot::HbValid& V = T.hb_valid;
        const bool can = e->hb_delta && !S.hb_once && !e->multi && !requeue && !fault_tick && !e->no_stream && V.ok &&
                         V.arena == T.arena && V.n == nhb && V.stride == e->hb_stride && V.units == S.hb_units &&
                         V.gen == e->hb_gen;
        T.hb_prev = can ? V.clock : 0;
        T.hb_n = nhb;
        T.hb_record = !requeue && !fault_tick && !e->no_stream && !S.hb_once && !e->multi;
        T.hb_valid.ok = false;  // the region is being rewritten: known again when this tick retires
    }
    T.requeued = requeue;
    T.state_gen = e->state_gen;
    if (e->hb_pre_dirty) {
        // heartbeat handles are written in node order at per-chain-block bases:
        // managed nodes of the buckets before each block's range (k_hb_pre, from
        // the node batches' per-bucket counts)
        launch_hb_pre(S, e->d_hb_pre, e->d_hb_bpre, st);
        HIPCHK(e, hipGetLastError());
        e->hb_pre_dirty = false;
        qstamp(0);
    }
    // a long heartbeat stream is shared with the chain blocks once they are done
    // (measured at C2: 921/1024 to the streamers; short streams: streamers only)
    // a stream that fits the 256 MB Infinity Cache is rewritten from it every tick
    // (plain stores); a larger one (1M nodes: 1.07 GB) is written non-temporally:
    // 239 -> 216 us per 1M x 10M tick (no L2 pollution under the chain's reads,
    // no dirty L2 left for the kernel-end write-back)
    const uint64_t hb_bytes = (S.hb_once ? std::min<uint32_t>(nhb, 1u) : nhb) * (uint64_t)e->hb_stride;
    S.hb_nt = e->nt_env >= 0 ? (uint32_t)e->nt_env : (hb_bytes >= (256ull << 20) ? 1u : 0u);
    // (a delta tick's stores are whole 64-byte lines a quarter of a body apart: plain and
    // non-temporal stores measured the same, tools/micro/fill_sparse.hip; the rule stays)
    // the streamers' share: with the non-temporal stream the chain blocks finish
    // sooner (1M x 10M: classification 172 -> 122 us) and take more of the tail
    // (tools/share_sweep2.sh: 921 -> 860 /1024, 217 -> 208 us per tick)
    // ticks that likely emit pod jobs (events since the last tick) build them in
    // k_pod_jobs, one wave per two dirty 64-group runs, instead of the chain blocks'
    // serial chunk walk (KWOK_SPLIT=0: the chain blocks, for A/B)
    T.split = T.emit_queued && e->split_jobs;
    // ... writing the pod patch bytes there too when every spec has unit tables
    // (no 16-byte job record per patch written by k_pod_jobs and read back by k_emit)
    // and the tick is dense: pod records ingested since the last tick (creates,
    // updates, deletes: a bound on the patches their pods can need) >= 1/4 of the pod slots,
    // so most dirty runs hold hundreds of jobs (1M x 10M initial tick: emission
    // 1.79 -> 1.72 ms).  A sparse tick's runs hold a few jobs each; their serial
    // emission per wave loses to k_emit's packed 64-job chunks (C4 churn tick
    // 0.51 -> 0.57 ms fused; tools/gpu_r6b.sh)
    if (!requeue) {  // (a requeued tick keeps its decision)
        const bool dense = e->pod_records_since_tick * 4 >= (uint64_t)S.nb * e->Cp;
        e->pod_records_since_tick = 0;
        T.fuse = T.split && e->n_untabled == 0 && (e->fuse_emit > 0 || (e->fuse_emit < 0 && dense));
    }
    S.fuse_pods = T.fuse ? 1u : 0u;
    S.sparse_jobs = T.split && !T.fuse && e->sparse_jobs ? 1u : 0u;
    T.inits_folded = false;  // (set where k_pod_jobs is launched)
    // ... and leave the whole stream to the streamers: a dirty chain block's share
    // of it would hold up the pool phase, which waits for every dirty block
    // a tick expected to have nothing to emit (no events since the previous tick, quiet
    // Use checks) is counted by k_once: one wave per bucket, every load of the bucket in
    // flight at once.  One that has work after all is run again with k_tick by retire
    // (TickHdr::redo; a launch queued behind it skips).  A heartbeat-once engine's is
    // k_once alone; an engine that writes every body runs k_once_stream, the same count
    // beside the heartbeat streamers (KWOK_ONCE_STREAM=0: k_tick, for A/B)
    if (!requeue) T.no_once = false;
    T.once = !e->multi && e->once_ok && !T.emit_queued && !T.split && T.quiet && !T.no_once &&
             S.cn <= (uint32_t)ONCE_NODE_LDS && e->PL < (1u << ONCE_FIELD_BITS) && e->NL < (1u << ONCE_FIELD_BITS) &&
             (S.hb_once || (e->once_stream_ok && e->n_stream > 0 && !e->no_stream && !e->pp_followup));
    T.once_stream = T.once && !S.hb_once;
    // count reuse: the engine holds a clean count of this very state and the slot's handle list
    // is that count's - the streamers alone (k_hb_stream); retire fills the header from the record
    {
        const kwok_engine::TickSlot::ListValid L = T.list_valid;
        const kwok_engine::CleanCount& C = e->clean_count;
        T.list_valid.ok = false;  // (whatever runs may write the list: known again when this tick retires)
        T.count_reused = T.once_stream && !requeue && !fault_tick && e->count_reuse_ok && C.ok && C.gen == e->state_gen &&
                         C.tot[AG_HB] == nhb && L.ok && L.list == T.hb_nodes && L.n == nhb && L.gen == e->state_gen;
    }
    // a non-temporal delta stream keeps a share of its lines in the Infinity Cache: the dirty
    // lines of a slot are the same addresses tick after tick, so hb_keep of every 64 groups are
    // stored plain and overwritten on die, and HBM takes the rest (all plain
    // cycles both slots' lines through the cache and keeps none).  The share is what fits
    // HB_KEEP_BUDGET over the allocated slots' dirty lines: one slot (blocking ticks) holds
    // twice the share of two.  On the quiet ticks (k_hb_stream, k_once_stream); a k_tick delta
    // tick, whose classification reads share that cache, stays all non-temporal until its own
    // A/B is repeated (one C4 run with the share forced was faster).
    // KWOK_HB_KEEP forces a value on every delta tick (A/B, tests; 0: no share)
    S.hb_keep = 0;
    if (T.hb_prev && S.hb_nt) {
        if (e->keep_env >= 0) {
            S.hb_keep = (uint32_t)e->keep_env;
        } else if (T.once && hb_bytes >= (256ull << 20)) {
            const double lines = hb_dirty_lines_per_body(e->hb_tpl.now_slots.data(), e->hb_tpl.now_slots.size(), S.hb_units,
                                                         T.hb_prev, T.now);
            const double dirty = ((e->slots[0].alloc ? 1 : 0) + (e->slots[1].alloc ? 1 : 0)) * (double)nhb * lines * 64.0;
            S.hb_keep = dirty > 0 ? (uint32_t)std::min(64.0, 64.0 * (double)HB_KEEP_BUDGET / dirty) : 0u;
        }
    }
    // (k_once_stream's counting blocks are done in ~10 us: the stream is the streamers')
    S.stream_share = e->n_stream == 0 ? 0u
                     : T.count_reused  ? 1024u  // (nobody else to write a tail)
                     : e->share_env >= 0 ? (uint32_t)e->share_env
                                         : (hb_bytes < (32ull << 20) || T.split || T.hb_prev || T.once_stream ? 1024u
                                            : S.hb_nt                                        ? 860u
                                                                                             : 921u);
    S.use_events_only = T.quiet ? 1u : 0u;
    S.foreign = e->foreign_ips ? 1u : 0u;
    int rc = bind_slot(e, k);
    if (rc) return rc;
    qstamp(1);
    const int prof = (ev ? TICK_PROF : 0) | (e->chain_prio ? TICK_PRIO : 0) | (e->no_stream ? TICK_NOSTREAM : 0) |
                     (T.split ? TICK_SPLIT : 0);
    if (!requeue) {
        memset(T.hdr_h, 0, sizeof(TickHdr));  // the slot's previous tick was collected
        if (++e->tick_tag == 0) e->tick_tag = 1;
        T.tag = e->tick_tag;
        T.target = ++e->front_launches * S.n_chain;
    }
    const uint64_t now = T.now;
    if (T.once) {
        // per-bucket summaries: BUILD them on the first once tick after a change, USE them after
        uint32_t mode = ONCE_SUM_OFF;
        if (e->once_sum_ok && e->Cp <= 0xFFFFu) {
            if (!e->sum_valid) {
                if (++e->sum_gen == 0) e->sum_gen = 1;
                e->sum_valid = true;
                mode = ONCE_SUM_BUILD;
            } else {
                mode = ONCE_SUM_USE;
            }
        }
        T.once_use = mode == ONCE_SUM_USE;
        // k_once_stream's 512-thread streamer blocks: one per CU, two (16 streaming waves) for a
        // region past the Infinity Cache (hb_nt's size).  1M x 10M: 0.1146 ms per step with one,
        // 0.1088 with two; 100k x 1M: 0.0156 with one, 0.0177 with two (profiles/q1_layout_ab.txt)
        const uint32_t n_os = e->n_once_stream ? e->n_once_stream : hb_bytes >= (256ull << 20) ? 2 * e->n_stream : e->n_stream;
        if (T.count_reused)
            launch_hb_stream(S, n_os, now, (uint64_t)e->start, nhb, prof & (TICK_PROF | TICK_NOSTREAM), T.hb_prev, st,
                             ev ? ev[0] : nullptr, ev ? ev[1] : nullptr);
        else if (T.once_stream)
            launch_tick_once_stream(S, n_os, now, (uint64_t)e->start, nhb, prof & (TICK_PROF | TICK_NOSTREAM), mode,
                                    e->sum_gen, T.hb_prev, st, ev ? ev[0] : nullptr, ev ? ev[1] : nullptr);
        else
            launch_tick_once(S, now, (uint64_t)e->start, nhb, prof & TICK_PROF, mode, e->sum_gen, st, ev ? ev[0] : nullptr,
                             ev ? ev[1] : nullptr);
        HIPCHK(e, hipGetLastError());
        qstamp(2);
    } else if (!e->multi) {
        e->state_changed();  // (a k_tick may change pod states)
        launch_tick(S, e->n_stream, now, (uint64_t)e->start, nhb, TICK_FRONT | TICK_BACK | prof, T.tag, T.target, st,
                    ev ? ev[0] : nullptr, ev ? ev[1] : nullptr, T.hb_prev);
        HIPCHK(e, hipGetLastError());
        qstamp(2);
    } else {
        e->state_changed();
        launch_tick(S, e->n_stream, now, (uint64_t)e->start, nhb, TICK_FRONT | prof, T.tag, T.target, st,
                    ev ? ev[0] : nullptr, ev ? ev[1] : nullptr);
        // one allgather of the fixed-size exchange message, then BACK: it folds the
        // gathered messages and applies the inline lists itself (no host round trip).
        // Lists too long to be inline: BACK flags it and the host finishes the tick
        // with a second allgather (finish_long_lists).
        // After a long-list tick (TICK_XSPEC): the lists follow in a second allgather
        // of fixed capacity and k_pool_apply_spec applies them if every rank's fit.
        if (!requeue && e->xspec_ttl && --e->xspec_ttl == 0) e->xspec_u = e->xspec_r = 0;
        const bool spec = e->xspec_u + e->xspec_r != 0;
        if (spec) {
            S.xcap_u = e->xspec_u, S.xcap_r = e->xspec_r;
            launch_gather_lists(S, e->d_ssend, st, S.xcap_u, S.xcap_u, S.xcap_r);
            HIPCHK(e, hipGetLastError());
        }
        rc = exchange(e, S.xmsg, sizeof(XMsg), e->d_xall);
        if (rc) return rc;
        if (e->XW > e->W) launch_emulate_msgs(S, e->d_xall, (uint32_t)e->XW, st);  // (diagnostics: one rank, XW > 1)
        if (spec) {
            const uint32_t per = S.xcap_u + S.xcap_r;
            if ((rc = exchange(e, e->d_ssend, (size_t)per * 4, e->d_srecv))) return rc;
            if (e->XW > e->W) launch_emulate_lists(S, e->d_srecv, per, (uint32_t)e->XW, per, st);  // (diagnostics)
            launch_pool_apply_spec(S, e->d_srecv, st);
            HIPCHK(e, hipGetLastError());
        }
        launch_tick(S, e->n_stream, now, (uint64_t)e->start, nhb, TICK_BACK | prof | (spec ? TICK_XSPEC : 0), T.tag,
                    T.target, st, ev ? ev[2] : nullptr, ev ? ev[3] : nullptr);
        HIPCHK(e, hipGetLastError());
    }
    // a fused launch writes the node inits too (its last blocks): no k_emit
    T.inits_folded = T.fuse && e->fold_inits;
    if (T.split) {
        launch_pod_jobs(S, T.tag, st, T.inits_folded ? e->emit_grid : 0u, now, (uint64_t)e->start, ev ? ev[6] : nullptr,
                        ev ? ev[7] : nullptr);
        HIPCHK(e, hipGetLastError());
        qstamp(3);
    }
    // the patch bytes, when events since the last tick make jobs likely (otherwise
    // retire launches k_emit if the tick turns out to have jobs)
    if (T.emit_queued && !T.inits_folded && (rc = enqueue_emit(e, k))) return rc;
    HIPCHK(e, hipEventRecord(T.done, st));
    if (e->iprof)
        fprintf(stderr, "[kwok enqueue] us: hb_pre %.1f, bound %.1f, tick %.1f, pod_jobs %.1f, all %.1f\n", qs[0], qs[1], qs[2],
                qs[3], ms_between(q0, clk::now()) * 1e3);
    return KWOK_OK;
}
}  // namespace kwok

namespace {
// multi rank, after the BACK launch of slot k's tick found lists too long to be
// inline (the same on every rank: the flag comes from the gathered messages):
// gather the lists, apply every rank's Uses and Puts, and run BACK again.  A tick
// queued behind it skipped on the device (GridBar::skip) and is enqueued again.
int finish_long_lists(kwok_engine* e, int k, int next) {
    DevState& S = e->S;
    kwok_engine::TickSlot& T = e->slots[k];
    hipStream_t st = e->st;
    T.hdr_h->xovf = 0;
    // the skipped tick's allgather re-gathered the same messages (its FRONT did not run)
    if (int rc = release_for_host(e)) return rc;
    HIPCHK(e, hipStreamSynchronize(st));
    HIPCHK(e, hipMemcpyAsync(e->h_xall, e->d_xall, sizeof(XMsg) * e->XW, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    uint64_t maxl = 0, mu = 0, mr = 0;
    for (int r = 0; r < e->XW; r++) {
        maxl = std::max<uint64_t>(maxl, e->h_xall[r].n_use + e->h_xall[r].n_rel);
        mu = std::max<uint64_t>(mu, e->h_xall[r].n_use);
        mr = std::max<uint64_t>(mr, e->h_xall[r].n_rel);
    }
    if (e->xspec_env != 0) {
        // the next ticks' speculative list exchange: room for 1.25x this tick's
        // longest lists (the same on every rank: the gathered messages)
        if (e->xspec_u + e->xspec_r) e->xspec_miss++;
        auto cap = [](uint64_t m) { return (uint32_t)std::min<uint64_t>(((m + m / 4) | 1023) + 1, 1u << 30); };
        const bool miss = e->xspec_u + e->xspec_r != 0;  // a speculative tick whose lists did not fit: grow
        const uint32_t cu = miss ? std::max(e->xspec_u, cap(mu)) : cap(mu), cr = miss ? std::max(e->xspec_r, cap(mr)) : cap(mr);
        if (cu + cr > e->xspec_alloc) {
            if (e->d_ssend) (void)hipFree(e->d_ssend);
            if (e->d_srecv) (void)hipFree(e->d_srecv);
            e->d_ssend = e->d_srecv = nullptr;
            e->xspec_alloc = 0;
            if (hipMalloc((void**)&e->d_ssend, (size_t)(cu + cr) * 4) != hipSuccess ||
                hipMalloc((void**)&e->d_srecv, (size_t)(cu + cr) * 4 * e->XW) != hipSuccess)
                return e->fail(KWOK_ENOMEM, "speculative exchange lists");
            e->xspec_alloc = cu + cr;
        }
        e->xspec_u = cu, e->xspec_r = cr;
        e->xspec_ttl = e->xspec_env > 0 ? (uint32_t)e->xspec_env : 256u;
    }
    if (maxl > e->xlist_cap) {
        if (e->d_xsend) (void)hipFree(e->d_xsend);
        if (e->d_xrecv) (void)hipFree(e->d_xrecv);
        e->xlist_cap = maxl;
        if (hipMalloc((void**)&e->d_xsend, maxl * 4) != hipSuccess ||
            hipMalloc((void**)&e->d_xrecv, maxl * 4 * e->XW) != hipSuccess)
            return e->fail(KWOK_ENOMEM, "exchange lists");
    }
    int rc = bind_slot(e, k);
    if (rc) return rc;
    S.fuse_pods = T.fuse ? 1u : 0u;
    S.sparse_jobs = T.split && !T.fuse && e->sparse_jobs ? 1u : 0u;
    HIPCHK(e, hipMemsetAsync(&S.bar->skip, 0, sizeof(uint32_t), st));
    const XMsg& me = e->h_xall[e->rank];
    if (me.n_use + me.n_rel) {  // the chain blocks' list segments, gathered in block order
        launch_gather_lists(S, e->d_xsend, st);
        HIPCHK(e, hipGetLastError());
    }
    rc = exchange(e, e->d_xsend, maxl * 4, e->d_xrecv);
    if (rc) return rc;
    if (e->XW > e->W)  // (diagnostics)
        launch_emulate_lists(S, e->d_xrecv, maxl, (uint32_t)e->XW, (uint32_t)(me.n_use + me.n_rel), st);
    std::vector<ListDesc> ld(e->XW);
    for (int r = 0; r < e->XW; r++) {
        ld[r].use = e->d_xrecv + (size_t)r * maxl;
        ld[r].rel = e->d_xrecv + (size_t)r * maxl + e->h_xall[r].n_use;
        ld[r].n_use = (uint32_t)e->h_xall[r].n_use;
        ld[r].n_rel = (uint32_t)e->h_xall[r].n_rel;
    }
    HIPCHK(e, hipMemcpyAsync(e->d_ld, ld.data(), sizeof(ListDesc) * e->XW, hipMemcpyHostToDevice, st));
    launch_pool_apply(S, e->d_ld, e->XW, (uint32_t)maxl, st);  // every rank's Uses, then Puts pending
    launch_tick(S, e->n_stream, T.now, (uint64_t)e->start, (uint32_t)e->n_managed,
                TICK_BACK | TICK_XLISTS | (T.split ? TICK_SPLIT : 0), T.tag, T.target, st);
    HIPCHK(e, hipGetLastError());
    T.inits_folded = T.fuse && e->fold_inits;
    if (T.split) {
        launch_pod_jobs(S, T.tag, st, T.inits_folded ? e->emit_grid : 0u, T.now, (uint64_t)e->start);
        HIPCHK(e, hipGetLastError());
    }
    if (T.inits_folded) T.emit_queued = true;  // (the fused launch wrote every patch)
    else if ((rc = enqueue_emit(e, k))) return rc;  // this launch built the jobs
    HIPCHK(e, hipStreamSynchronize(st));
    if (next >= 0) return enqueue_tick(e, next, true);
    return KWOK_OK;
}

// single rank: the kernel publishes the tick's field totals (TickHdr::tot); the
// counts, output layout and counters follow from them
void derive_header(TickHdr& H, uint64_t arena_cap, uint32_t hb_stride, bool hb_once) {
    const uint64_t* t = H.tot;
    H.n_hb = (uint32_t)t[AG_HB];
    H.n_init = (uint32_t)t[AG_INIT];
    H.n_pp = (uint32_t)t[AG_PP];
    H.n_del = (uint32_t)t[AG_DEL];
    H.n_use = 0;
    H.n_rel = (uint32_t)t[AG_REL];
    H.n_alloc_local = (uint32_t)t[AG_ALLOC];
    H.n_eval = (uint32_t)t[AG_EVAL];
    H.n_lock = (uint32_t)t[AG_LOCK];
    H.init_bytes = t[AG_INIT_BYTES];
    H.pp_bytes = t[AG_PP_BYTES];
    H.hb_base = 0;
    H.init_base = (uint64_t)(hb_once ? std::min<uint32_t>(H.n_hb, 1u) : H.n_hb) * hb_stride;
    H.pod_base = H.init_base + H.init_bytes;
    H.arena_bytes = H.pod_base + H.pp_bytes;
    H.overflow = H.arena_bytes > arena_cap;
    const int map[13] = {AG_HB, AG_INIT, AG_PP, AG_DEL, AG_ALLOC, AG_REL, AG_EVAL,
                         AG_LOCK, AG_MANAGED, AG_READY, AG_TOTAL, AG_PENDING, AG_RUNNING};
    for (int k = 0; k < 16; k++) H.local_counters[k] = H.counters[k] = k < 13 ? t[map[k]] : 0;
    H.alloc_total = t[AG_ALLOC];
    H.alloc_base = 0;
    H.rel_total = t[AG_REL];
}

bool trace_enabled(const kwok_engine* e) { return e->S.trace != nullptr; }

// KWOK_JOBS_TRACE=file: the k_pod_jobs wave stamps of the last tick with pod jobs
// (tools/jobs_trace.py reads them), zeroed for the next
void jobs_trace_dump(kwok_engine* e) {
    const size_t n = (size_t)e->S.n_chain * (MAX_WC + 4) * 4;
    std::vector<uint64_t> h(n);
    if (hipMemcpy(h.data(), e->S.jtrace, n * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemset(e->S.jtrace, 0, n * 8) != hipSuccess)
        return;
    if (FILE* f = fopen(getenv("KWOK_JOBS_TRACE"), "wb")) {
        fwrite(h.data(), 8, n, f);
        fclose(f);
    }
}

// per stamp k: earliest / median / latest block, microseconds after the earliest block start
void trace_tick(kwok_engine* e) {
    // (the rows allocated: k_once_stream and k_hb_stream run up to two streamer blocks per CU)
    const size_t G = e->S.n_chain, N = G + std::max(2 * e->n_stream, e->n_once_stream);
    static const int skip = getenv("KWOK_TICK_TRACE_SKIP") ? atoi(getenv("KWOK_TICK_TRACE_SKIP")) : 5;
    static const uint64_t only = getenv("KWOK_TICK_TRACE_COUNT") ? strtoull(getenv("KWOK_TICK_TRACE_COUNT"), nullptr, 10) : 0;
    if ((int)++e->trace_seen <= skip) {  // skip the initial (bulk) ticks; their stamps go (not every kernel writes every row)
        (void)hipMemsetAsync(e->S.trace, 0, N * TRACE_SLOTS * 8, e->st);
        return;
    }
    if (only && e->trace_ticks >= only) return;  // KWOK_TICK_TRACE_COUNT: summarise only the first traced ticks
    const size_t TS = TRACE_SLOTS;
    e->trace_h.assign(N * TS, 0);
    if (release_for_host(e) || hipMemcpyAsync(e->trace_h.data(), e->S.trace, N * TS * 8, hipMemcpyDeviceToHost, e->st) != hipSuccess ||
        hipMemsetAsync(e->S.trace, 0, N * TS * 8, e->st) != hipSuccess || hipStreamSynchronize(e->st) != hipSuccess)
        return;
    uint64_t t0 = ~0ull;
    for (size_t b = 0; b < G; b++) t0 = std::min(t0, e->trace_h[b * TS]);
    if (t0 == 0) {  // no chain or counting block ran (k_hb_stream): after the first streamer's start
        t0 = ~0ull;
        for (size_t b = G; b < N; b++)
            if (e->trace_h[b * TS]) t0 = std::min(t0, e->trace_h[b * TS]);
    }
    // stamps a block did not reach this tick (a clean block skips the pool phase) are 0
    auto summarise = [&](size_t lo, size_t hi, int k, double* out) {
        std::vector<double> v;
        for (size_t b = lo; b < hi; b++)
            if (e->trace_h[b * TS + k] >= t0) v.push_back((double)(e->trace_h[b * TS + k] - t0) * 0.01);
        if (v.empty()) return;
        std::sort(v.begin(), v.end());
        out[0] += v[0];
        out[1] += v[v.size() / 2];
        out[2] += v[v.size() - 1];
    };
    for (int k = 0; k < TRACE_SLOTS; k++) summarise(0, G, k, e->trace_sum[k]);
    summarise(G, N, 0, e->trace_sum[TRACE_SLOTS]);
    summarise(G, N, 6, e->trace_sum[TRACE_SLOTS + 1]);
    if (getenv("KWOK_TICK_TRACE_SLOW")) {  // per XCC: median / max pods-done and arrival; the slowest blocks
        std::vector<double> pd[16], ar[16];
        std::vector<std::pair<double, size_t>> slow;
        for (size_t b = 0; b < G; b++) {
            const uint64_t* T = &e->trace_h[b * TS];
            if (T[2] < t0 || T[3] < t0) continue;
            const uint32_t x = (uint32_t)(T[21] >> 28) & 15u;
            pd[x].push_back((double)(T[2] - t0) * 0.01);
            ar[x].push_back((double)(T[3] - t0) * 0.01);
            slow.emplace_back((double)(T[3] - t0) * 0.01, b);
        }
        for (int x = 0; x < 16; x++) {
            if (pd[x].empty()) continue;
            std::sort(pd[x].begin(), pd[x].end());
            std::sort(ar[x].begin(), ar[x].end());
            fprintf(stderr, "[kwok trace xcc %d] blocks %zu pods-done %.1f / %.1f arrived %.1f / %.1f\n", x, pd[x].size(),
                    pd[x][pd[x].size() / 2], pd[x].back(), ar[x][ar[x].size() / 2], ar[x].back());
        }
        std::sort(slow.rbegin(), slow.rend());
        for (size_t q = 0; q < std::min<size_t>(8, slow.size()); q++) {
            const uint64_t* T = &e->trace_h[slow[q].second * TS];
            fprintf(stderr, "[kwok trace slow] block %zu hw %08llx nodes %.1f pods %.1f sum %.1f drained %.1f arrived %.1f\n",
                    slow[q].second, (unsigned long long)T[21], (double)(T[1] - t0) * 0.01, (double)(T[2] - t0) * 0.01,
                    (double)(T[10] - t0) * 0.01, (double)(T[11] - t0) * 0.01, (double)(T[3] - t0) * 0.01);
        }
    }
    if (getenv("KWOK_TICK_TRACE_RAW")) {  // the last block's 16 stamps (ad-hoc kernel probes), us after t0
        fprintf(stderr, "[kwok trace raw]");
        for (size_t k = 0; k < TS; k++) {
            const uint64_t v = e->trace_h[(N - 1) * TS + k];
            fprintf(stderr, " %.3f", k == 8 ? (double)v : v >= t0 ? (double)(v - t0) * 0.01 : -1.0);
        }
        fprintf(stderr, "\n");
    }
    e->trace_ticks++;
}

// k_once met work to emit in slot k's tick (a delete, patch, Get, Put, Use, pod
// event or node init): run the tick again with k_tick (same tag and arrival
// target: k_once made no arrivals).  The launch queued behind it skipped on the
// device (GridBar::skip); retire enqueues it again afterwards.
int redo_tick(kwok_engine* e, int k) {
    kwok_engine::TickSlot& T = e->slots[k];
    e->stats[KWOK_STAT_ONCE_REDO]++;
    e->state_changed();
    memset(T.hdr_h, 0, sizeof(TickHdr));
    HIPCHK(e, hipMemsetAsync(&e->S.bar->skip, 0, sizeof(uint32_t), e->st));
    T.no_once = true;
    if (int rc = enqueue_tick(e, k, true)) return rc;
    HIPCHK(e, hipEventSynchronize(T.done));
    return KWOK_OK;
}

// Finish the oldest queued tick on the host: wait for it, complete a multi-rank
// tick with long lists, derive the header, check errors, mirror DeletePods into
// the host slot state.  The result stays in the slot until kwok_tick_collect.
int retire(kwok_engine* e) {
    int qi = -1;
    for (int i = 0; i < e->nq; i++)
        if (e->slots[e->queue[i]].state == SLOT_QUEUED) {
            qi = i;
            break;
        }
    if (qi < 0) return KWOK_OK;
    const int k = e->queue[qi];
    const int next = qi + 1 < e->nq ? e->queue[qi + 1] : -1;  // a tick queued behind this one
    kwok_engine::TickSlot& T = e->slots[k];
    T.state = SLOT_DONE;
    T.rc = KWOK_OK;
    // every failure here leaves the device state (advanced by the kernels) and the
    // host mirrors / the caller's view out of step: the engine is poisoned, and a
    // tick queued behind this one (it ran on that state) fails with it
    auto failed = [&](int rc) {
        T.rc = rc;
        T.err = e->err;
        e->poisoned = true;
        if (next >= 0 && e->slots[next].state == SLOT_QUEUED) {
            kwok_engine::TickSlot& U = e->slots[next];
            (void)hipStreamSynchronize(e->st);
            U.state = SLOT_DONE;
            U.rc = rc;
            U.err = e->err;
        }
        return rc;
    };
    const auto t1 = clk::now();
    if (e->sync_spin) {
        // spin on the tick's completion event: a blocking wait sleeps and pays the
        // wake-up latency on every tick
        hipError_t q;
        while ((q = hipEventQuery(T.done)) == hipErrorNotReady) {
        }
        if (q != hipSuccess) return failed(e->fail(KWOK_EDEVICE, "tick: %s", hipGetErrorString(q)));
    } else if (hipEventSynchronize(T.done) != hipSuccess) {
        return failed(e->fail(KWOK_EDEVICE, "tick event sync"));
    }
    if (e->multi && T.hdr_h->xovf) {
        int rc = finish_long_lists(e, k, next);
        if (rc) return failed(rc);
    }
    if (e->multi && T.hdr_h->xforeign) e->global_foreign = true;  // (the BACK launch that ran to the end)
    bool requeue_next = false;
    // a reused count: the totals the clean count published (k_hb_stream writes no header;
    // a launch that skipped on the device was enqueued again as a counting tick)
    if (T.count_reused) memcpy(T.hdr_h->tot, e->clean_count.tot, sizeof(T.hdr_h->tot));
    if (T.once && T.hdr_h->redo) {
        if (int rc = redo_tick(e, k)) return failed(rc);
        requeue_next = next >= 0 && e->slots[next].state == SLOT_QUEUED;
    }
    const auto t2 = clk::now();
    if (!e->multi) derive_header(*T.hdr_h, T.arena_cap, e->hb_stride, e->S.hb_once != 0);
    const TickHdr& H = *T.hdr_h;
    if (!H.err && (H.n_pp || H.n_init) && !T.emit_queued) {
        // jobs nobody expected (no events since the previous tick): their bytes now
        int rc = bind_slot(e, k);
        if (!rc) rc = enqueue_emit(e, k);
        if (rc) return failed(rc);
        if (hipEventRecord(T.done, e->st) != hipSuccess || hipEventSynchronize(T.done) != hipSuccess)
            return failed(e->fail(KWOK_EDEVICE, "k_emit"));
    }
    if (trace_enabled(e)) trace_tick(e);
    if (e->S.jtrace && H.n_pp) jobs_trace_dump(e);
    if (H.err) {
        const uint32_t err = H.err;
        // a tick queued behind a failed one ran on its state: fail it as well
        (void)hipStreamSynchronize(e->st);
        (void)hipMemsetAsync(e->S.bar, 0, sizeof(GridBar), e->st);  // the next tick starts from a clean count
        (void)hipStreamSynchronize(e->st);
        e->front_launches = 0;
        int rc = (err & TICK_ERR_BARRIER)
                     ? e->fail(KWOK_EDEVICE, "k_tick cross-block wait timed out (%u chain blocks not co-resident?)",
                               e->S.n_chain)
                 : (err & TICK_ERR_SEQ)
                     ? e->fail(KWOK_ECOMM, "ranks out of step: the gathered exchange messages are of different ticks")
                 : (err & TICK_ERR_EMIT)
                     ? e->fail(KWOK_EDEVICE, "k_pod_jobs: a pod spec without unit tables in a fused emission")
                     : e->fail(KWOK_EDEVICE, "k_tick: device heartbeat count differs from the host's (%llu)",
                               (unsigned long long)e->n_managed);
        e->poisoned = true;
        if (next >= 0) {
            kwok_engine::TickSlot& U = e->slots[next];
            U.state = SLOT_DONE;
            U.rc = rc;
            U.err = e->err;
        }
        return failed(rc);
    }
    if (e->prof) {
        // kernel time from the launch events; the phase split from the kernel's
        // s_memrealtime stamps (100 MHz)
        float k0 = 0, k1 = 0;
        (void)hipEventElapsedTime(&k0, T.pev[0], T.pev[1]);
        if (e->multi) (void)hipEventElapsedTime(&k1, T.pev[2], T.pev[3]);
        float k2 = 0;
        if (T.emit_queued && !T.inits_folded) (void)hipEventElapsedTime(&k2, T.pev[4], T.pev[5]);
        float k3 = 0;
        if (T.split) (void)hipEventElapsedTime(&k3, T.pev[6], T.pev[7]);
        const double kern = (double)k0 + k1 + k2 + k3;
        // the streamers' latest exit, kept on the device (they never touch the header)
        unsigned long long send = 0;
        (void)release_for_host(e);
        (void)hipMemcpyAsync(&send, &e->S.bar->stream_end_max, 8, hipMemcpyDeviceToHost, e->st);
        (void)hipMemsetAsync(&e->S.bar->stream_end_max, 0, 8, e->st);
        unsigned long long nent = 0;  // (k_hb_stream: no counting block publishes the earliest entry)
        if (T.count_reused) {
            (void)hipMemcpyAsync(&nent, &e->S.bar->neg_entry_max, 8, hipMemcpyDeviceToHost, e->st);
            (void)hipMemsetAsync(&e->S.bar->neg_entry_max, 0, 8, e->st);
        }
        (void)hipStreamSynchronize(e->st);
        T.hdr_h->clk[CLK_STREAM_END] = send;
        if (T.count_reused) T.hdr_h->clk[CLK_ENTRY_MIN] = ~nent;
        auto span = [&](int a, int b) { return H.clk[b] > H.clk[a] ? (double)(H.clk[b] - H.clk[a]) * 1e-5 : 0.0; };
        const double classify = span(CLK_ENTRY_MIN, CLK_P1_MAX), stream = span(CLK_ENTRY_MIN, CLK_STREAM_END);
        const double header = span(CLK_P1_MAX, CLK_HDR), pool = span(CLK_BACK, CLK_POOL);
        e->prof_ms[KWOK_T_CLASSIFY] += classify;
        e->prof_ms[KWOK_T_STREAM] += stream;
        e->prof_ms[KWOK_T_HEADER] += header;
        e->prof_ms[KWOK_T_EXCHANGE] += e->multi ? span(CLK_HDR, CLK_BACK) : 0.0;
        e->prof_ms[KWOK_T_POOL] += pool;
        // what follows the header in the chain (pool, job lists) beyond the stream, and k_emit
        e->prof_ms[KWOK_T_EMIT] += std::max(0.0, k0 + k1 - std::max(classify + header + pool, stream)) + k2 + k3;
        e->prof_ms[KWOK_T_KERNEL] += kern;
        e->prof_ms[KWOK_T_EMIT_KERNEL] += k2 + k3;  // k_emit and k_pod_jobs (split ticks)
        e->prof_ticks++;
    }
    if (H.overflow) return failed(e->fail(KWOK_ENOMEM, "output arena overflow (%llu bytes)", (unsigned long long)H.arena_bytes));
    // deleted nodes (and placeholders) whose last pod this tick deleted: their
    // entries go (k_free_zombies, queued on the engine stream: a tick already
    // queued behind this one reads no such node; every ingest follows it)
    if (H.n_del) {
        e->state_changed();
        launch_free_zombies(e->S, e->st);
        if (hipGetLastError() != hipSuccess) return failed(e->fail(KWOK_EDEVICE, "k_free_zombies"));
    }
    kwok_tick_result& r = T.res;
    memset(&r, 0, sizeof(r));
    r.n_heartbeat = H.n_hb;
    r.heartbeat_len = e->hb_len;
    r.heartbeat_stride = e->S.hb_once ? 0 : e->hb_stride;
    r.n_node_init = H.n_init;
    r.n_pod_patch = H.n_pp;
    r.n_delete = H.n_del;
    r.heartbeat_epoch = T.epoch;
    r.arena_bytes = H.arena_bytes;
    for (int c = 0; c < KWOK_COUNTER_COUNT; c++) {
        r.counters[c] = H.counters[c];
        r.local_counters[c] = H.local_counters[c];
    }
    const auto t3 = clk::now();
    if (e->iprof && (H.n_pp || H.n_del || H.n_init))
        fprintf(stderr, "[kwok retire] wait %.3f ms, post %.3f ms\n", ms_between(t1, t2), ms_between(t2, t3));
    e->host_ms[KWOK_H_WAIT] += ms_between(t1, t2);
    e->host_ms[KWOK_H_POST] += ms_between(t2, t3);
    e->host_ms[KWOK_H_TOTAL] += ms_between(t1, t3);
    e->host_ticks++;
    e->stats[T.once && !T.once_stream ? KWOK_STAT_TICKS_ONCE : KWOK_STAT_TICKS_FULL]++;
    if (T.once_stream) e->stats[KWOK_STAT_TICKS_ONCE_STREAM]++;
    if (T.count_reused) e->stats[KWOK_STAT_TICKS_COUNT_REUSED]++;
    // a k_once_stream tick that completed cleanly (no error or overflow: returned above; not
    // redone, not requeued after a device skip): its count is the engine's clean count, and the
    // slot's handle list is that count's, as is a reused tick's (nothing wrote it)
    if (T.once_stream && !T.requeued && !T.no_once) {
        if (!T.count_reused) {
            e->clean_count.ok = true;
            e->clean_count.gen = T.state_gen;
            memcpy(e->clean_count.tot, H.tot, sizeof(H.tot));
        }
        kwok_engine::TickSlot::ListValid& L = T.list_valid;
        L.list = T.hb_nodes, L.n = H.n_hb, L.gen = T.state_gen;
        L.ok = true;
    }
    e->pp_followup = !e->S.cni && H.n_pp != H.n_alloc_local;
    // the slot's heartbeat region now holds this tick's bodies (TickSlot::HbValid); a
    // tick that was redone records nothing (hb_record: no heartbeat-once engine, no requeue)
    if (T.hb_record && !T.no_once) {
        kwok_engine::TickSlot::HbValid& V = T.hb_valid;
        V.arena = T.arena, V.n = T.hb_n, V.stride = e->hb_stride, V.units = e->S.hb_units, V.gen = e->hb_gen;
        V.clock = T.now;
        V.ok = true;
    }
    if (T.hb_prev) e->stats[KWOK_STAT_TICKS_HB_DELTA]++;
    if (T.once && T.once_use) e->stats[KWOK_STAT_ONCE_SUMMARY]++;  // (a launch that skipped or was redone read none)
    if (requeue_next) {  // the tick queued behind a redone one skipped on the device
        if (int rc = enqueue_tick(e, next, true)) {
            kwok_engine::TickSlot& U = e->slots[next];
            U.state = SLOT_DONE;
            U.rc = rc;
            U.err = e->err;
            e->poisoned = true;
        }
    }
    return KWOK_OK;
}

}  // namespace

namespace kwok {
// every queued tick finished on the host (before anything that reads or changes
// the host mirrors or device state outside the tick stream)
int drain(kwok_engine* e) {
    for (int i = 0; i < e->nq; i++)
        if (e->slots[e->queue[i]].state == SLOT_QUEUED) retire(e);  // per-tick failures stay in the slots
    return KWOK_OK;
}

// what kwok_tick_submit checks before it queues anything
int tick_submit_check(kwok_engine* e, int64_t now_unix) {
    if (now_unix < 0 || now_unix > 0xFFFFFFFFll) return e->fail(KWOK_EDOMAIN, "now out of range");
    if (e->nq >= 2) return e->fail(KWOK_EBUSY, "two ticks outstanding: collect one first");
    if (e->nq >= 1 && (e->prof || trace_enabled(e)))
        return e->fail(KWOK_EBUSY, "profiled / traced ticks are not queued behind each other");
    return KWOK_OK;
}
}  // namespace kwok

extern "C" int kwok_tick_submit(kwok_engine* e, int64_t now_unix) {
    if (!e) return KWOK_EINVAL;
    if (e->poisoned) return poisoned(e);
    if (int rc = tick_submit_check(e, now_unix)) return rc;
    return tick_submit_impl(e, now_unix);
}

namespace kwok {
// kwok_tick_submit after its checks (kwok_ingest_pods_packed12_tick queues it
// behind the batch's apply passes)
int tick_submit_impl(kwok_engine* e, int64_t now_unix) {
    const auto t0 = clk::now();
    // multi rank: the previous tick is finished (its long-list allgather, if any,
    // included) before this one's collectives are enqueued, so every rank issues
    // its collectives in the same order whatever its submit / collect pattern
    if (e->multi) drain(e);
    if (e->poisoned) return poisoned(e);  // the drained tick failed (its error stays collectable)
    const auto t_drained = clk::now();
    int k = -1;
    for (int pass = 0; pass < 2 && k < 0; pass++)  // prefer keeping the last collected tick's outputs
        for (int i = 0; i < 2 && k < 0; i++)
            if (e->slots[i].alloc && e->slots[i].state == SLOT_FREE && (pass == 1 || i != e->cur)) k = i;
    if (k < 0) {
        int rc = alloc_slot(e, 1);
        if (rc) return rc;
        k = 1;
    }
    kwok_engine::TickSlot& T = e->slots[k];
    int rc = grow_arena(e, T);
    if (rc) return rc;
    if (T.rd_pending) {  // the tick's kernels write the arena after the reads queued from it
        HIPCHK(e, hipStreamWaitEvent(e->st, T.rd, 0));
        T.rd_pending = false;
    }
    if (k == e->cur) e->cur = -1;  // its outputs are overwritten
    T.now = (uint64_t)now_unix;
    T.epoch = e->hb_epoch;
    T.ref_gen[0] = e->refs.gen[0], T.ref_gen[1] = e->refs.gen[1];
    T.emit_queued = e->emit_hint;
    e->emit_hint = false;
    // multi rank: every rank's pods hold the addresses the global pool gave them
    // unless some rank ever took a foreign one - its flag travels in the exchange
    // message; a rank that became foreign since the last exchange cannot make a
    // Use of this tick a change (its Puts come after the Uses, its ingest-time
    // releases reach the others through kwok_pool_put, which marks them foreign)
    T.quiet = e->quiet_ok && (e->multi ? !e->foreign_ips && !e->global_foreign : (e->quiet >= 2 || !e->foreign_ips));
    if (e->quiet < 0xFFFFFFFFu) e->quiet++;
    rc = enqueue_tick(e, k, false);
    if (rc) return rc;
    T.state = SLOT_QUEUED;
    e->queue[e->nq++] = k;
    if (e->iprof)
        fprintf(stderr, "[kwok submit] enqueue %.3f ms (drain %.3f)\n", ms_between(t0, clk::now()), ms_between(t0, t_drained));
    e->host_ms[KWOK_H_ENQUEUE] += ms_between(t0, clk::now());
    e->host_ms[KWOK_H_TOTAL] += ms_between(t0, clk::now());
    return KWOK_OK;
}
}  // namespace kwok

extern "C" int kwok_engine_stats(const kwok_engine* e, uint64_t out[KWOK_STAT_COUNT]) {
    if (!e || !out) return KWOK_EINVAL;
    for (int i = 0; i < KWOK_STAT_COUNT; i++) out[i] = e->stats[i];
    return KWOK_OK;
}

extern "C" int kwok_tick_collect(kwok_engine* e, kwok_tick_result* res) {
    if (!e) return KWOK_EINVAL;
    if (e->nq == 0) return e->fail(KWOK_EINVAL, "no tick submitted");
    const int k = e->queue[0];
    kwok_engine::TickSlot& T = e->slots[k];
    if (T.state == SLOT_QUEUED) retire(e);
    e->queue[0] = e->queue[1];
    e->queue[1] = -1;
    e->nq--;
    T.state = SLOT_FREE;
    if (T.rc) {
        e->err = T.err;
        return T.rc;
    }
    e->cur = k;
    if (res) *res = T.res;
    return KWOK_OK;
}

extern "C" int kwok_tick(kwok_engine* e, int64_t now_unix, kwok_tick_result* res) {
    if (!e) return KWOK_EINVAL;
    if (e->nq) return e->fail(KWOK_EBUSY, "ticks outstanding: kwok_tick_collect them first");
    int rc = kwok_tick_submit(e, now_unix);
    return rc ? rc : kwok_tick_collect(e, res);
}
