// The body of the counting kernels (k_once, and the counting blocks of
// k_once_stream), included into each of them: as a function inlined into the two
// it compiles to other code than in place (k_once<false, ONCE_SUM_USE>: 118 -> 165
// VGPRs, one block per CU instead of two), so the text is shared instead.
// In scope at the include: the kernel's S, now_unix, start_unix, n_hb, phases, gen and
// CNI, SUM; ONCE_B / ONCE_G: this block's index among the counting blocks and their
// number; ONCE_BODY: the block also writes the one body of a heartbeat-once engine.
// A launch that skips returns from the kernel.
    __shared__ uint32_t nfl32[ONCE_WAVES][ONCE_NODE_LDS / 4];  // the bucket's node tick flags, per wave
    __shared__ uint64_t part[ONCE_WAVES][ONCE_ACC_WORDS];
    const uint32_t t = threadIdx.x, l = t & 63u, w = (uint32_t)wave_id(), b = ONCE_B;
    if (ld32_sc1(&S.bar->skip)) return;  // queued behind a tick the host must finish (re-enqueued then)
    const bool stamp = S.trace && t == 0 && b < S.n_chain;
#define OSTAMP(k) \
    if (stamp) S.trace[(size_t)b * TRACE_SLOTS + (k)] = __builtin_amdgcn_s_memrealtime()
    OSTAMP(0);
    // profiled ticks: the earliest start, from the first block of each XCD (512 adds to one
    // word would serialise ~6 us into the kernel)
    if ((phases & TICK_PROF) && t == 0 && b < 8u)
        atomicMax(&S.bar->neg_entry_max, ~(unsigned long long)__builtin_amdgcn_s_memrealtime());
    const uint32_t bk = b * ONCE_WAVES + w;
    uint32_t hb = 0, lock = 0, mng = 0, rdy = 0, ev = 0, tot = 0, pnd = 0, run = 0, rare = 0;
    uint32_t be0 = 0, be1 = 0, br0 = 0, br1 = 0;  // SUM == ONCE_SUM_BUILD: eval / rare under both uniform flags
    if (bk < S.nb) {  // (wave-uniform)
        const uint32_t cn = S.cn, cp = S.cp;
        const uint32_t fill = min((uint32_t)S.pod_fill[bk], cp);
        // ---- every load of the bucket: node bytes first (classified first), pod state rows
        const uint8_t* nst = S.node_state + (size_t)bk * cn;
        uint32_t nw[ONCE_NODE_WORDS];
#pragma unroll
        for (int c = 0; c < ONCE_NODE_WORDS; c++) {
            const uint32_t i = 4u * (l + 64u * c);
            nw[c] = 0;
            if (256u * c < cn && i < cn) nw[c] = *reinterpret_cast<const uint32_t*>(nst + i);
        }
        const uint16_t* pst = S.pod_state + (size_t)bk * cp;
        constexpr bool use = SUM == ONCE_SUM_USE;
        uint4 sm = make_uint4(0, 0, 0, 0), st[ONCE_ROWS];
        if (use) sm = S.once_sum[bk];  // (one address: one request)
#pragma unroll
        for (int r = 0; r < ONCE_ROWS; r++) {
            const uint32_t g8 = 8u * (l + 64u * r);
            st[r] = make_uint4(0, 0, 0, 0);
            if (!use && g8 < (r < ONCE_SPEC_ROWS ? cp : fill)) st[r] = *reinterpret_cast<const uint4*>(pst + g8);
        }
        // ---- nodes: LockNode / configureNode (A.5), heartbeat handles, re-lock flags
        uint32_t or0 = 0, and0 = 1, has = 0, base = S.hb_bpre[bk];
#pragma unroll
        for (int c = 0; c < ONCE_NODE_WORDS; c++) {
            if (256u * c < cn) {  // (uniform)
                const uint32_t word = nw[c], i0 = 4u * (l + 64u * c);
                uint32_t tickw = 0, m = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint8_t s = (uint8_t)(word >> (8 * k));
                    const NodeCls nc = classify_node(s);
                    hb += nc.hb;
                    lock += nc.lock;
                    mng += nc.managed;
                    rdy += nc.ready;
                    rare |= (nc.init || (s & NS_EVENT_LOCK)) ? 1u : 0u;
                    const uint32_t f = node_tick_flags(s);
                    tickw |= f << (8 * k);
                    if (s) or0 |= f & 1u, and0 &= f & 1u, has = 1;
                    m += (uint32_t)nc.managed << k;
                }
                if (i0 < cn) nfl32[w][l + 64u * c] = tickw;
                // KeepNodeHeartbeat's handles, node order: the wave's managed nodes of this word
                const uint32_t cnt = (uint32_t)__popc(m), inc = wave_incl_scan(cnt);
                uint32_t pos = base + inc - cnt;
                for (uint32_t mm = m; mm; mm &= mm - 1) {
                    if (pos < S.n_node_slots)
                        S.hb_nodes[pos] = S.node_handle_base + (int32_t)((size_t)bk * cn + i0 + (uint32_t)__builtin_ctz(mm));
                    pos++;
                }
                base += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
            }
        }
        // a pod's node matters only if the bucket's node entries disagree on RELOCK
        const bool any_set = __ballot(has && or0) != 0, any_clr = __ballot(has && !and0) != 0;
        const bool uni = !(any_set && any_clr);
        const uint8_t u = any_set ? (uint8_t)NT_RELOCK : (uint8_t)0;
        OSTAMP(8);
        const uint16_t* pnd_ = S.pod_node + (size_t)bk * cp;
        // ---- pods: needLockPod / computePatchData, counted (once_group)
        auto count_row = [&](uint32_t g8, const uint4& s4, const uint32_t (&rl)[4]) {
            const bool in = g8 < fill;
            const uint32_t stw[4] = {in ? s4.x : 0u, in ? s4.y : 0u, in ? s4.z : 0u, in ? s4.w : 0u};
            rare |= once_group<CNI>(stw, rl, ev, tot, pnd, run);
            if constexpr (SUM == ONCE_SUM_BUILD) once_group_both<CNI>(stw, be0, be1, br0, br1);
        };
        auto lds_flags = [&](const uint4& n4, uint32_t (&rl)[4]) {
            const uint8_t* nfw = reinterpret_cast<const uint8_t*>(nfl32[w]);
            const uint32_t q[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t a = nfw[min(q[k] & 0xFFFFu, (uint32_t)ONCE_NODE_LDS - 1u)];
                const uint32_t c = nfw[min(q[k] >> 16, (uint32_t)ONCE_NODE_LDS - 1u)];
                rl[k] = a | c << 16;  // (NT_RELOCK is bit 0)
            }
        };
        if (use && uni && sm.w == gen) {  // the bucket's summary (lane 0's counts; rare from any lane)
            if (l == 0) {
                ev += u ? sm.x >> 16 : sm.x & 0xFFFFu;
                tot += sm.y & 0xFFFFu, pnd += sm.y >> 16, run += sm.z & 0xFFFFu;
            }
            rare |= (sm.z >> (u ? 17 : 16)) & 1u;
        } else if (uni) {
            if (use) {  // (another generation: the rows now)
#pragma unroll
                for (int r = 0; r < ONCE_ROWS; r++) {
                    const uint32_t g8 = 8u * (l + 64u * r);
                    if (g8 < fill) st[r] = *reinterpret_cast<const uint4*>(pst + g8);
                }
            }
            const uint32_t p = u ? 0x00010001u : 0u;
            const uint32_t rl[4] = {p, p, p, p};
#pragma unroll
            for (int r = 0; r < ONCE_ROWS; r++) count_row(8u * (l + 64u * r), st[r], rl);
            for (uint32_t r = ONCE_ROWS; 512u * r < fill; r++) {  // buckets of more than 4096 pod slots
                const uint32_t g8 = 8u * (l + 64u * r);
                const uint4 s4 = g8 < fill ? *reinterpret_cast<const uint4*>(pst + g8) : make_uint4(0, 0, 0, 0);
                count_row(g8, s4, rl);
            }
        } else {
            uint4 nd[ONCE_ROWS];
#pragma unroll
            for (int r = 0; r < ONCE_ROWS; r++) {
                const uint32_t g8 = 8u * (l + 64u * r);
                nd[r] = g8 < fill ? *reinterpret_cast<const uint4*>(pnd_ + g8) : make_uint4(0, 0, 0, 0);
                if (use && g8 < fill) st[r] = *reinterpret_cast<const uint4*>(pst + g8);
            }
            __builtin_amdgcn_wave_barrier();  // (the wave's node flags are in LDS)
#pragma unroll
            for (int r = 0; r < ONCE_ROWS; r++) {
                uint32_t rl[4];
                lds_flags(nd[r], rl);
                count_row(8u * (l + 64u * r), st[r], rl);
            }
            for (uint32_t r = ONCE_ROWS; 512u * r < fill; r++) {
                const uint32_t g8 = 8u * (l + 64u * r);
                uint4 s4 = make_uint4(0, 0, 0, 0), n4 = s4;
                if (g8 < fill) {
                    s4 = *reinterpret_cast<const uint4*>(pst + g8);
                    n4 = *reinterpret_cast<const uint4*>(pnd_ + g8);
                }
                uint32_t rl[4];
                lds_flags(n4, rl);
                count_row(g8, s4, rl);
            }
        }
        OSTAMP(2);
    }
    // ---- counts: wave -> block -> XCD shard -> fleet
    auto wsum = [](uint32_t x) { return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan(x), 63); };
    {
        const uint64_t v0 = wsum(hb) | wsum(lock) << ONCE_FIELD_BITS, v1 = wsum(mng) | wsum(rdy) << ONCE_FIELD_BITS;
        const uint64_t v2 = wsum(ev) | wsum(tot) << ONCE_FIELD_BITS, v3 = wsum(pnd) | wsum(run) << ONCE_FIELD_BITS;
        const uint64_t v4 = __ballot(rare != 0) ? 1u : 0u;
        if (l == 0) part[w][0] = v0, part[w][1] = v1, part[w][2] = v2, part[w][3] = v3, part[w][4] = v4;
        if constexpr (SUM == ONCE_SUM_BUILD) {  // the bucket's summary (one wave = one bucket)
            const uint32_t E0 = (uint32_t)wsum(be0), E1 = (uint32_t)wsum(be1);
            const uint32_t k0 = __ballot(br0 != 0) ? 1u : 0u, k1 = __ballot(br1 != 0) ? 1u : 0u;
            if (l == 0 && bk < S.nb)
                S.once_sum[bk] = make_uint4(E0 | E1 << 16, (uint32_t)(v2 >> ONCE_FIELD_BITS) | (uint32_t)(v3 & ONCE_M27) << 16,
                                            (uint32_t)(v3 >> ONCE_FIELD_BITS) | k0 << 16 | k1 << 17, gen);
        }
    }
    __syncthreads();
    if (t < (uint32_t)ONCE_ACC_WORDS) {
        uint64_t v = 0;
#pragma unroll
        for (int i = 0; i < ONCE_WAVES; i++) v += part[i][t];
        const uint32_t G = ONCE_G, x = b & 7u, nsh = min(G, 8u), nx = (G - x + 7u) / 8u;
        const unsigned long long old = atomicAdd(&S.bar->once_acc[x][t][0], (1ull << ACC_SHIFT) | v);
        if ((old >> ACC_SHIFT) == nx - 1u) {  // the shard is complete
            const uint64_t sx = (old & ACC_MASK) + v;
            st_sc1(&S.bar->once_acc[x][t][0], 0ull);  // the next tick starts from zero
            const unsigned long long o2 = atomicAdd(&S.bar->once_acc[8][t][0], (1ull << ACC_SHIFT) | sx);
            if ((o2 >> ACC_SHIFT) == nsh - 1u) {
                st_sc1(&S.bar->once_acc[8][t][0], 0ull);
                once_publish(S, t, (o2 & ACC_MASK) + sx, n_hb, phases, __builtin_amdgcn_s_memrealtime());
            }
        }
    }
    OSTAMP(3);
    // ---- the one heartbeat body (hb_bodies), arena offset 0
    if constexpr (ONCE_BODY) {
    __shared__ uint8_t tmpl[16 * HB_MAX_UNITS];
    if (b == 0 && n_hb) {
        const Ts nw = format_ts(now_unix), sw = format_ts(start_unix);
        const uint32_t nb16 = 16u * S.hb_units;
        for (uint32_t i = t; i < nb16; i += 64u * ONCE_WAVES) {
            const uint8_t k = S.hb_kind[i];
            tmpl[i] = (uint8_t)(k == 0xFF ? S.hb_static[i] : k < TS_LEN ? ts_byte(nw, k) : ts_byte(sw, k - TS_LEN));
        }
        __syncthreads();
        for (uint32_t i = t; i < S.hb_units; i += 64u * ONCE_WAVES)
            reinterpret_cast<uint4*>(S.arena)[i] = reinterpret_cast<const uint4*>(tmpl)[i];
    }
    }
    OSTAMP(6);
#undef OSTAMP
