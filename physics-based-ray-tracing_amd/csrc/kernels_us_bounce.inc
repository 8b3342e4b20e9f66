// kernels_us_bounce.inc -- the body of the fused ultrasound bounce, included by k_us_bounce and k_us_bounce_convex (kernels_us.h).
// In scope: the kernel's argument `a` and the compile-time switches FIRST, ACCEL, EMIT, Q, TAB, CONVEX.
    const uint32_t quirks = Q == US_Q_RUNTIME ? a.p.quirks : Q;
    const bool have_hit_tab = TAB < 0 ? a.first_hit != nullptr : TAB == 1;
    const bool have_rx_tab = TAB < 0 ? a.first_rx != nullptr : TAB == 1;
    constexpr uint32_t SEG = seg_threads(ACCEL);
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn_lds[];
    __shared__ uint32_t wave_tot[2][SEG / 64];
    __shared__ uint32_t wave_seg[2][SEG / 64];
    constexpr uint32_t REGION = us_region_segs(ACCEL, EMIT) * SEG;
    constexpr bool WP = rad_wave_private(ACCEL);  // BVH scenes: per-wave compaction, no barrier per chunk (see k_bounce)
    constexpr uint32_t W = SEG / 64, WREG = REGION / W, CH = WP ? 64u : SEG;
    // seg: region index (see k_bounce).  Emitter rays: consecutive workgroups take regions a stride apart, so that the workgroups that
    // run -- and flush their echo tables -- side by side do not belong to the same ray (the six regions of a ray's paths land on the
    // same ~10^3 channel words): 20.3 -> 18.4 ms.  Any stride of a ray or more does (7 .. 1229 of 2048 regions: 18.5 - 19.0 ms); the
    // host takes regions / n_angles.  With the integrator's own rays (table-driven first bounce, <= 64 words per ray) it changes nothing
    const uint32_t seg = a.blk_mul ? (uint32_t)(((unsigned long long)blockIdx.x * a.blk_mul) % gridDim.x) : blockIdx.x;
    const uint32_t tid = threadIdx.x;
    const uint32_t lane_c = WP ? (tid & 63u) : tid;
    const uint32_t own = WP ? seg * W + (tid >> 6) : seg;
    const uint32_t base = WP ? seg * REGION + (tid >> 6) * WREG : seg * REGION;
    uint32_t cnt_in = FIRST ? (a.n_paths > base ? min(a.n_paths - base, WP ? WREG : REGION) : 0u) : a.seg_in[own];
    if (WP) {
        cnt_in = (uint32_t)__builtin_amdgcn_readfirstlane((int)cnt_in);
        uint32_t c = 0;
        if ((tid & 63u) < W) {
            const uint32_t b2 = seg * REGION + (tid & 63u) * WREG;
            c = FIRST ? (a.n_paths > b2 ? 1u : 0u) : a.seg_in[seg * W + (tid & 63u)];
        }
        if (__ballot(c != 0) == 0) {  // no wave of the workgroup has work (same answer in every wave)
            if ((tid & 63u) == 0) a.seg_out[own] = 0;
            return;
        }
    } else if (cnt_in == 0) {
        if (tid == 0) a.seg_out[seg] = 0;
        return;
    }
    BVH_STACK_LDS(ACCEL, SEG);
    LdsScene ls = {NO_TREE_LDS, MAKE_BVH_STACK(bvh_stk_lds, SEG)};
    if (ACCEL == ACCEL_K_BVH_LDS) ls.tree = stage_tree_lds(a.sc, dyn_lds);
    __shared__ uint32_t tab_lds[ACCEL == ACCEL_K_BRUTE ? TAB_DW : 1];
    const Tables tb = make_tables<ACCEL>(a.sc, ls, tab_lds);
    constexpr uint32_t AGG_LOG2 = EMIT ? US_AGG_LOG2_EMIT : US_AGG_LOG2;
    __shared__ uint32_t agg_idx[1u << AGG_LOG2];
    __shared__ float agg_sum[1u << AGG_LOG2];
    us_echo_clear(agg_idx, agg_sum, threadIdx.x, blockDim.x);
    __shared__ float uni[U_COUNT];
    us_stage_uniforms(a, uni);
    if (ACCEL == ACCEL_K_BRUTE)
        fill_tables_lds(a.sc, tab_lds, blockDim.x);  // ends with the barrier that also publishes the empty bins
    else
        __syncthreads();
    const uint32_t cap = a.cap;
    const uint32_t NE = a.p.n_elements, T = a.p.time_samples;
    // ALL bounces of a pass run in ONE launch (a.fuse; the FIRST kernel goes on with the later bounces): compaction is
    // local to the region (to the wave for BVH scenes), so the owner carries its survivors from bounce to bounce on its
    // own, ping-ponging between the two state buffers -- no grid-wide barrier per bounce, the survivors are re-read
    // while they are still in L2, and no launches for the bounces that find nothing alive (ultrasound paths die
    // fast: Sphere_Box has 20 % of them left after the first bounce and none after the second; the 8 empty launches up
    // to max_depth cost 5 us each per pass).  Config 3: 10.1 ms with one launch per bounce, 9.1 with bounces >= 1
    // fused, 8.6 with all of them.
    // path state: tiles of 64 slots x 11 rows like the radiance kernels' (kernels_radiance.h state_voff), read and written through
    // buffer descriptors: the row offset k * 256 is an immediate of the instruction, no 64-bit address arithmetic and no
    // pointer pair per array in SGPRs (this kernel spills scalars)
    // (the EMIT instances carry a twelfth row: the weight of the path's primary ray, a factor of every echo it deposits)
    constexpr uint32_t ROWS = EMIT ? US_N_STATE + 1u : US_N_STATE;
    Rsrc r_in = make_rsrc(a.in, cap * (ROWS * 4u)), r_out = make_rsrc(a.out, cap * (ROWS * 4u));
    uint32_t depth = a.depth;
    uint32_t out_off, ns_acc;
    for (;;) {  // bounce loop: a single trip unless a.fuse
    const bool first = FIRST && depth == 0;  // FIRST kernels continue with the later bounces when a.fuse
    out_off = 0;
    ns_acc = 0;
    for (uint32_t it0 = 0; it0 < cnt_in; it0 += CH) {
    const uint32_t buf = (it0 / SEG) & 1u;
    const bool alive = it0 + lane_c < cnt_in;
    const uint32_t slot = base + it0 + lane_c;
    bool survive = false, did_seg = false;
    V3 o, d;
    float amp, atten, tof, geo_len, w_ray = 1.0f;
    uint32_t home = slot;
    if (alive) {
#ifdef PBRT_PROBE_EXTRA_VALU  // diagnostic builds only (see k_bounce)
        {
            float probe = __uint_as_float(slot);
#pragma unroll
            for (int kk = 0; kk < PBRT_PROBE_EXTRA_VALU; ++kk) asm volatile("v_add_f32 %0, %0, %0" : "+v"(probe));
            if (probe == 12345.678f) home = 0;  // never true; keeps the chain alive
        }
#endif
        uint32_t ray_id, k;
        if (first) {
            ray_id = udiv_fast(home, a.div_ppr);
            k = a.path_first + (home - ray_id * a.ppr_pass);
            const uint32_t ang = udiv_fast(ray_id, a.div_ne), el = ray_id - ang * NE;
            o = us_elem_point<CONVEX>(a, uni, el);                     // :270,273
            d = v3(a.dir0[3 * ang], a.dir0[3 * ang + 1], a.dir0[3 * ang + 2]);         // :271,273
            amp = 1.0f;
            atten = 1.0f;
            tof = 0.0f;
            geo_len = 0.0f;                                                            // :276-279
            if (EMIT) w_ray = us_emitter_primary(a.p, uni, ray_id, k, ang, el, a.seed, &o, &d, &tof);  // (a.tx is all zero then)
        } else {
            const uint32_t v4 = us_state_voff(slot, ROWS);
            constexpr uint32_t row = STATE_ROW_BYTES;
            if (EMIT) w_ray = bld(r_in, v4 + 11 * row, 0);
            o = {bld(r_in, v4 + 0 * row, 0), bld(r_in, v4 + 1 * row, 0), bld(r_in, v4 + 2 * row, 0)};
            d = {bld(r_in, v4 + 3 * row, 0), bld(r_in, v4 + 4 * row, 0), bld(r_in, v4 + 5 * row, 0)};
            amp = bld(r_in, v4 + 6 * row, 0);
            atten = bld(r_in, v4 + 7 * row, 0);
            tof = bld(r_in, v4 + 8 * row, 0);
            geo_len = bld(r_in, v4 + 9 * row, 0);
            home = __float_as_uint(bld(r_in, v4 + 10 * row, 0));
            ray_id = udiv_fast(home, a.div_ppr);
            k = a.path_first + (home - ray_id * a.ppr_pass);
        }
        const uint32_t ang = udiv_fast(ray_id, a.div_ne);
        const V3 tn = {uni[U_TN], uni[U_TN + 1], uni[U_TN + 2]};
        Hit h;
        bool hit;
        if (first && have_hit_tab) {  // shared first hit of the ray (k_us_first)
            const float4 r = a.first_hit[ray_id];
            h.t = r.x;
            h.u = r.y;
            h.v = r.z;
            h.slot = __float_as_uint(r.w);
            h.prim = 0;
            hit = h.slot != 0xffffffffu;
        } else {
            hit = scene_intersect<ACCEL, false>(a.sc, ls, o, d, K_INF, &h);             // :309-312
        }
        if (hit) {
            did_seg = true;
            const pbrt_prim &P = tb.prims_by_slot[h.slot];
            SI si = make_si<ACCEL != ACCEL_K_BRUTE>(P, o, d, h.t, h.u, h.v, a.sc.vnormals, h.slot);
            const float distance = h.t;                                                // :314
            geo_len += distance;                                                       // :315
            if (!(quirks & PBRT_USQ_NO_TOF_ACCUM)) tof += distance * uni[U_INVC];       // :316
            // B1 (Dr.Jit variant): the draws are constants of the traced loop body -- every bounce reuses block 0
            const uint32_t block = (quirks & PBRT_USQ_FROZEN_DRAWS) ? 0u : depth;
            F4 u = rng4(ray_id, k, block, a.seed);
            uint32_t recv = min((uint32_t)(u.x * (float)NE), NE - 1);                  // :319
            const bool tab = first && have_rx_tab;  // (ray, receive element) record of k_us_first
            float4 rx = {0.0f, 0.0f, 0.0f, 0.0f};
            UsRecv rc = {{0.0f, 0.0f, 0.0f}, 0.0f};
            bool visible = false;
            float total_time = 0.0f, phase = 0.0f;
            if (tab) {
                rx = a.first_rx[(size_t)ray_id * NE + recv];
            } else {
                rc = us_receive<CONVEX>(a, uni, si.p, recv);
                Hit hs;
                visible = !scene_intersect<ACCEL, true>(a.sc, ls, offset_origin(si.p, si.n, rc.sec_dir), rc.sec_dir, K_INF, &hs);  // :324-325
                total_time = us_arrival(a, uni[U_INVC], quirks, ray_id, tof, distance, rc.dist_recv);
                phase = uni[U_2PIF] * total_time;                                      // :330
            }
            constexpr bool CONES = ACCEL != ACCEL_K_BRUTE;
            survive = us_scatter_step<CONES, CONES>(a, uni, quirks, tb.mats, P, si, distance, u, ray_id, k, block, depth, tn, o, d, amp, atten,
                                                    geo_len, [&] {
                float fd = 0.0f, carrier = 0.0f;
                uint32_t ci = 0xffffffffu;
                if (tab) {
                    fd = rx.x;
                    carrier = rx.y;
                    ci = __float_as_uint(rx.z);
                } else if (us_echo_bin(NE, T, quirks, total_time, uni[U_FS], ang, recv, visible, &ci)) {
                    us_echo_weight(a, NE, quirks, d, si.ns, rc.sec_dir, us_recv_normal<CONVEX>(a, uni, recv, tn), uni[U_AM], uni[U_AC], phase,
                                   &fd, &carrier);
                }
                float pressure = atten * amp * fd * carrier;                           // :348
                if (ci != 0xffffffffu) {
                    if (EMIT) pressure *= w_ray;  // the weight of the path's primary ray (DESIGN D15)
                    us_echo_deposit(agg_idx, agg_sum, a.channel, ci, pressure);
                }
            });
        }
    }
    const uint32_t wid = tid >> 6;
    const unsigned long long bal = __ballot(survive);
    const uint32_t prefix = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
    const unsigned long long bseg = __ballot(did_seg);
    uint32_t off = 0, total = 0;
    if (WP) {  // the wave packs its own survivors behind its own cursor
        total = (uint32_t)__popcll(bal);
        ns_acc += (uint32_t)__popcll(bseg);
    } else {
        if ((tid & 63) == 0) {
            wave_tot[buf][wid] = (uint32_t)__popcll(bal);
            wave_seg[buf][wid] = (uint32_t)__popcll(bseg);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t w = 0; w < SEG / 64; ++w) {
            uint32_t t = wave_tot[buf][w];
            off += (w < wid) ? t : 0u;
            total += t;
        }
    }
    if (survive) {
        const uint32_t v4 = us_state_voff(base + out_off + off + prefix, ROWS);
        constexpr uint32_t row = STATE_ROW_BYTES;
        if (EMIT) bst(r_out, v4 + 11 * row, 0, w_ray);
        bst(r_out, v4 + 0 * row, 0, o.x);
        bst(r_out, v4 + 1 * row, 0, o.y);
        bst(r_out, v4 + 2 * row, 0, o.z);
        bst(r_out, v4 + 3 * row, 0, d.x);
        bst(r_out, v4 + 4 * row, 0, d.y);
        bst(r_out, v4 + 5 * row, 0, d.z);
        bst(r_out, v4 + 6 * row, 0, amp);
        bst(r_out, v4 + 7 * row, 0, atten);
        bst(r_out, v4 + 8 * row, 0, tof);
        bst(r_out, v4 + 9 * row, 0, geo_len);
        bst(r_out, v4 + 10 * row, 0, __uint_as_float(home));
    }
    out_off += total;
    if (!WP && tid == 0)
        for (uint32_t w = 0; w < SEG / 64; ++w) ns_acc += wave_seg[buf][w];
    }  // chunk loop
    if (WP ? (tid & 63u) == 0 : tid == 0) {
        unsigned long long *row = a.stats + own;  // per-region / per-wave rows, see k_bounce
        const size_t stride = a.stat_stride;
        row[0] += ns_acc;
        row[stride] += ns_acc;  // one occlusion ray per shaded segment
        row[(2 + min(depth, (uint32_t)MAX_DEPTH_STATS - 1)) * stride] += cnt_in;
    }
    if (!a.fuse || out_off == 0 || depth + 1 >= a.p.max_depth) break;  // uniform over the owner
    // the survivors just written are the next bounce's input: stores complete (release at workgroup scope; the waves
    // of a workgroup share the CU's vector L1, so no invalidate), then everybody has finished reading the old input
    __threadfence_block();
    if (!WP) __syncthreads();
    const Rsrc nxt_in = r_out;
    r_out = r_in;
    r_in = nxt_in;
    cnt_in = out_off;
    ++depth;
    }  // bounce loop
    __syncthreads();  // all echoes of the workgroup are in the bins
    us_echo_flush(agg_idx, agg_sum, a.channel, tid, SEG);
    if (WP ? (tid & 63u) == 0 : tid == 0) a.seg_out[own] = out_off;
