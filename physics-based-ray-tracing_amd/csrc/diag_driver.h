// diag_driver.h -- host side of the diagnostic build only (make diag, -DPBRT_DIAG -> libpbrt_hip_diag.so).
//
// Everything the diagnostic build adds to the drivers of pbrt_api.hip, which includes this file after the product helpers it calls
// (launch_bounce, chain_len, poll_live, the stages of the radiance render).  The launch structures here lost their A/B (DESIGN.md
// section 6, kernels_diag.h); tests and tools/walk_ab.py / tools/parity_sweep.py still hold them to the product's film:
//   PBRT_FILM_REGEN            k_regen: persistent waves with path regeneration, one launch per pass
//   PBRT_FILM_WALK_FROM(d)     k_walk: from depth d on one launch walks every remaining bounce of the pass
//   PBRT_PAIR_MERGE=k          k_chain_pair: the whole path in one launch, two tiles per wave, merged at bounce k
//   PBRT_FILM_NO_HIT_POOL      BVH scenes through the fused k_bounce, with the repack pass unless PBRT_FILM_NO_REPACK
//   PBRT_US_FUSED_BVH=1        BVH scenes through the fused k_us_bounce (no emitter rays), not the streams
// The product library refuses the flags and does not read the two environment variables.
#pragma once

// Depth from which one launch walks every remaining bounce of a pass (k_walk; 0xff: never).  PBRT_FILM_WALK_FROM overrides.
#ifndef PBRT_DEFAULT_WALK_FROM
#define PBRT_DEFAULT_WALK_FROM 0xffu
#endif

// ---- kernel selectors -----------------------------------------------------------------------------------------------------------
// k_walk: every remaining bounce of the pass in one launch (nb == 2: with a fused first trip)
static RadKern diag_walk_kernel(const pbrt_scene *s, bool first, uint32_t nb) {
    return with_flags(
        [](auto F, auto B, auto N) -> RadKern { return &k_walk<F(), B() ? ACCEL_K_BRUTE_BIG : ACCEL_K_BRUTE, N() ? 2 : 1>; }, first,
        s->accel_kernel != ACCEL_K_BRUTE, nb == 2);
}
// the fused bounce of BVH scenes, radiance and ultrasound (the product runs them as k_trace / k_shade / k_us_shade streams)
static RadKern diag_bvh_kernel(const pbrt_scene *s, bool first) {
    return with_flags([](auto F, auto L) -> RadKern { return &k_bounce<F(), L() ? ACCEL_K_BVH_LDS : ACCEL_K_BVH_GLOBAL>; }, first,
                      s->accel_kernel == ACCEL_K_BVH_LDS);
}
static UsKern diag_us_bvh_kernel(const pbrt_scene *s, bool first, bool convex) {
    return with_flags([](auto F, auto L, auto X) -> UsKern {
        return &k_us_bounce<F(), L() ? ACCEL_K_BVH_LDS : ACCEL_K_BVH_GLOBAL, false, US_Q_RUNTIME, -1, X()>; },
                      first, s->accel_kernel == ACCEL_K_BVH_LDS, convex);
}
// Scenes whose tree is in LDS: the LDS limit of their fused kernels (us: the ultrasound ones, else the radiance ones)
static int diag_lds_attr(pbrt_scene *s, bool us) {
    if (s->accel_kernel != ACCEL_K_BVH_LDS) return PBRT_OK;
    for (bool first : {true, false}) {
        if (!us) {
            HIPCHK(s->ctx, set_max_lds(diag_bvh_kernel(s, first), s->lds_bytes));
            continue;
        }
        for (bool convex : {false, true}) HIPCHK(s->ctx, set_max_lds(diag_us_bvh_kernel(s, first, convex), s->lds_bytes));
    }
    return PBRT_OK;
}

// ---- ultrasound: PBRT_US_FUSED_BVH=1 (read per call) takes BVH scenes off the streams (us_impl; launch_us picks the kernel) -----
static int diag_us_fused_bvh(pbrt_scene *s, bool *streams) {
    const char *e = getenv("PBRT_US_FUSED_BVH");
    if (!*streams || !e || atoi(e) == 0) return PBRT_OK;
    *streams = false;
    return diag_lds_attr(s, true);
}

// ---- radiance -------------------------------------------------------------------------------------------------------------------
// k_chain_pair is launched instead of the k_bounce chain when PBRT_PAIR_MERGE=k names the merge bounce and the plan walks the whole
// path in one launch.
static uint32_t pair_merge_bounce(uint32_t k, uint32_t plan, uint32_t max_depth) {
    if (max_depth > MAX_CHAIN || max_depth < 2 || chain_len(plan, 0, max_depth) < max_depth) return 0;
    return k < max_depth ? k : 0u;
}
// What a diagnostic render adds to the Render of the product stages
struct DiagRender {
    uint32_t pair_merge = 0;                   // PBRT_PAIR_MERGE (read per call; 0: off)
    uint32_t walk_from = PBRT_DEFAULT_WALK_FROM;
    // fused BVH kernels: the live paths are made dense again before every bounce of depth >= 2 (k_scan_owners / k_repack_copy)
    bool repack = false;
    float *stC = nullptr;
    uint32_t *segC = nullptr, *offs = nullptr, *quota = nullptr;
};
static uint32_t diag_pair_merge() {
    const char *e = getenv("PBRT_PAIR_MERGE");
    return e ? (uint32_t)atoi(e) : 0u;
}
// Does this call select a diagnostic launch structure?  (BVH scenes without PBRT_FILM_NO_HIT_POOL run as streams whatever else is set.)
static bool diag_selected(const Render &r) {
    if (r.rq.wavefront) return false;
    return !r.rq.brute || (r.f->flags & (PBRT_FILM_REGEN | PBRT_FILM_WALK_SET)) || diag_pair_merge() != 0 || PBRT_DEFAULT_WALK_FROM != 0xffu;
}

// The bounces of one pass through a diagnostic launch structure: k_regen, or the chain of the plan with k_walk from walk_from on,
// k_chain_pair in place of a chain that walks the whole path, or the fused BVH bounce with or without repack.
static int diag_pass(Render &r, const DiagRender &dg, RadArgs a, uint32_t nseg_pass) {
    pbrt_scene *s = r.s;
    pbrt_ctx *c = r.c;
    const pbrt_film_desc *f = r.f;
    const bool brute = r.rq.brute;
    const uint32_t region = r.rq.launch.region;
    hipStream_t st = c->stream;
    int rc;
    // state for this pass: none if one launch walks all its bounces
    const bool one_launch = brute && !(f->flags & (PBRT_FILM_WALK_SET | PBRT_FILM_REGEN)) && chain_len(r.fp.plan, 0, f->max_depth) >= f->max_depth;
    const size_t need = one_launch ? (size_t)region : (size_t)nseg_pass * region;
    float *in = (float *)c->buf("stateA", need * N_STATE * 4), *out = (float *)c->buf("stateB", need * N_STATE * 4);
    if (!in || !out) return PBRT_E_NOMEM;
    a.state_cap = (uint32_t)need;
    uint32_t *sin = r.segA, *sout = r.segB;
    if (brute && (f->flags & PBRT_FILM_REGEN)) {
        // persistent waves with path regeneration (k_regen): one launch per pass, as many workgroups as the GPU holds at once
        int per_cu = 0;
        const void *fn = s->accel_kernel == ACCEL_K_BRUTE ? reinterpret_cast<const void *>(&k_regen<ACCEL_K_BRUTE>)
                                                          : reinterpret_cast<const void *>(&k_regen<ACCEL_K_BRUTE_BIG>);
        HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, REGEN_WG, 0));
        const uint32_t wpw = REGEN_WG / 64;
        uint32_t grid = (uint32_t)std::max(per_cu, 1) * (uint32_t)c->n_cu;
        grid = std::min(grid, std::max(1u, r.n_rows / wpw));            // one statistics row per wave
        grid = std::min(grid, div_up(a.n_paths, REGEN_WG));
        a.depth = 0;
        if ((rc = r.timer.begin()) != 0) return rc;
        if (s->accel_kernel == ACCEL_K_BRUTE)
            hipLaunchKernelGGL(k_regen<ACCEL_K_BRUTE>, dim3(grid), dim3(REGEN_WG), 0, st, a);
        else
            hipLaunchKernelGGL(k_regen<ACCEL_K_BRUTE_BIG>, dim3(grid), dim3(REGEN_WG), 0, st, a);
        HIPCHK(c, hipGetLastError());
        ++r.launches;
        return PBRT_OK;
    }
    for (uint32_t depth = 0; depth < f->max_depth;) {
        const uint32_t nb = brute ? chain_len(r.fp.plan, depth, f->max_depth) : 1u;
        a.depth = depth;
        a.nb = nb;
        a.in = in;
        a.out = out;
        a.seg_in = sin;
        a.seg_out = sout;
        if (dg.repack && depth >= 2) {
            // Only the regions THIS pass launched take part: a short last pass (spp not a multiple of the pass size)
            // launches nseg_pass < nseg workgroups, so paths dealt to regions >= nseg_pass would never be traced, and
            // the counters of those regions are left over from the previous pass.
            const uint32_t owners = rad_owners_per_region(s->accel_kernel), wreg = region / owners;
            const uint32_t n_own_pass = nseg_pass * owners;
            hipLaunchKernelGGL(k_scan_owners, dim3(1), dim3(1024), 0, st, sin, n_own_pass, wreg, owners, (uint32_t)c->n_cu, dg.offs,
                               dg.segC, dg.quota);
            hipLaunchKernelGGL(k_repack_copy, dim3(n_own_pass), dim3(256), 0, st, in, dg.stC, sin, dg.offs, dg.quota, n_own_pass, wreg);
            a.in = dg.stC;
            a.seg_in = dg.segC;
        }
        if (depth == 0 && (rc = r.timer.begin()) != 0) return rc;
        const bool walk = brute && depth >= dg.walk_from;  // this launch walks every remaining bounce of the pass
        const uint32_t pair_m = (brute && depth == 0 && !walk) ? pair_merge_bounce(dg.pair_merge, r.fp.plan, f->max_depth) : 0u;
        if (pair_m) {  // the whole path in one launch, two tiles per wave
            a.merge_at = pair_m;
            const uint32_t g2 = div_up(a.n_paths, 2u * SEG_BRUTE);
            if (s->accel_kernel == ACCEL_K_BRUTE)
                hipLaunchKernelGGL(k_chain_pair<ACCEL_K_BRUTE>, dim3(g2), dim3(SEG_BRUTE), 0, st, a);
            else
                hipLaunchKernelGGL(k_chain_pair<ACCEL_K_BRUTE_BIG>, dim3(g2), dim3(SEG_BRUTE), 0, st, a);
        } else if (walk || !brute) {
            const RadKern k = walk ? diag_walk_kernel(s, depth == 0, nb) : diag_bvh_kernel(s, depth == 0);
            const bool lds = s->accel_kernel == ACCEL_K_BVH_LDS;
            hipLaunchKernelGGL(k, dim3(nseg_pass), dim3(seg_threads(s->accel_kernel)), lds ? s->lds_bytes : 0u, st, a);
        } else if ((rc = launch_bounce(s, a, nseg_pass, depth == 0, nb)) != 0) {
            return rc;
        }
        HIPCHK(c, hipGetLastError());
        ++r.launches;
        if (walk) break;
        std::swap(in, out);
        std::swap(sin, sout);
        const uint32_t depth_before = depth;
        depth += nb;
        bool dead;
        if ((rc = poll_live(c, f->max_depth, depth_before, depth, sin, r.n_own, &dead)) != 0) return rc;
        if (dead) break;
    }
    return PBRT_OK;
}

// A radiance render whose passes go through diag_pass: the stages of render_impl around the pass loop of render_passes, repeated
// here with the other pass function.
static int diag_render(Render &r) {
    pbrt_ctx *c = r.c;
    const pbrt_film_desc *f = r.f;
    const bool brute = r.rq.brute;
    int rc;
    if (!brute && (rc = diag_lds_attr(r.s, false)) != 0) return rc;
    if ((rc = render_buffers(r)) != 0) return rc;
    if ((rc = render_clear(r)) != 0) return rc;
    render_plan(r, !(f->flags & (PBRT_FILM_WALK_SET | PBRT_FILM_REGEN)));
    DiagRender dg;
    dg.pair_merge = diag_pair_merge();
    if (f->flags & PBRT_FILM_WALK_SET) dg.walk_from = (f->flags >> 17) & 0xffu;
    dg.repack = !brute && rad_wave_private(r.s->accel_kernel) && !(f->flags & PBRT_FILM_NO_REPACK);
    if (dg.repack) {
        dg.stC = (float *)c->buf("stateC", (size_t)r.ps.cap * N_STATE * 4);
        dg.segC = (uint32_t *)c->buf("segC", (size_t)r.n_own * 4);
        dg.offs = (uint32_t *)c->buf("seg_offs", (size_t)r.n_own * 4);
        dg.quota = (uint32_t *)c->buf("seg_quota", 64);
        if (!dg.stC || !dg.segC || !dg.offs || !dg.quota) return PBRT_E_NOMEM;
    }
    if ((rc = render_args(r)) != 0) return rc;
    if ((rc = render_tile_keep(r)) != 0) return rc;
    render_film(r);
    for (PassSchedule p{f->spp, r.ps.per_pass, r.fp.probe}; p.next(); ++r.passes) {
        RadArgs a = r.base;
        a.n_paths = (uint32_t)(r.rq.npix_r * p.sc);
        a.key.s_first = f->sample_offset + p.s0;
        if ((rc = diag_pass(r, dg, a, div_up(a.n_paths, r.rq.launch.region))) != 0) return rc;
        if ((rc = r.timer.end()) != 0) return rc;
        r.fa.key.s_first = a.key.s_first;
        r.fa.s_count = p.sc;
        film_accum(c, r.fa);
        HIPCHK(c, hipGetLastError());
        // learn the plan from the probe pass
        if (p.probing() && (rc = probe_plan(c, r.segstats, r.n_rows, r.rq.stat_rows, r.dstats, f->max_depth, &r.fp.plan)) != 0) return rc;
    }
    if ((rc = render_finish(r)) != 0) return rc;
    if ((rc = render_stats(r)) != 0) return rc;
    if (brute && (f->flags & PBRT_FILM_REGEN)) {  // k_regen keeps the paths in registers: only the radiance records are written
        pbrt_stats &S = c->stats;
        S.model_bytes = S.model_bytes - S.bounce_model_bytes + S.samples * 12;
        S.bounce_model_bytes = S.samples * 12;
    }
    return PBRT_OK;
}
