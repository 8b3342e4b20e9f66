// One radiance render request: "render this crop of this camera's film at spp samples", as pbrt_render_radiance / _dev hand it to
// the stages of the driver (pbrt_api.hip render_impl) -- the argument rules, each written once, the rendered region and the row
// counts every stage reads, each derived once -- and the host arithmetic the radiance and ultrasound drivers and
// pbrt_integrator_sample share: the shape of a pass and its halving, the state-addressing rules, the default pass size, the fuse
// plan and the pass schedule, the grids of the trace / shade streams, the byte models of pbrt_stats.  Plain host code (no HIP), so
// that tests/native/render_request_check.cpp can build it on its own.  What depends on the accelerator of the scene arrives as
// arguments: region size, counters and rows per region in a RenderLaunch the driver fills, the streams' record limit (WF_DEAD),
// bytes per path (WF_BYTES_PER_PATH) and regions per workgroup (WF_KMAX) where they are used.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/pbrt_hip.h"
#include "film_key.h"

#define N_STATE 15
#define MAX_DEPTH_STATS 62
#define MAX_CHAIN 6  // bounces one launch of the multi-bounce kernels walks at most (the per-bounce counts are packed 10 bits each)
#define HIT_ROW0 (2 + MAX_DEPTH_STATS)  // k_bounce_pool: statistics rows HIT_ROW0 + d = rays of depth d that hit something

static inline uint32_t div_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

// a rule of the makers below: its own text is the refusal
#define RENDER_RULE(cond)          \
    do {                           \
        if (!(cond)) return #cond; \
    } while (0)

// ---- the request --------------------------------------------------------------------------------------------------------------
// What the scene's accelerator decides (kernels_radiance.h, kernels_wavefront.h)
struct RenderLaunch {
    bool brute;             // the fused brute-force kernels; else a BVH scene: trace / shade streams
    bool keep;              // ACCEL_K_BRUTE with at most 32 primitives: the first bounce can read tile keep words
    uint32_t region;        // slots per region (one workgroup each)
    uint32_t owners;        // live counters per region
    uint32_t rows_fused;    // statistics rows per region of the fused kernels,
    uint32_t rows_streams;  // and of k_shade
};
struct RenderRequest {
    const pbrt_camera *cam;
    const pbrt_film_desc *f;
    RenderLaunch launch;
    // the launch structure.  Brute-force scenes, or BVH scenes: these run intersection and shading as separate streams
    // (kernels_wavefront.h); PBRT_FILM_NO_HIT_POOL keeps the fused k_bounce (one launch per bounce, shading in the lanes the
    // traversal leaves) as the A/B reference -- in the diagnostic build (diag_driver.h)
    bool brute, wavefront;
    // the rendered region: the crop and the margin its filter reads, clipped to the film; rows of it in 8-row bands (region_index)
    uint32_t radius, rx0, ry0, rw, rh, tile_rows;
    uint64_t npix_r, film_px;
    uint32_t stat_rows;   // statistics rows in use: segments, shadow rays, one per depth
    uint32_t hit_rows;    // k_shade counts the rays of every depth that hit something (rows HIT_ROW0 + d, for the byte model)
    uint32_t out_floats;  // per pixel of the output: 3, or 4 with PBRT_FILM_RAW_ACCUM
    // may the call carry the keep words of the camera tiles (kernels_radiance.h k_tile_keep)?  The waves of the first bounce are
    // whole blocks of 64 region indices only if the region's pixel count is a multiple of 64
    bool tile_keep;
    uint32_t rows_per_region() const { return wavefront ? launch.rows_streams : launch.rows_fused; }
};

// -> nullptr and *rq filled, or the text of the first rule that failed (the refusal is "invalid argument: " and that text).
// d_out: the caller has an output buffer.
static inline const char *render_request(RenderRequest *rq, const pbrt_camera *cam, const pbrt_film_desc *f, bool d_out,
                                         const RenderLaunch &launch) {
    RENDER_RULE(cam && f && d_out);
    const uint32_t W = cam->film_w, H = cam->film_h;
    RENDER_RULE(W > 0 && H > 0 && f->crop_w > 0 && f->crop_h > 0);
    RENDER_RULE((uint64_t)f->crop_x + f->crop_w <= W && (uint64_t)f->crop_y + f->crop_h <= H);
    RENDER_RULE(f->spp > 0 && f->max_depth > 0 && f->filter <= PBRT_FILTER_GAUSSIAN);
    RENDER_RULE((uint64_t)W * H <= 0xffffffffull);
    rq->cam = cam;
    rq->f = f;
    rq->launch = launch;
    rq->brute = launch.brute;
    rq->wavefront = !launch.brute && !(f->flags & PBRT_FILM_NO_HIT_POOL);
    const uint32_t R = rq->radius = f->filter == PBRT_FILTER_BOX ? 0 : (f->filter == PBRT_FILTER_TENT ? 1 : 2);
    rq->rx0 = f->crop_x > R ? f->crop_x - R : 0;
    rq->ry0 = f->crop_y > R ? f->crop_y - R : 0;
    const uint32_t rx1 = std::min(f->crop_x + f->crop_w + R, W), ry1 = std::min(f->crop_y + f->crop_h + R, H);
    rq->rw = rx1 - rq->rx0;
    rq->rh = ry1 - rq->ry0;
    rq->tile_rows = rq->rh & ~7u;
    rq->npix_r = (uint64_t)rq->rw * rq->rh;
    rq->film_px = (uint64_t)f->crop_w * f->crop_h;
    rq->stat_rows = 2 + (uint32_t)std::min<uint64_t>(f->max_depth, MAX_DEPTH_STATS);
    rq->hit_rows = rq->wavefront ? rq->stat_rows - 2 : 0;
    rq->out_floats = (f->flags & PBRT_FILM_RAW_ACCUM) ? 4 : 3;
    rq->tile_keep = launch.keep && rq->npix_r % 64 == 0 && !(f->flags & PBRT_FILM_NO_TILE_CULL);
    return nullptr;
}

// the film key of the request (film_key.h), as every argument block of the kernels carries it: the region and its pixel order, the
// sizes and the two fast divisors; s_first is the pass's
static inline FilmKey render_film_key(const RenderRequest &rq) {
    FilmKey k{};
    k.rx0 = rq.rx0;
    k.ry0 = rq.ry0;
    k.rw = rq.rw;
    k.npix_r = (uint32_t)rq.npix_r;
    k.film_w = rq.cam->film_w;
    k.film_h = rq.cam->film_h;
    k.tile_rows = rq.tile_rows;
    k.div_npix = make_fastdiv(k.npix_r);
    k.div_rw = make_fastdiv(k.rw);
    return k;
}

// ---- the shape of a pass ------------------------------------------------------------------------------------------------------
// Sizing a pass: `per_call` units (samples of a film region of `unit` pixels, paths per ray of `unit` rays) in passes of at most
// pass_paths paths, rounded up to whole regions.  equal: passes of equal size instead of full ones plus a small remainder.
static const uint64_t PASS_MIN_PATHS = 1u << 20;
struct PassShape {
    uint32_t per_pass = 1, cap = 0, nseg = 0;  // units per pass; slots; regions (one workgroup each)
};
static inline const char *pass_shape(PassShape *ps, uint64_t pass_paths, uint32_t per_call, uint64_t unit, uint32_t region, bool equal) {
    uint32_t k = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(per_call, pass_paths / std::max<uint64_t>(unit, 1)));
    if (equal) k = div_up(per_call, div_up(per_call, k));
    RENDER_RULE(unit * k < 0xfffffc00ull);
    ps->per_pass = k;
    ps->cap = div_up(unit * k, region) * region;
    ps->nseg = ps->cap / region;
    return nullptr;
}
// After a failed allocation: the next pass_paths to try (half of what the shape took), or false -- a caller-fixed size, a pass of
// one unit and the smallest pass give up.
static inline bool pass_halve(uint64_t *pass_paths, bool fixed, const PassShape &ps, uint64_t unit) {
    if (fixed || ps.per_pass <= 1 || *pass_paths <= PASS_MIN_PATHS) return false;
    *pass_paths = std::max<uint64_t>(PASS_MIN_PATHS, std::min<uint64_t>(*pass_paths, unit * ps.per_pass) / 2);
    return true;
}
// How the kernels address the state of a pass of `cap` slots.  The fused kernels (`rows` dwords per slot): the tiled state arrays
// are addressed through 32-bit buffer offsets.  The streams: ray records are addressed with two flag bits on top (dead: WF_DEAD).
static inline const char *pass_addressing(uint32_t cap, bool wavefront, uint32_t rows, uint32_t dead) {
    if (!(wavefront || (uint64_t)cap * rows * 4 < 0xffffffffull)) return "wavefront || (uint64_t)cap * N_STATE * 4 < 0xffffffffull";
    if (wavefront && !(cap < dead)) return "cap < WF_DEAD";
    return nullptr;
}

// ---- the default pass size ----------------------------------------------------------------------------------------------------
// Default paths in flight per pass of the trace / shade streams: the largest power of two (PASS_MIN_PATHS .. 512 Mi) whose
// workspace (bytes_per_path each) fits two thirds of the free device memory -- `held`, what the context already holds for these
// buffers, is re-used, not allocated on top --, one half of the device's total memory, and the context's workspace limit (0: none;
// ws_total: what the context holds in all).
// Two thirds of what is free, and never more than half of the device: a tenant that arrives second (torch beside the renderer,
// USMain.py:5) still finds room, and the pass size depends less on who allocated first.  A caller that owns the device asks
// for more per call (pbrt_film_desc.pass_paths) -- bench.py does for BASELINE config 4.
static inline uint64_t stream_default_pass_paths(size_t free_b, size_t total_b, size_t held, size_t limit, size_t ws_total,
                                                 uint32_t bytes_per_path) {
    double budget = std::min((2.0 / 3.0) * (double)(free_b + held), 0.5 * (double)total_b);
    if (limit) budget = std::min(budget, (double)limit - (double)(ws_total - held) - 64e6 /* the small buffers */);
    uint64_t pass_paths = PASS_MIN_PATHS;
    while (pass_paths < (512u << 20) && 2.0 * (double)pass_paths * bytes_per_path <= budget) pass_paths *= 2;
    return pass_paths;
}
// ... and of the fused kernels: `paths`, halved under a workspace limit until bytes_per_path of each fit it (the small buffers: 64 MB)
static inline uint64_t fused_default_pass_paths(uint64_t paths, uint32_t bytes_per_path, size_t limit) {
    if (limit)
        while (paths > PASS_MIN_PATHS && (double)paths * (double)bytes_per_path > (double)limit - 64e6) paths /= 2;
    return paths;
}

// ---- the fuse plan and the pass schedule --------------------------------------------------------------------------------------
// Depths at which a launch of the brute-force kernels walks two bounces (bit d: bounces d and d + 1).  Measured on the
// Cornell box (0x1 while the two-bounce kernels ran at 6 - 7 waves per SIMD, every pair since they run
// at 8); pbrt_film_desc.flags can override it per call (PBRT_FILM_FUSE_PLAN).
#ifndef PBRT_DEFAULT_FUSE_PLAN
#define PBRT_DEFAULT_FUSE_PLAN 0x15u
#endif
// Fuse plan: bit d set = the launch that walks bounce d goes on with bounce d + 1 in registers (at most MAX_CHAIN bounces per
// launch).  0 = one launch per bounce, 0x15 = pairs, all ones = as many bounces per launch as MAX_CHAIN allows.
static inline uint32_t chain_len(uint32_t plan, uint32_t depth, uint32_t max_depth) {
    uint32_t nb = 1;
    while (nb < MAX_CHAIN && depth + nb < max_depth && depth + nb - 1 < 32 && ((plan >> (depth + nb - 1)) & 1u)) ++nb;
    return nb;
}
// The plan that pays for a scene follows from how many paths survive each bounce: walking bounce d + 1 in the same launch saves
// the state round trip of the survivors and costs the idle lanes of the others.  Measured (cbox, survival 0.87 / 0.77 / 0.83 /
// 0.85 / 0.20: ONE launch for all six bounces 6.23 ms, triples 6.30, pairs 6.58; open scenes with survival 0.37 - 0.49 / 0.29 /
// 0.33: pairs 2.11 / 4.52 ms, triples 2.11 / 4.84, one launch 2.47 / 5.70): go on while at least 45 % of the paths do; the last
// bounce of a path only looks for emitters and is always taken along.  Any plan renders the same film.
static inline uint32_t plan_from_survival(const unsigned long long *live, uint32_t max_depth) {
    uint32_t plan = 0;
    for (uint32_t d = 0; d + 1 < max_depth && d < 31; ++d) {
        const bool last = d + 2 == max_depth;
        if (live[d] == 0) break;
        if (last || (double)live[d + 1] >= 0.45 * (double)live[d]) plan |= 1u << d;
    }
    return plan;
}
// First render of a brute-force scene with the plan left to the library: the first PROBE_SPP samples are a pass of their own,
// their path survival is read back and decides the plan of all the other passes.  The film does not depend on how the samples
// are split into passes, nor on the plan.
constexpr uint32_t PROBE_SPP = 2;
// The fuse plan of a call: the caller's, or the one learnt from the last render of this scene (hint), or the library default --
// and then, with samples enough (may_probe: and a launch structure that reads the plan), a probe pass replaces it.
struct FusePlan {
    uint32_t plan = 0;
    bool probe = false;
    uint32_t source = PBRT_PLAN_DEFAULT;  // PBRT_PLAN_*
};
static inline FusePlan fuse_plan(const RenderRequest &rq, bool hint_valid, uint32_t hint, uint32_t s_pass, bool may_probe = true) {
    const uint32_t flags = rq.f->flags;
    const bool caller = (flags & PBRT_FILM_FUSE_PLAN_SET) != 0, learnt = rq.brute && hint_valid;
    FusePlan p;
    p.plan = !rq.brute ? 0u : caller ? ((flags >> 8) & 0xffu) : (hint_valid ? hint : PBRT_DEFAULT_FUSE_PLAN);
    p.probe = may_probe && rq.brute && !hint_valid && rq.f->spp >= 8 * PROBE_SPP && s_pass >= PROBE_SPP && !caller;
    p.source = rq.wavefront ? PBRT_PLAN_STREAMS : caller ? PBRT_PLAN_CALLER : p.probe ? PBRT_PLAN_PROBED : learnt ? PBRT_PLAN_LEARNT : PBRT_PLAN_DEFAULT;
    return p;
}
// The passes of a call: `spp` samples in passes of s_pass, the probe pass of PROBE_SPP first (if the plan is to be learnt), and
// then equal passes for what is left.  for (PassSchedule p{spp, s_pass, probe}; p.next();) -- pass p.passes - 1 takes the samples
// [p.s0, p.s0 + p.sc); p.probing(): it is the probe pass.
struct PassSchedule {
    uint32_t spp, s_pass;
    bool probe;
    uint32_t s0 = 0, sc = 0, passes = 0;
    bool probing() const { return probe && passes == 1; }
    bool next() {
        s0 += sc;
        if (s0 >= spp) return false;
        if (probing()) s_pass = div_up(spp - s0, div_up(spp - s0, s_pass));  // (the pass before this one was the probe pass)
        sc = probe && passes == 0 ? PROBE_SPP : std::min(s_pass, spp - s0);
        ++passes;
        return true;
    }
};

// ---- the grids of the trace / shade streams -------------------------------------------------------------------------------------
// Workgroup shape of k_trace: the image plus (rows + 1) stack rows per workgroup; two 1024-thread workgroups per CU when both fit
// (8 waves per SIMD at <= 64 VGPRs), else one.
// 1024-thread workgroups for trees in global memory as well: what counts is the size of the queue a workgroup's waves share
// (bunny.ply 1024^2 x 64: 256 / 512 / 1024 threads 38.5 / 31.6 / 30.2 ms), not the LDS -- a copy of the top of the tree (the
// first 16 .. 1008 nodes in breadth-first order) in LDS on top of that was worth 1 - 2 %: the vector caches hold those nodes anyway
struct WfShape {
    uint32_t threads, rows;
    size_t lds;
    bool packet;  // camera rays as packets: the wave's stack is the 64 lanes of one register (bvh_packet_closest)
};
static inline WfShape wf_shape(uint32_t lds_limit, uint32_t image, uint32_t bvh_depth, bool packet) {
    WfShape p;
    const uint32_t limit = lds_limit ? lds_limit : 65536u;
    p.threads = 1024u;
    const uint32_t statics = 1024;  // queue words and the segment table, with slack
    uint32_t budget = limit / 2;     // two workgroups per CU
    if (image + statics + 3u * p.threads * 4u > budget) budget = limit;
    const uint32_t rows_fit = (budget - image - statics) / (p.threads * 4u);
    p.rows = std::max(2u, std::min(rows_fit, 8u));
    p.packet = packet && 3u * bvh_depth <= 64u;
    p.lds = (size_t)image + (size_t)p.rows * p.threads * 4u;
    return p;
}
// workgroups of a k_trace launch over nr regions: at least nr / kmax (a workgroup walks at most kmax = WF_KMAX regions), else `mult` per CU
static inline uint32_t wf_trace_grid(uint32_t nr, uint32_t mult, uint32_t cus, uint32_t kmax) {
    return std::min(nr, std::max(div_up(nr, kmax), std::max(1u, mult * cus)));
}
// part h of `parts` of a pass of nreg regions: its first region and how many
static inline void wf_part(uint32_t nreg, uint32_t parts, uint32_t h, uint32_t *reg0, uint32_t *regn) {
    *reg0 = (uint32_t)((uint64_t)nreg * h / parts);
    *regn = (uint32_t)((uint64_t)nreg * (h + 1) / parts) - *reg0;
}

// ---- the byte models ----------------------------------------------------------------------------------------------------------
// Byte model of the radiance path (DESIGN.md "Algorithmic bytes").  live[d] = paths entering depth d.
// A launch that walks two bounces (fuse plan bit d) keeps its paths in registers between them: the survivors of bounce d
// are neither written nor read back, only the survivors of bounce d + 1 are.
// hits (k_bounce_pool launches, BVH scenes, bounces >= 1; else nullptr): hits[d] = rays of depth d that hit something.  Every ray
// reads its origin and direction (24 B), a path that hit something reads its full state.
static inline void radiance_model_bytes(const unsigned long long *live, uint32_t nd, uint64_t samples, uint64_t film_px,
                                        uint32_t passes, uint32_t fuse_plan, uint32_t max_depth, const unsigned long long *hits,
                                        uint64_t *total, uint64_t *bounce) {
    uint64_t b = 0;
    for (uint32_t d = 0; d < nd;) {
        const uint32_t nb = std::min(chain_len(fuse_plan, d, max_depth), nd - d);
        uint64_t in = live[d], next = (d + nb < nd) ? live[d + nb] : 0;
        if (d > 0 && hits)
            b += in * 24 + hits[d] * (N_STATE * 4);
        else if (d > 0)
            b += in * (N_STATE * 4);  // state read
        b += next * (N_STATE * 4);            // compacted survivors written
        b += (in - next) * 12;                // radiance of the paths that ended (at either bounce of the launch)
        d += nb;
    }
    *bounce = b;
    *total = b + samples * 12 /* film gather reads Lhome once */ + film_px * 32ull * passes /* accumulator RMW */ +
             film_px * 28 /* resolve */;
}
// Byte model of the two-launch bounce, the bytes the algorithm NEEDS, per depth d with live[d] rays of which
// hits[d] hit something (both counted on the device), S = shadow rays of the render:
//   k_trace (k_trace_primary at depth 0: the camera rays are generated in registers)
//       32 B per continuation ray (origin, direction planes; depth >= 1), 4 B hit index written (the primitive, or none)
//       per shadow ray: 32 B read + 4 B visibility written
//   k_shade
//       4 B hit index per ray ((t, u, v) are recomputed from the primitive's record, not read)
//       depth >= 1: the state of a path once -- 48 B (L / A / B planes) if its ray left the scene, all six planes (96 B) if it hit
//       16 B radiance record per path that ends, 96 B per survivor, 32 B per shadow ray it emits
// (the 64-byte primitive record and the vertex normals of a hit come from tables that stay in L2: 0 B.)  What the kernels move on
// top of that -- the 48 bytes k_shade reads twice for a path that hit, whole 128-byte lines for sparse gathers -- is traffic, not
// model: profiles/pmc_traffic.json has the ratio.  *trace = the part of the total that is k_trace's.
static inline uint64_t wavefront_model_bytes(const unsigned long long *live, const unsigned long long *hits, uint32_t nd, uint64_t shadows,
                                             uint64_t *trace) {
    uint64_t tr = 0, sh = 0;
    for (uint32_t d = 0; d < nd; ++d) {
        const uint64_t in = live[d], next = d + 1 < nd ? live[d + 1] : 0, h = std::min<uint64_t>(hits[d], in);
        if (!in) break;
        tr += (d > 0 ? in * 32 : 0) + in * 4;
        sh += in * 4 + (d > 0 ? (in - h) * 48 + h * 96 : 0);
        sh += (in - next) * 16 + next * 96;
    }
    tr += shadows * 36;
    sh += shadows * 32;
    if (trace) *trace = tr;
    return tr + sh;
}
// What pbrt_stats reports of a render from its reduced statistics rows (hstats: segments, shadow rays, live paths per depth; from
// HIT_ROW0 on k_shade's hits per depth): the fused kernels' model, or with the streams' bounces in place of theirs.
struct ModelBytes {
    uint64_t total, bounce, trace;
};
static inline ModelBytes render_model_bytes(const RenderRequest &rq, const unsigned long long *hstats, uint64_t samples, uint32_t passes,
                                            uint32_t plan) {
    ModelBytes m{0, 0, 0};
    radiance_model_bytes(hstats + 2, MAX_DEPTH_STATS, samples, rq.film_px, passes, plan, rq.f->max_depth,
                         rq.wavefront ? hstats + HIT_ROW0 : nullptr, &m.total, &m.bounce);
    if (rq.wavefront) {
        m.total -= m.bounce;
        m.bounce = wavefront_model_bytes(hstats + 2, hstats + HIT_ROW0, MAX_DEPTH_STATS, hstats[1], &m.trace);
        m.total += m.bounce;
    }
    return m;
}
