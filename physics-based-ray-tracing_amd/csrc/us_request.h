// One acquisition request: "acquire this pbrt_us_params at ppr paths per ray", as pbrt_us_acquire / _dev / _queue_dev hand it to the
// stages of the driver (pbrt_api.hip us_impl) -- the rules the block must keep, each written once, the facts every stage reads, each
// derived once, and the constants of UsArgs the host computes.  Plain host code (no HIP), so that tests/native/us_request_check.cpp
// can build it on its own.  What needs a sine the kernels share (the curved element table, emit_sincos of kernels_us.h) stays with
// the driver.
#pragma once
#include <cmath>
#include <cstdint>
#include <numeric>

#include "../../include/pbrt_hip.h"

static inline float host_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
#define US_PI_F 3.14159265358979323846f  // (device_math.h K_PI, which does not compile without hipcc)

struct UsRequest {
    int code;  // of a refusal: PBRT_E_INVALID (the text is the rule), or PBRT_E_UNSUPPORTED (the text is the whole message)
    const pbrt_us_params *p;
    bool convex;       // the curved array (DESIGN D18): geometry from p->emitter, kernels of their own
    bool emit;         // primary rays from CustomEmitter.sample_ray, echoes times the ray's weight
    uint32_t primary;  // p->primary without the array bit (the kernels compare it with PBRT_US_PRIMARY_*; the array is a template switch of theirs)
    uint32_t NA, NE, T, n_rays;
    uint32_t n_ex;     // element positions, or the curved array's (x, z, nx, nz) table
    uint64_t nchan;
    bool tables;       // first-bounce tables (kernels_us.h k_us_first): worth it once a ray has more paths than receive elements
    bool fuse;         // all bounces of a pass in one launch
    // the constants of UsArgs: transducer normal and primary directions (world), directivity ramp, attenuation, carrier, 1 / c
    float tn[3], dir0[3 * PBRT_US_MAX_ANGLES];
    float am, ac, cos_min, katt, two_pi_f, inv_c;
};

// :248 float32 elem_x = pitch * (arange_f32 - (N-1)/2)
static inline float us_elem_x(const pbrt_us_params *p, uint32_t e) {
    return (float)((double)p->pitch * ((double)(float)e - ((double)p->n_elements - 1.0) / 2.0));
}

// a rule of the makers below: its own text is the refusal
#define US_RULE(cond)              \
    do {                           \
        if (!(cond)) return #cond; \
    } while (0)

static inline bool us_convex(const pbrt_us_params *p) { return (p->primary & PBRT_US_ARRAY_CONVEX) != 0; }
// the rules of the curved array (PBRT_US_ARRAY_CONVEX): the acquisition's, and those of pbrt_us_tx_delays and pbrt_us_array_elements
static inline const char *us_array_rules(const pbrt_us_params *p) {
    const pbrt_us_emitter &E = p->emitter;
    US_RULE(std::isfinite(E.radius) && E.radius > 0.0f);
    US_RULE(std::isfinite(E.opening_angle) && E.opening_angle > 0.0f && E.opening_angle < 180.0f);
    US_RULE(E.number_of_elements == p->n_elements);
    return nullptr;
}

// sensor frame -> world (the rotation of p->sensor_to_world), and the normalisation: CustomIntegrator.py:271,273
static inline void us_to_world(const float *M, float x, float y, float z, float *o) {
    o[0] = host_fma(M[0], x, host_fma(M[1], y, M[2] * z));
    o[1] = host_fma(M[4], x, host_fma(M[5], y, M[6] * z));
    o[2] = host_fma(M[8], x, host_fma(M[9], y, M[10] * z));
}
static inline void us_normalize(float *v) {
    float inv = 1.0f / std::sqrt(host_fma(v[0], v[0], host_fma(v[1], v[1], v[2] * v[2])));
    v[0] *= inv;
    v[1] *= inv;
    v[2] *= inv;
}

// -> nullptr and *rq filled, or the text of the first rule that failed and rq->code.  has_channel: the caller has a channel buffer.
static inline const char *us_request(UsRequest *rq, const pbrt_us_params *p, uint32_t ppr, bool has_channel) {
    rq->code = PBRT_E_INVALID;
    US_RULE(p && has_channel);
    US_RULE(p->n_angles > 0 && p->n_angles <= PBRT_US_MAX_ANGLES && p->n_elements > 0 && p->time_samples > 0);
    US_RULE((uint64_t)p->n_angles * p->n_elements * p->time_samples < 0xffffffffull);  // channel index is 32-bit (echo bins)
    US_RULE(p->max_depth > 0 && ppr > 0 && p->sound_speed > 0 && p->fs > 0);
    US_RULE(p->max_depth < 0x40000000u);  // RNG block = bounce index; bit 30 marks a path's second block of a bounce, bit 31 the emitter's
    const bool convex = us_convex(p);
    const uint32_t primary = p->primary & ~PBRT_US_ARRAY_CONVEX;
    US_RULE(primary <= PBRT_US_PRIMARY_EMITTER);
    const bool emit = primary == PBRT_US_PRIMARY_EMITTER;
    if (emit) {  // CustomEmitter as the source of the primary rays: its elements are the acquisition's (include/pbrt_hip.h)
        const pbrt_us_emitter &E = p->emitter;
        US_RULE(E.number_of_elements == p->n_elements && E.number_of_rays_per_element > 0 && E.speed_of_sound > 0.0f);
        US_RULE(std::isfinite(E.pitch) && std::isfinite(E.element_width) && std::isfinite(E.element_height) && std::isfinite(E.radius));
        US_RULE(std::isfinite(E.steering_angle_min) && std::isfinite(E.steering_angle_max) && std::isfinite(E.opening_angle));
        // an emitter on an arc and receivers on a line: never defined (D18) -- the curved array is asked for with PBRT_US_ARRAY_CONVEX
        if (!convex && E.radius != 0.0f) {
            rq->code = PBRT_E_UNSUPPORTED;
            return "emitter.radius != 0 transmits from an arc: set PBRT_US_ARRAY_CONVEX in pbrt_us_params.primary";
        }
    }
    if (convex)
        if (const char *why = us_array_rules(p)) return why;
    rq->code = PBRT_OK;
    rq->p = p;
    rq->convex = convex;
    rq->emit = emit;
    rq->primary = primary;
    const uint32_t NA = rq->NA = p->n_angles, NE = rq->NE = p->n_elements;
    rq->T = p->time_samples;
    rq->n_rays = NA * NE;
    rq->n_ex = convex ? 4u * NE : NE;
    rq->nchan = (uint64_t)rq->n_rays * rq->T;
    rq->tables = ppr >= NE && !(p->quirks & PBRT_USQ_NO_FIRST_TABLES) && !emit;  // (emitter rays: every path has its own origin)
    rq->fuse = !(p->quirks & PBRT_USQ_NO_FUSED_BOUNCES);
    const float *M = p->sensor_to_world;
    for (uint32_t a = 0; a < NA; ++a) {  // CustomIntegrator.py:265,271,273
        float ar = (float)((double)p->angles_deg[a] * (M_PI / 180.0));
        us_to_world(M, sinf(ar), 0.0f, cosf(ar), &rq->dir0[3 * a]);
        us_normalize(&rq->dir0[3 * a]);
    }
    us_to_world(M, 0.0f, 0.0f, 1.0f, rq->tn);
    us_normalize(rq->tn);
    rq->am = p->main_beam_angle * (US_PI_F / 180.0f);
    rq->ac = p->cutoff_angle * (US_PI_F / 180.0f);
    rq->cos_min = cosf(rq->ac);                                                           // :370
    rq->katt = (float)(-(double)p->attenuation * (double)p->frequency * 1e-6);            // :328
    rq->two_pi_f = (float)(2.0 * M_PI * (double)p->frequency);                            // :330
    rq->inv_c = 1.0f / p->sound_speed;
    return nullptr;
}

// what the argument block of the kernels (kernels_us.h UsArgs) takes from the request: the parameter block with `primary` as the
// kernels compare it (the array is a template switch of theirs), the constants, the fuse flag
template <class Args>
static inline void us_request_args(const UsRequest &rq, Args *a) {
    a->p = *rq.p;
    a->p.primary = rq.primary;
    for (int k = 0; k < 3; ++k) a->tn[k] = rq.tn[k];
    a->am = rq.am;
    a->ac = rq.ac;
    a->cos_min = rq.cos_min;
    a->katt = rq.katt;
    a->two_pi_f = rq.two_pi_f;
    a->inv_c = rq.inv_c;
    a->fuse = rq.fuse ? 1u : 0u;
}

// Emitter rays through the fused kernels: workgroup b walks region (b * blk_mul) mod nseg_pass, a permutation (blk_mul coprime to
// nseg_pass) with a stride of about one angle's share of the regions.  0: workgroup b stays on region b -- few regions, or
// PBRT_US_EMIT_PERMUTE=0 (A/B and test); permute > 1 (A/B): another stride.
static inline uint32_t us_emit_blk_mul(uint32_t nseg_pass, uint32_t NA, int permute) {
    if (nseg_pass <= 2u * NA || permute == 0) return 0;
    uint32_t m = (nseg_pass / NA) | 1u;
    if (permute > 1) m = (uint32_t)permute | 1u;
    while (std::gcd(m, nseg_pass) != 1u) m += 2u;
    return m % nseg_pass;
}
