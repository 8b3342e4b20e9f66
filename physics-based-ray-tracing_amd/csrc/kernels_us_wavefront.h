// kernels_us_wavefront.h -- ultrasound mode on BVH scenes (tessellated phantoms, meshes) as streams (gfx950).
//
// The fused ultrasound bounce (kernels_us.h k_us_bounce<.., BVH>) walks the tree for the closest hit, shades, and walks it again
// for the unbounded occlusion ray towards the receive element (CustomIntegrator.py:324-325), all in one kernel: 125 - 128 VGPRs,
// four waves per SIMD, and a wave stays in the tree until its last lane has left it.  Here a bounce is the two launches of the
// radiance streams (kernels_wavefront.h):
//   k_trace      unchanged: the continuation rays of the live paths (closest hit) and the occlusion rays the previous bounce
//                emitted (any hit, unbounded), 64 VGPRs, eight waves per SIMD
//   k_us_shade   every wave on its own: paths whose ray left the scene end, the others are listed and shaded 64 at a time --
//                the bounce from the hit on (:314-376; kernels_us.h us_receive .. us_scatter_step) -- the occlusion ray is handed out instead of
//                traced: the echo (channel index, pressure) rides in the path state as PENDING and is deposited by the next
//                k_us_shade once k_trace has written its visibility (a path that ended meanwhile leaves a record of its own).
//                A flush (k_trace + k_us_shade on the records alone) follows the last bounce.
//                The kernel is one call of shade_walk (kernels_wavefront.h: regions, chunks, hit lists, slot reservation, counts)
//                with the mode UsShade below -- the statements of k_us_bounce at the walk's hooks -- and, around it, the echo
//                table and the uniforms in LDS and the final barrier before the table is flushed.
// Same arithmetic per path, same RNG keys; the echoes of a bin are summed in another order (f32 atomics, as before).
// With first-bounce tables (k_us_first) depth 0 needs no tracing at all: k_us_shade<true> reads the ray's shared hit and the
// (ray, receive element) record, visibility included, and deposits at once.
//
// Path state, 64 B in float4 planes:  q0 = (o, amp)  q1 = (d, atten)  q2 = (tof, geo_len, home, pending channel index | ~0)
//                                     q3 = (pending pressure, weight of the primary ray, -, visibility: written 0 here, set by k_trace)
// Occlusion-ray records as in kernels_wavefront.h: q0 = (origin, tmax = inf), q1 = (direction, dest); records of ended paths also
// q2 = (pressure, channel index, -, visibility).
#pragma once
#include "kernels_us.h"
#include "kernels_wavefront.h"

#define US_WF_STATE_Q 4u
#define US_WF_VIS_Q 3u   // plane whose .w receives the visibility (WfArgs::vis_q)

struct UsWfArgs {
    UsArgs u;                       // scene, acquisition parameters, tables, channel buffer, statistics rows
    float4 *st_in, *st_out;         // [4][cap]
    uint32_t *hit_id;
    float4 *shd_in, *shd_out;       // [4][cap]
    const uint32_t *seg_in, *nsh_in;
    uint32_t *seg_out, *nsh_out;
    uint32_t region0, n_regions;
    uint32_t *guard;                // the context's guard words (kernels_wavefront.h WfArgs::guard)
};

// primary rays of a pass into the path state (depth 0 without first-bounce tables): CustomIntegrator.py:270-279
// CONVEX: the curved array's origins come from the element table (kernels_us.h us_elem_point)
template <bool CONVEX = false>
__global__ __launch_bounds__(256) void k_us_init_wf(const UsArgs a, float4 *st, uint32_t *seg_cnt, uint32_t n_regions) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_regions) seg_cnt[i] = a.n_paths > i * WF_REGION ? min(a.n_paths - i * WF_REGION, WF_REGION) : 0u;  // (wf_region_fill, spelled out as in k_init_rays_wf)
    if (i >= a.n_paths) return;
    const uint32_t ray_id = udiv_fast(i, a.div_ppr);
    const uint32_t ang = udiv_fast(ray_id, a.div_ne), el = ray_id - ang * a.p.n_elements;
    V3 o = us_elem_point<CONVEX>(a, a.p.sensor_to_world, el);
    V3 d = v3(a.dir0[3 * ang], a.dir0[3 * ang + 1], a.dir0[3 * ang + 2]);
    float tof = 0.0f, w_ray = 1.0f;
    if (a.p.primary == PBRT_US_PRIMARY_EMITTER)  // the path's own ray from CustomEmitter.sample_ray (kernels_us.h us_emitter_primary)
        w_ray = us_emitter_primary(a.p, a.p.sensor_to_world, ray_id, a.path_first + (i - ray_id * a.ppr_pass), ang, el, a.seed, &o, &d, &tof);
    const size_t cp = a.cap;
    const float4 q0 = {o.x, o.y, o.z, 1.0f}, q1 = {d.x, d.y, d.z, 1.0f}, q2 = {tof, 0.0f, __uint_as_float(i), __uint_as_float(0xffffffffu)},
                 q3 = {0.0f, w_ray, 0.0f, 0.0f};  // q3.y: the weight of the path's primary ray (1 for the integrator's own)
    st[i] = q0;
    st[cp + i] = q1;
    st[2u * cp + i] = q2;
    st[3u * cp + i] = q3;
}

// TAB: depth 0 with the first-bounce tables (the paths are generated from their index, nothing is read but the tables).
// CYL: the scene holds cylinders (else their code is compiled out).  CONVEX: the curved array (kernels_us.h us_elem_point)
// The mode of shade_walk (kernels_wavefront.h): what an ultrasound bounce does at the walk's hooks.
template <bool TAB, bool CYL, bool CONVEX>
struct UsShade {
    struct Chunk {
        float4 q2, q3;  // (tof, geo_len, home, pending channel index | ~0), (pending pressure, weight, -, visibility)
    };
    struct Path {
        V3 o = {0, 0, 0}, d = {0, 0, 1}, so = {0, 0, 0}, sdir = {0, 0, 1};
        float amp = 1.0f, atten = 1.0f, tof = 0.0f, geo_len = 0.0f, pressure = 0.0f, w_ray = 1.0f;
        uint32_t home = 0, ci = 0xffffffffu;  // ci: the channel index of an echo (pressure) that waits for its occlusion ray
    };
    const UsWfArgs &w;     // (by reference: its tables are indexed at run time, a copy would live in scratch)
    const uint32_t NE, T;  // elements, time samples: read once by the kernel
    uint32_t (&agg_idx)[US_AGG_BINS];  // the workgroup's echo table, and its uniforms
    float (&agg_sum)[US_AGG_BINS], (&uni)[U_COUNT];

    DEV void stage() const {
        us_echo_clear(agg_idx, agg_sum, threadIdx.x, WF_SHADE_THREADS);
        us_stage_uniforms(w.u, uni);  // through LDS as in k_us_bounce: the kernel wants more scalars than a wave has
    }
    DEV void dead_record(uint32_t i) const {  // the echo of a path that ended at the previous bounce, if its ray got through
        const float4 rec = w.shd_in[2u * (size_t)w.u.cap + i];
        if (rec.w != 0.0f) us_echo_deposit(agg_idx, agg_sum, w.u.channel, __float_as_uint(rec.y), rec.x);
    }
    DEV uint32_t load(uint32_t slot, Chunk &c) const {
        const UsArgs &a = w.u;
        if (TAB) return __float_as_uint(a.first_hit[udiv_fast(slot, a.div_ppr)].w);  // the primitive the ray's shared first hit lies on
        const size_t cp = a.cap;
        const uint32_t hid = w.hit_id[slot];
        c.q2 = w.st_in[2u * cp + slot];
        c.q3 = w.st_in[3u * cp + slot];
        return hid;
    }
    DEV void entry(uint32_t, bool valid, bool, const Chunk &c) const {
        // the pending echo of the previous bounce (every path, whether it goes on or not; a path that missed ends without a record)
        if (!TAB && valid && c.q3.w != 0.0f && __float_as_uint(c.q2.w) != 0xffffffffu)
            us_echo_deposit(agg_idx, agg_sum, w.u.channel, __float_as_uint(c.q2.w), c.q3.x);
    }
    DEV void keep(uint32_t, const Chunk &) const {}
    // the bounce from the hit on, through the pieces of kernels_us.h that k_us_bounce runs
    DEV bool shade(uint32_t slot, uint32_t prim, uint32_t, Path &p) const {
        const UsArgs &a = w.u;
        const size_t cp = a.cap;
        Hit h;
        h.slot = prim;
        h.prim = h.slot;
        uint32_t ray_id, k, ang;
        float4 rx = {0.0f, 0.0f, 0.0f, 0.0f};
        if (TAB) {
            p.home = slot;
            ray_id = udiv_fast(p.home, a.div_ppr);
            k = a.path_first + (p.home - ray_id * a.ppr_pass);
            ang = udiv_fast(ray_id, a.div_ne);
            const uint32_t el = ray_id - ang * NE;
            p.o = us_elem_point<CONVEX>(a, uni, el);                                    // :270,273
            p.d = v3(a.dir0[3 * ang], a.dir0[3 * ang + 1], a.dir0[3 * ang + 2]);        // :271,273
            const float4 fh = a.first_hit[ray_id];
            h.t = fh.x;
            h.u = fh.y;
            h.v = fh.z;
        } else {
            const float4 q0 = w.st_in[slot], q1 = w.st_in[cp + slot], q2 = w.st_in[2u * cp + slot];
            // the weight of the path's primary ray rides in q3.y (k_us_init_wf); it is 1 unless the rays come from the emitter, so
            // only that mode reads it
            if (a.p.primary == PBRT_US_PRIMARY_EMITTER) p.w_ray = w.st_in[3u * cp + slot].y;
            p.o = {q0.x, q0.y, q0.z};
            p.amp = q0.w;
            p.d = {q1.x, q1.y, q1.z};
            p.atten = q1.w;
            p.tof = q2.x;
            p.geo_len = q2.y;
            p.home = __float_as_uint(q2.z);
            ray_id = udiv_fast(p.home, a.div_ppr);
            k = a.path_first + (p.home - ray_id * a.ppr_pass);
            ang = udiv_fast(ray_id, a.div_ne);
        }
        const pbrt_prim P = wf_load_prim(a.sc.prims + h.slot);
        const bool has_vn = a.sc.vnormals != nullptr;  // uniform
        WfVn vn;
        if (has_vn) vn = wf_load_vn(a.sc.vnormals, h.slot);
        if (!TAB) {  // (t, u, v) of the hit k_trace found; a repetition that disagrees fails the call (kernels_wavefront.h k_shade)
            h.t = K_INF;
            h.u = h.v = 0.0f;
            if (!prim_hit<CYL>(P, p.o, p.d, K_INF, &h.t, &h.u, &h.v)) atomicAdd(w.guard + WF_GUARD_REHIT, 1u);
        }
        const uint32_t depth = a.depth;
        const V3 tn = {uni[U_TN], uni[U_TN + 1], uni[U_TN + 2]};
        const SI si = make_si<true, CYL>(P, p.o, p.d, h.t, h.u, h.v, has_vn, [&](int k) { return vn.n[k]; });
        const float distance = h.t;                                                   // :314
        p.geo_len += distance;                                                        // :315
        if (!(a.p.quirks & PBRT_USQ_NO_TOF_ACCUM)) p.tof += distance * uni[U_INVC];   // :316
        const uint32_t block = (a.p.quirks & PBRT_USQ_FROZEN_DRAWS) ? 0u : depth;
        const F4 u = rng4(ray_id, k, block, a.seed);
        const uint32_t recv = min((uint32_t)(u.x * (float)NE), NE - 1);               // :319
        float total_time = 0.0f, phase = 0.0f;
        if (TAB) {
            rx = a.first_rx[(size_t)ray_id * NE + recv];
        } else {
            const UsRecv rc = us_receive<CONVEX>(a, uni, si.p, recv);
            p.sdir = rc.sec_dir;
            p.so = offset_origin(si.p, si.n, p.sdir);                                 // :324 (the ray k_trace walks)
            total_time = us_arrival(a, uni[U_INVC], a.p.quirks, ray_id, p.tof, distance, rc.dist_recv);
            phase = uni[U_2PIF] * total_time;                                         // :330
        }
        return us_scatter_step<true, CYL>(a, uni, a.p.quirks, a.sc.mats, P, si, distance, u, ray_id, k, block, depth, tn, p.o, p.d, p.amp,
                                          p.atten, p.geo_len, [&] {
            float fd = 0.0f, carrier = 0.0f;
            if (TAB) {
                fd = rx.x;
                carrier = rx.y;
                p.ci = __float_as_uint(rx.z);                                         // (visibility included)
            } else if (us_echo_bin(NE, T, a.p.quirks, total_time, uni[U_FS], ang, recv, true, &p.ci)) {
                us_echo_weight(a, NE, a.p.quirks, p.d, si.ns, p.sdir, us_recv_normal<CONVEX>(a, uni, recv, tn), uni[U_AM], uni[U_AC], phase, &fd,
                               &carrier);
            }
            p.pressure = p.atten * p.amp * fd * carrier * p.w_ray;                    // :348 (x 1, or the emitter ray's weight: D15)
            if (TAB && p.ci != 0xffffffffu) {  // (else an occlusion ray decides)
                us_echo_deposit(agg_idx, agg_sum, a.channel, p.ci, p.pressure);
                p.ci = 0xffffffffu;
            }
        });
    }
    DEV static bool pending(const Path &p) { return p.ci != 0xffffffffu; }
    DEV void put_survivor(uint32_t out_slot, const Path &p, bool shd_live) const {
        const size_t cp = w.u.cap;
        const float4 q0 = {p.o.x, p.o.y, p.o.z, p.amp}, q1 = {p.d.x, p.d.y, p.d.z, p.atten},
                     q2 = {p.tof, p.geo_len, __uint_as_float(p.home), __uint_as_float(shd_live ? p.ci : 0xffffffffu)},
                     q3 = {shd_live ? p.pressure : 0.0f, p.w_ray, 0.0f, 0.0f};
        w.st_out[out_slot] = q0;
        w.st_out[cp + out_slot] = q1;
        w.st_out[2u * cp + out_slot] = q2;
        w.st_out[3u * cp + out_slot] = q3;
    }
    DEV void end_path(const Path &) const {}
    DEV void put_ray(uint32_t k, uint32_t out_slot, const Path &p) const {
        const float4 q0 = {p.so.x, p.so.y, p.so.z, K_INF}, q1 = {p.sdir.x, p.sdir.y, p.sdir.z, __uint_as_float(out_slot)};
        w.shd_out[k] = q0;
        w.shd_out[w.u.cap + k] = q1;
    }
    DEV void put_dead_ray(uint32_t k, const Path &p) const {  // the path ended at this bounce; its echo still waits for its occlusion ray
        const size_t cp = w.u.cap;
        const float4 q0 = {p.so.x, p.so.y, p.so.z, K_INF}, q1 = {p.sdir.x, p.sdir.y, p.sdir.z, __uint_as_float(WF_DEAD | k)},
                     q2 = {p.pressure, __uint_as_float(p.ci), 0.0f, 0.0f};
        w.shd_out[k] = q0;
        w.shd_out[cp + k] = q1;
        w.shd_out[2u * cp + k] = q2;
    }
    DEV void stats(unsigned long long *row, size_t stride, uint32_t n_seg, uint32_t) const {
        row[0] += n_seg;
        row[stride] += n_seg;  // one occlusion ray per shaded segment (the reference traces one per bounce, :324)
    }
};
template <bool TAB, bool CYL, bool CONVEX = false>
__global__ __launch_bounds__(WF_SHADE_THREADS, WF_SHADE_WAVES_PER_EU) void k_us_shade(const UsWfArgs w) {
    __shared__ uint32_t agg_idx[US_AGG_BINS];
    __shared__ float agg_sum[US_AGG_BINS];
    __shared__ float uni[U_COUNT];
    UsShade<TAB, CYL, CONVEX> m = {w, w.u.p.n_elements, w.u.p.time_samples, agg_idx, agg_sum, uni};
    if (!shade_walk<TAB>(w, w.u, m)) return;  // uniform: an empty region, before any barrier
    __syncthreads();  // all echoes of the workgroup are in the bins (every wave gets here: the walk has no exit after its set-up)
    us_echo_flush(agg_idx, agg_sum, w.u.channel, threadIdx.x, WF_SHADE_THREADS);
}
