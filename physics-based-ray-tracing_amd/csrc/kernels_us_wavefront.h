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
    if (i < n_regions) seg_cnt[i] = a.n_paths > i * WF_REGION ? min(a.n_paths - i * WF_REGION, WF_REGION) : 0u;
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
template <bool TAB, bool CYL, bool CONVEX = false>
__global__ __launch_bounds__(WF_SHADE_THREADS, WF_SHADE_WAVES_PER_EU) void k_us_shade(const UsWfArgs w) {
    constexpr uint32_t T_ = WF_SHADE_THREADS, W = T_ / 64;
    constexpr int NCH = WF_SHADE_CHUNKS;
    const UsArgs &a = w.u;
    __shared__ uint32_t wlist[W][64 * (NCH + 1)], wprim[W][64 * (NCH + 1)];
    __shared__ uint32_t q_out, q_shd, q_dead, q_done;
    __shared__ uint32_t agg_idx[US_AGG_BINS];
    __shared__ float agg_sum[US_AGG_BINS];
    __shared__ float uni[U_COUNT];
    const uint32_t r = w.region0 + xcd_swizzle(blockIdx.x, gridDim.x), base = r * WF_REGION;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t cnt_in = TAB ? (a.n_paths > base ? min(a.n_paths - base, WF_REGION) : 0u) : w.seg_in[r];
    const uint32_t n_dead = (!TAB && w.nsh_in) ? w.nsh_in[r] >> 16 : 0u;
    if (cnt_in == 0 && n_dead == 0) {  // uniform
        if (tid == 0) {
            w.seg_out[r] = 0;
            w.nsh_out[r] = 0;
        }
        return;
    }
    if (tid == 0) {
        q_out = 0;
        q_shd = 0;
        q_dead = 0;
        q_done = 0;
    }
    us_echo_clear(agg_idx, agg_sum, tid, T_);
    us_stage_uniforms(a, uni);  // through LDS as in k_us_bounce: the kernel wants more scalars than a wave has
    __syncthreads();
    const uint32_t NE = a.p.n_elements, T = a.p.time_samples;
    const size_t cp = a.cap;
    // ---- occlusion rays of paths that ended at the previous bounce: their echo, if the ray got through
    for (uint32_t k = tid; k < n_dead; k += T_) {
        const float4 rec = w.shd_in[2u * cp + (base + WF_REGION - n_dead + k)];
        if (rec.w != 0.0f) us_echo_deposit(agg_idx, agg_sum, a.channel, __float_as_uint(rec.y), rec.x);
    }
    uint32_t list_n = 0, n_seg_w = 0;
    uint32_t c0 = wid * 64u;
    for (;;) {
        if (c0 < cnt_in) {
            // WF_SHADE_CHUNKS chunks per step, their loads in one batch (kernels_wavefront.h k_shade)
            uint32_t hidv[NCH];
            float4 q2v[NCH], q3v[NCH];
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const uint32_t s = c0 + (uint32_t)j * (W * 64u) + lane;
                hidv[j] = 0xffffffffu;
                q2v[j] = q3v[j] = float4{0.0f, 0.0f, 0.0f, 0.0f};
                if (s < cnt_in) {
                    if (TAB) {
                        const uint32_t ray_id = udiv_fast(base + s, a.div_ppr);
                        hidv[j] = __float_as_uint(a.first_hit[ray_id].w);  // the primitive the ray's shared first hit lies on
                    } else {
                        hidv[j] = w.hit_id[base + s];
                        q2v[j] = w.st_in[2u * cp + base + s];
                        q3v[j] = w.st_in[3u * cp + base + s];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const uint32_t s = c0 + (uint32_t)j * (W * 64u) + lane;
                const uint32_t hid = hidv[j];
                // the pending echo of the previous bounce (every path, whether it goes on or not)
                if (!TAB && s < cnt_in && q3v[j].w != 0.0f && __float_as_uint(q2v[j].w) != 0xffffffffu)
                    us_echo_deposit(agg_idx, agg_sum, a.channel, __float_as_uint(q2v[j].w), q3v[j].x);
                const bool is_hit = hid != 0xffffffffu;
                const unsigned long long bh = __ballot(is_hit);
                if (is_hit) {
                    const uint32_t e = list_n + __builtin_amdgcn_mbcnt_hi((uint32_t)(bh >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bh, 0u));
                    wlist[wid][e] = s;
                    wprim[wid][e] = hid;
                }
                list_n += (uint32_t)__popcll(bh);
            }
            __builtin_amdgcn_wave_barrier();
            c0 += (uint32_t)NCH * W * 64u;
        } else if (list_n == 0) {
            break;
        }
        if (list_n < 64u && c0 < cnt_in) continue;
        // ---- shade 64 listed paths: the bounce from the hit on, through the pieces of kernels_us.h that k_us_bounce runs (the list is
        // emptied below 64 entries before the wave reads its next chunks)
        for (;;) {
        const uint32_t take = min(list_n, 64u);
        const bool act = lane < take;
        list_n -= take;
        bool survive = false, pend = false;
        V3 o = {0, 0, 0}, d = {0, 0, 1}, so = {0, 0, 0}, sdir = {0, 0, 1};
        float amp = 1.0f, atten = 1.0f, tof = 0.0f, geo_len = 0.0f, pressure = 0.0f, w_ray = 1.0f;
        uint32_t home = 0, ci = 0xffffffffu;
        if (act) {
            const uint32_t s = wlist[wid][list_n + lane];
            Hit h;
            h.slot = wprim[wid][list_n + lane];
            h.prim = h.slot;
            uint32_t ray_id, k, ang;
            float4 rx = {0.0f, 0.0f, 0.0f, 0.0f};
            if (TAB) {
                home = base + s;
                ray_id = udiv_fast(home, a.div_ppr);
                k = a.path_first + (home - ray_id * a.ppr_pass);
                ang = udiv_fast(ray_id, a.div_ne);
                const uint32_t el = ray_id - ang * NE;
                o = us_elem_point<CONVEX>(a, uni, el);                                   // :270,273
                d = v3(a.dir0[3 * ang], a.dir0[3 * ang + 1], a.dir0[3 * ang + 2]);        // :271,273
                const float4 fh = a.first_hit[ray_id];
                h.t = fh.x;
                h.u = fh.y;
                h.v = fh.z;
            } else {
                const float4 q0 = w.st_in[base + s], q1 = w.st_in[cp + base + s], q2 = w.st_in[2u * cp + base + s];
                // the weight of the path's primary ray rides in q3.y (k_us_init_wf); it is 1 unless the rays come from the emitter, so
                // only that mode reads it
                if (a.p.primary == PBRT_US_PRIMARY_EMITTER) w_ray = w.st_in[3u * cp + base + s].y;
                o = {q0.x, q0.y, q0.z};
                amp = q0.w;
                d = {q1.x, q1.y, q1.z};
                atten = q1.w;
                tof = q2.x;
                geo_len = q2.y;
                home = __float_as_uint(q2.z);
                ray_id = udiv_fast(home, a.div_ppr);
                k = a.path_first + (home - ray_id * a.ppr_pass);
                ang = udiv_fast(ray_id, a.div_ne);
            }
            const pbrt_prim P = wf_load_prim(a.sc.prims + h.slot);
            const bool has_vn = a.sc.vnormals != nullptr;  // uniform
            WfVn vn;
            if (has_vn) vn = wf_load_vn(a.sc.vnormals, h.slot);
            if (!TAB) {  // (t, u, v) of the hit k_trace found; a repetition that disagrees fails the call (kernels_wavefront.h k_shade)
                h.t = K_INF;
                h.u = h.v = 0.0f;
                if (!prim_hit<CYL>(P, o, d, K_INF, &h.t, &h.u, &h.v)) atomicAdd(w.guard + WF_GUARD_REHIT, 1u);
            }
            const uint32_t depth = a.depth;
            const V3 tn = {uni[U_TN], uni[U_TN + 1], uni[U_TN + 2]};
            const SI si = make_si<true, CYL>(P, o, d, h.t, h.u, h.v, has_vn, [&](int k) { return vn.n[k]; });
            const float distance = h.t;                                                   // :314
            geo_len += distance;                                                          // :315
            if (!(a.p.quirks & PBRT_USQ_NO_TOF_ACCUM)) tof += distance * uni[U_INVC];     // :316
            const uint32_t block = (a.p.quirks & PBRT_USQ_FROZEN_DRAWS) ? 0u : depth;
            const F4 u = rng4(ray_id, k, block, a.seed);
            const uint32_t recv = min((uint32_t)(u.x * (float)NE), NE - 1);               // :319
            float total_time = 0.0f, phase = 0.0f;
            if (TAB) {
                rx = a.first_rx[(size_t)ray_id * NE + recv];
            } else {
                const UsRecv rc = us_receive<CONVEX>(a, uni, si.p, recv);
                sdir = rc.sec_dir;
                so = offset_origin(si.p, si.n, sdir);                                     // :324 (the ray k_trace walks)
                total_time = us_arrival(a, uni[U_INVC], a.p.quirks, ray_id, tof, distance, rc.dist_recv);
                phase = uni[U_2PIF] * total_time;                                         // :330
            }
            survive = us_scatter_step<true, CYL>(a, uni, a.p.quirks, a.sc.mats, P, si, distance, u, ray_id, k, block, depth, tn, o, d, amp, atten,
                                                 geo_len, [&] {
                float fd = 0.0f, carrier = 0.0f;
                if (TAB) {
                    fd = rx.x;
                    carrier = rx.y;
                    ci = __float_as_uint(rx.z);                                           // (visibility included)
                } else if (us_echo_bin(NE, T, a.p.quirks, total_time, uni[U_FS], ang, recv, true, &ci)) {
                    us_echo_weight(a, NE, a.p.quirks, d, si.ns, sdir, us_recv_normal<CONVEX>(a, uni, recv, tn), uni[U_AM], uni[U_AC], phase, &fd,
                                   &carrier);
                }
                pressure = atten * amp * fd * carrier * w_ray;                            // :348 (x 1, or the emitter ray's weight: D15)
                if (ci != 0xffffffffu) {
                    if (TAB) {
                        us_echo_deposit(agg_idx, agg_sum, a.channel, ci, pressure);
                        ci = 0xffffffffu;
                    } else {
                        pend = true;  // an occlusion ray decides
                    }
                }
            });
        }
        n_seg_w += take;
        // survivors -> front of the region of the `out` state
        const unsigned long long bs = __ballot(survive);
        uint32_t out_slot = 0;
        if (bs) {
            uint32_t got = 0;
            if (lane == 0) got = atomicAdd(&q_out, (uint32_t)__popcll(bs));
            const uint32_t off = (uint32_t)__builtin_amdgcn_readfirstlane((int)got);
            out_slot = base + off + __builtin_amdgcn_mbcnt_hi((uint32_t)(bs >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bs, 0u));
        }
        const bool shd_live = pend && survive, shd_dead = pend && !survive;
        if (survive) {
            const float4 q0 = {o.x, o.y, o.z, amp}, q1 = {d.x, d.y, d.z, atten},
                         q2 = {tof, geo_len, __uint_as_float(home), __uint_as_float(shd_live ? ci : 0xffffffffu)},
                         q3 = {shd_live ? pressure : 0.0f, w_ray, 0.0f, 0.0f};
            w.st_out[out_slot] = q0;
            w.st_out[cp + out_slot] = q1;
            w.st_out[2u * cp + out_slot] = q2;
            w.st_out[3u * cp + out_slot] = q3;
        }
        const unsigned long long bl = __ballot(shd_live);
        if (bl) {
            uint32_t got = 0;
            if (lane == 0) got = atomicAdd(&q_shd, (uint32_t)__popcll(bl));
            const uint32_t off = (uint32_t)__builtin_amdgcn_readfirstlane((int)got);
            if (shd_live) {
                const uint32_t k = base + off + __builtin_amdgcn_mbcnt_hi((uint32_t)(bl >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bl, 0u));
                const float4 q0 = {so.x, so.y, so.z, K_INF}, q1 = {sdir.x, sdir.y, sdir.z, __uint_as_float(out_slot)};
                w.shd_out[k] = q0;
                w.shd_out[cp + k] = q1;
            }
        }
        const unsigned long long bd = __ballot(shd_dead);
        if (bd) {  // the path ended at this bounce; its echo still waits for its occlusion ray
            uint32_t got = 0;
            if (lane == 0) got = atomicAdd(&q_dead, (uint32_t)__popcll(bd));
            const uint32_t off = (uint32_t)__builtin_amdgcn_readfirstlane((int)got);
            if (shd_dead) {
                const uint32_t k =
                    base + WF_REGION - 1u - (off + __builtin_amdgcn_mbcnt_hi((uint32_t)(bd >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bd, 0u)));
                const float4 q0 = {so.x, so.y, so.z, K_INF}, q1 = {sdir.x, sdir.y, sdir.z, __uint_as_float(WF_DEAD | k)},
                             q2 = {pressure, __uint_as_float(ci), 0.0f, 0.0f};
                w.shd_out[k] = q0;
                w.shd_out[cp + k] = q1;
                w.shd_out[2u * cp + k] = q2;
            }
        }
        if (list_n < 64u && c0 < cnt_in) break;  // room for the next chunks
        if (list_n == 0u) break;
        }  // shading steps
    }
    if (lane == 0) {
        unsigned long long *row = a.stats + (size_t)r * W + wid;  // per-wave statistics rows
        const size_t stride = a.stat_stride;
        row[0] += n_seg_w;
        row[stride] += n_seg_w;  // one occlusion ray per shaded segment (the reference traces one per bounce, :324)
        if (wid == 0) row[(2 + min(a.depth, (uint32_t)MAX_DEPTH_STATS - 1)) * stride] += cnt_in;
        if (atomicAdd(&q_done, 1u) == W - 1) {
            w.seg_out[r] = atomicAdd(&q_out, 0u);
            w.nsh_out[r] = atomicAdd(&q_shd, 0u) | (atomicAdd(&q_dead, 0u) << 16);
        }
    }
    __syncthreads();  // all echoes of the workgroup are in the bins (every wave gets here: no exit after the set-up)
    us_echo_flush(agg_idx, agg_sum, a.channel, tid, T_);
}
