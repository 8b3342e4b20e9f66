// kernels_wavefront_shade.inc -- the body of k_shade and k_shade_glossy (kernels_wavefront.h includes it once for each, behind the
// kernel's template head and signature, with WF_SHADE_GLOSSY defined).  One text, two kernels: the instances of k_shade stay the
// code they were, instruction for instruction, which a body shared through a device function did not give, and keep their mangled
// names, which a fourth template parameter would not (tests/test_fp_short_forms_asm.py finds them by name; DESIGN.md D17).
{
    constexpr bool GLOSSY = WF_SHADE_GLOSSY;
    constexpr uint32_t T = WF_SHADE_THREADS, W = T / 64;
    constexpr int NCH = WF_SHADE_CHUNKS;  // chunks of 64 hit indices a wave reads per step
    // per wave: the paths that hit something and wait for a full wave -- slot within the region, and the primitive that was hit
    __shared__ uint32_t wlist[W][64 * (NCH + 1)], wprim[W][64 * (NCH + 1)];
    // ... and (bounces >= 1) its radiance so far with the pending shadow contribution folded in, and its home: the chunk phase streams
    // the L / A / B planes of EVERY path of the chunk anyway (a path that missed needs them to end), so a path that hit keeps what
    // they amount to -- L = fma(A, B, L), home -- on the list instead of gathering the three planes again in the shading step:
    // 48 of the 96 gathered bytes per hit, at 128-byte lines for 16-byte records (round 4: traffic 1.25 x the model)
    __shared__ float4 wlh[FIRST ? 1 : W][FIRST ? 1 : 64 * (NCH + 1)];
    __shared__ uint32_t q_out, q_shd, q_dead, q_done;
    __shared__ uint32_t tab_lds[TABS ? WF_TAB_DW : 1];
    const uint32_t r = a.region0 + xcd_swizzle(blockIdx.x, gridDim.x), base = r * WF_REGION;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t cnt_in = FIRST ? (a.n_paths > base ? min(a.n_paths - base, WF_REGION) : 0u) : a.seg_in[r];
    const uint32_t n_dead = (!FIRST && a.nsh_in) ? a.nsh_in[r] >> 16 : 0u;
    if (cnt_in == 0 && n_dead == 0) {  // uniform
        if (tid == 0) {
            a.seg_out[r] = 0;
            a.nsh_out[r] = 0;
        }
        return;
    }
    if (tid == 0) {
        q_out = 0;
        q_shd = 0;
        q_dead = 0;
        q_done = 0;
    }
    const Tables tb = TABS ? wf_tables_lds(a.sc, tab_lds, T) : global_tables(a.sc);
    __syncthreads();  // the only barrier
    float4 *Lh = reinterpret_cast<float4 *>(a.Lhome);
    // ---- shadow rays of paths that ended at the previous bounce: L = fma(A, B, L) on the radiance record
    for (uint32_t k = tid; k < n_dead; k += T) {
        const float4 *rec = a.shd_in + (base + WF_REGION - n_dead + k);
        const float4 A = rec[2u * (size_t)a.cap], B = rec[3u * (size_t)a.cap];
        if (A.w != 0.0f) {
            float4 *Lp = Lh + __float_as_uint(B.w);
            float4 Lv = *Lp;
            Lv.x = fma_(A.x, B.x, Lv.x);
            Lv.y = fma_(A.y, B.y, Lv.y);
            Lv.z = fma_(A.z, B.z, Lv.z);
            *Lp = Lv;
        }
    }
    uint32_t list_n = 0;             // wave-uniform: entries on this wave's list
    uint32_t n_seg_w = 0, n_shd_w = 0;
    uint32_t c0 = wid * 64u;         // the wave's next chunk of the region
    for (;;) {
        if (c0 < cnt_in) {
            // ---- WF_SHADE_CHUNKS chunks of hit records: paths whose ray left the scene end here, the others go on the list.  One
            // batch of loads: the hit indices and (bounces >= 1) the three state planes a path that ends needs.
            uint32_t hidv[NCH];
            float4 q3v[NCH], q4v[NCH], q5v[NCH];
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const uint32_t s = c0 + (uint32_t)j * (W * 64u) + lane;
                hidv[j] = 0xffffffffu;
                q3v[j] = q4v[j] = q5v[j] = float4{0, 0, 0, 0};
                if (s < cnt_in) {
                    hidv[j] = a.hit_id[base + s];
                    if (!FIRST) {
                        const float4 *stp = a.st_in + (base + s);
                        const size_t cp = a.cap;
                        q3v[j] = stp[3u * cp];
                        q4v[j] = stp[4u * cp];
                        q5v[j] = stp[5u * cp];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const uint32_t s = c0 + (uint32_t)j * (W * 64u) + lane;
                const bool valid = s < cnt_in;
                const uint32_t hid = hidv[j];
                const float4 q3 = q3v[j], q4 = q4v[j], q5 = q5v[j];
                const bool is_hit = hid != 0xffffffffu;
                float4 Lv = q3;
                if (!FIRST && q4.w != 0.0f) {  // its shadow ray of the previous bounce got through
                    Lv.x = fma_(q4.x, q5.x, Lv.x);
                    Lv.y = fma_(q4.y, q5.y, Lv.y);
                    Lv.z = fma_(q4.z, q5.z, Lv.z);
                }
                if (valid && !is_hit) {
                    float4 rec = Lv;
                    rec.w = 0.0f;
                    Lh[FIRST ? base + s : __float_as_uint(q3.w)] = rec;
                }
                const unsigned long long bh = __ballot(is_hit);
                if (is_hit) {
                    const uint32_t e = list_n + __builtin_amdgcn_mbcnt_hi((uint32_t)(bh >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bh, 0u));
                    wlist[wid][e] = s;
                    wprim[wid][e] = hid;
                    if (!FIRST) wlh[wid][e] = Lv;  // (L with the pending contribution, home in .w)
                }
                list_n += (uint32_t)__popcll(bh);
            }
            __builtin_amdgcn_wave_barrier();  // other lanes of the wave read these entries below (LDS operations of a wave stay in order)
            c0 += (uint32_t)NCH * W * 64u;
        } else if (list_n == 0) {
            break;
        }
        if (list_n < 64u && c0 < cnt_in) continue;
        // ---- shade 64 listed paths (or what is left at the end) with every lane busy; the list is emptied below 64 entries before
        // the wave reads its next chunks (the list holds 64 x (WF_SHADE_CHUNKS + 1))
        for (;;) {
        const uint32_t take = min(list_n, 64u);
        const bool act = lane < take;
        list_n -= take;
        bool survive = false;
        WfShadow sh;
        sh.on = false;
        V3 o = {0, 0, 0}, d = {0, 0, 1}, thr = {1, 1, 1}, L = {0, 0, 0};
        float eta = 1.0f, prev_pdf = -1.0f;
        uint32_t home = 0;
        if (act) {
            const uint32_t s = wlist[wid][list_n + lane];
            Hit h;
            h.prim = wprim[wid][list_n + lane];
            h.slot = h.prim;
            // one batch of loads: the primitive's record, its vertex normals, the path state.  (t, u, v) of the hit are not carried
            // through memory: k_trace hands over the primitive it found, and the test of THAT primitive against the ray is repeated
            // here -- the same arithmetic on the same operands (a leaf record is the first nine floats of this record), so the same
            // bits, for 60 VALU instructions of a kernel that waits on HBM instead of a 16-byte record written scattered (a 32-byte
            // sector each) and gathered back (a 128-byte line each at the later bounces).
            const pbrt_prim P = wf_load_prim(tb.prims_by_slot + h.slot);
            const bool has_vn = a.sc.vnormals != nullptr;  // uniform
            WfVn vn;
            if (has_vn) vn = wf_load_vn(a.sc.vnormals, h.slot);
            uint32_t ka, kb;
            if (FIRST) {
                float tm;
                home = base + s;
                wf_camera_ray(a, home, &o, &d, &tm, &ka, &kb);
            } else {
                const float4 *stp = a.st_in + (base + s);
                const size_t cp = a.cap;
                const float4 q0 = stp[0], q1 = stp[cp], q2 = stp[2u * cp];
                const float4 lh = wlh[FIRST ? 0 : wid][FIRST ? 0 : list_n + lane];  // L (pending shadow contribution included), home
                o = {q0.x, q0.y, q0.z};
                d = {q1.x, q1.y, q1.z};
                thr = {q2.x, q2.y, q2.z};
                L = {lh.x, lh.y, lh.z};
                eta = (a.key_mode == 1 && a.depth == 0) ? 1.0f : q0.w;  // caller rays carry tmax in the eta slot
                prev_pdf = q1.w;
                home = __float_as_uint(lh.w);
                uint32_t px, py;
                const RadArgs ra = wf_key_args(a);
                path_key<true>(ra, home, &ka, &kb, &px, &py);
            }
            // (t, u, v) of the hit k_trace found: the same test on the same operands (a leaf record is the first nine floats of P).
            // Should the repetition ever disagree (other build flags, another code path for the primitive) the call fails with
            // PBRT_E_DEVICE instead of shading with whatever the registers held: guard word WF_GUARD_REHIT counts the cases.
            h.t = K_INF;
            h.u = h.v = 0.0f;
            if (!prim_hit<CYL>(P, o, d, K_INF, &h.t, &h.u, &h.v)) atomicAdd(a.guard + WF_GUARD_REHIT, 1u);
            const SI si = make_si<true, CYL>(P, o, d, h.t, h.u, h.v, has_vn, [&](int k) { return vn.n[k]; });
            // the bounce's arithmetic (kernels_radiance.h shade_step), its shadow segment handed out instead of traced
            survive = shade_step<GLOSSY>(
                a, tb, a.depth, ka, kb, h.t, P, si, o, d, thr, L, eta, prev_pdf,
                [&](V3 so, V3 sdir, float smax) {
                    sh.on = true;
                    sh.so = so;
                    sh.sdir = sdir;
                    sh.tmax = smax;
                    return true;
                },
                [&](V3 A, V3 B) {
                    sh.A = A;
                    sh.B = B;
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
        const bool shd_live = sh.on && survive, shd_dead = sh.on && !survive;
        if (survive) {
            float4 *stp = a.st_out + out_slot;
            const size_t cp = a.cap;
            const float4 q0 = {o.x, o.y, o.z, eta}, q1 = {d.x, d.y, d.z, prev_pdf}, q2 = {thr.x, thr.y, thr.z, 0.0f},
                         q3 = {L.x, L.y, L.z, __uint_as_float(home)};
            stp[0] = q0;
            stp[cp] = q1;
            stp[2u * cp] = q2;
            stp[3u * cp] = q3;
            const float4 q4 = {shd_live ? sh.A.x : 0.0f, shd_live ? sh.A.y : 0.0f, shd_live ? sh.A.z : 0.0f, 0.0f},
                         q5 = {shd_live ? sh.B.x : 0.0f, shd_live ? sh.B.y : 0.0f, shd_live ? sh.B.z : 0.0f, 0.0f};
            stp[4u * cp] = q4;
            stp[5u * cp] = q5;
        } else if (act) {  // the path ends (a pending shadow ray is added to this record by the next k_shade)
            const float4 rec = {L.x, L.y, L.z, 0.0f};
            Lh[home] = rec;
        }
        const unsigned long long bl = __ballot(shd_live);
        if (bl) {
            uint32_t got = 0;
            if (lane == 0) got = atomicAdd(&q_shd, (uint32_t)__popcll(bl));
            const uint32_t off = (uint32_t)__builtin_amdgcn_readfirstlane((int)got);
            n_shd_w += (uint32_t)__popcll(bl);
            if (shd_live) {
                const uint32_t k = base + off + __builtin_amdgcn_mbcnt_hi((uint32_t)(bl >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bl, 0u));
                float4 *rec = a.shd_out + k;
                const float4 q0 = {sh.so.x, sh.so.y, sh.so.z, sh.tmax}, q1 = {sh.sdir.x, sh.sdir.y, sh.sdir.z, __uint_as_float(out_slot)};
                rec[0] = q0;
                rec[a.cap] = q1;
            }
        }
        const unsigned long long bd = __ballot(shd_dead);
        if (bd) {  // rare: Russian roulette ended a path that had just sent a shadow ray
            uint32_t got = 0;
            if (lane == 0) got = atomicAdd(&q_dead, (uint32_t)__popcll(bd));
            const uint32_t off = (uint32_t)__builtin_amdgcn_readfirstlane((int)got);
            n_shd_w += (uint32_t)__popcll(bd);
            if (shd_dead) {
                const uint32_t k =
                    base + WF_REGION - 1u - (off + __builtin_amdgcn_mbcnt_hi((uint32_t)(bd >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bd, 0u)));
                float4 *rec = a.shd_out + k;
                const size_t cp = a.cap;
                const float4 q0 = {sh.so.x, sh.so.y, sh.so.z, sh.tmax},
                             q1 = {sh.sdir.x, sh.sdir.y, sh.sdir.z, __uint_as_float(WF_DEAD | k)},
                             q2 = {sh.A.x, sh.A.y, sh.A.z, 0.0f}, q3 = {sh.B.x, sh.B.y, sh.B.z, __uint_as_float(home)};
                rec[0] = q0;
                rec[cp] = q1;
                rec[2u * cp] = q2;
                rec[3u * cp] = q3;
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
        row[stride] += n_shd_w;
        row[(HIT_ROW0 + min(a.depth, (uint32_t)MAX_DEPTH_STATS - 1)) * stride] += n_seg_w;  // hits of this depth (byte model)
        if (wid == 0) row[(2 + min(a.depth, (uint32_t)MAX_DEPTH_STATS - 1)) * stride] += cnt_in;
        // the last wave to finish publishes the region's counts (LDS atomics of one CU are ordered)
        if (atomicAdd(&q_done, 1u) == W - 1) {
            a.seg_out[r] = atomicAdd(&q_out, 0u);
            a.nsh_out[r] = atomicAdd(&q_shd, 0u) | (atomicAdd(&q_dead, 0u) << 16);
        }
    }
}
