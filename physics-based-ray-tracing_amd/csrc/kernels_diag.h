// kernels_diag.h -- kernels of the diagnostic build only (make diag, -DPBRT_DIAG -> libpbrt_hip_diag.so).
//
// Launch structures that lost their A/B: k_chain_pair, k_walk, k_regen, and the repack pass (k_scan_owners,
// k_repack_copy) of the fused BVH bounce kernels (k_bounce<.., BVH>, whose template text is kernels_radiance.h's).  The product
// library does not carry them; diag_driver.h launches them.  Included after the product kernel headers.
#pragma once
#include "kernels_radiance.h"

// ---- k_chain_pair: the whole path in one launch, TWO 64-path tiles per wave ---------------------------------------------------
// A chain launch keeps a wave busy until the longest of its 64 paths has ended: in the Cornell box 100 / 87 / 67 / 56 / 47 / 9 % of
// the lanes carry a path at bounces 0 .. 5, and a bounce costs a wave the same whether 64 or 6 of its lanes are live.  Here a wave
// walks tile A up to bounce a.merge_at, parks the survivors in a wave-private LDS strip (N_STATE dwords each, packed), walks tile B
// up to the same bounce, deals the parked paths to B's idle lanes and walks the rest of both tiles ONCE.  Parked paths that find no
// idle lane (more than 64 survivors in the pair) are walked afterwards in a turn of their own.  Every path does the arithmetic it
// did before with the same RNG keys (path_key of its home), so the film does not change.  The strip is only touched by its own wave:
// LDS operations of one wave complete in order, no barrier.
// Measured (Cornell box 512^2 x 256, one launch per pass): k_bounce chain 6.02 - 6.07 ms; this kernel with merge bounce 3 / 4 / 5:
// 6.37 / 6.43 - 6.55 / 6.48 ms.  Merging at bounce 5 merges nothing that costs (the last bounce only looks for emitters), so 6.48 is
// the price of the structure itself (12 spilled VGPRs and 50 spilled SGPRs at the 64-register budget, against 1 and 13), and the
// merge buys 0.1 ms of the 0.6 - 0.8 ms that the count of wave-bounces promises: a wave with half of its lanes idle skips the
// branches that none of its paths takes, a full wave of paths from two tiles takes them all.  Diagnostic build only
// (PBRT_PAIR_MERGE=k picks the merge bounce).
// Host: max_depth <= MAX_CHAIN (every path ends inside the launch: no state goes out), 1 <= merge_at < max_depth,
// grid = ceil(n_paths / (2 * SEG_BRUTE)).
// row k of entry r of the wave's strip pk (get / put of STATE_LOAD / STATE_STORE)
#define PARK_GET(k) __uint_as_float(pk[k][r])
#define PARK_PUT(k, v) pk[k][r] = __float_as_uint(v)
template <int ACCEL>
__global__ __launch_bounds__(SEG_BRUTE, ACCEL == ACCEL_K_BRUTE ? FUSED_WAVES_PER_EU : BIG_WAVES_PER_EU) void k_chain_pair(const RadArgs a) {
    static_assert(ACCEL == ACCEL_K_BRUTE || ACCEL == ACCEL_K_BRUTE_BIG, "k_chain_pair: brute-force kernels");
    constexpr uint32_t SEG = SEG_BRUTE, W = SEG / 64;
    __shared__ uint32_t tab_lds[ACCEL == ACCEL_K_BRUTE ? TAB_DW : 1];
    __shared__ uint32_t park[W][N_STATE][64];
    __shared__ uint32_t wave_cnt[W][2 + MAX_CHAIN];  // per wave: segments, shadow rays, paths entering bounce b (lane 0 adds)
    const uint32_t region = xcd_swizzle(blockIdx.x, gridDim.x);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const LdsScene ls = NO_LDS_SCENE;
    const Tables tb = make_tables<ACCEL>(a.sc, ls, tab_lds);
    if (ACCEL == ACCEL_K_BRUTE) fill_tables_lds(a.sc, tab_lds, SEG);  // ends with a barrier
    const Rsrc r_L = make_rsrc(a.Lhome, a.cap * 16u);
    uint32_t(*pk)[64] = park[wid];
    const uint32_t tile0 = (region * W + wid) * 2u;
    const uint32_t m = a.merge_at;
    // four turns (wave-uniform): 0 = tile A up to the merge bounce, 1 = tile B likewise, 2 = both from there on, 3 = parked paths
    // that found no lane
    uint32_t n_park = 0, left0 = 0, n_left = 0;
    if (lane < 2u + MAX_CHAIN) wave_cnt[wid][lane] = 0u;
    V3 o = {0, 0, 0}, d = {0, 0, 1}, thr = {0, 0, 0}, L = {0, 0, 0};
    float eta = 1.0f, prev_pdf = -1.0f, tmax = K_INF;
    uint32_t home = 0, ka = 0, kb = 0;
    bool live = false;
#pragma unroll 1
    for (uint32_t turn = 0; turn < 4u; ++turn) {
        uint32_t b_first = 0, b_end = m;
        if (turn < 2u) {  // the camera paths of the tile
            const uint32_t slot = (tile0 + turn) * 64u + lane;
            live = slot < a.n_paths;
            home = slot;
            if (live) camera_start(a, home, &ka, &kb, &o, &d, &tmax, &thr, &L, &eta, &prev_pdf);
        } else {
            // turn 2: the parked paths go to the idle lanes of tile B, in order; turn 3: those that found none, from lane 0 on
            // (every lane is idle by then)
            if (turn == 3u && n_left == 0u) break;
            const unsigned long long idle = ~__ballot(live);
            const uint32_t rank = ballot_rank(idle);
            uint32_t n_take;
            if (turn == 2u) {
                n_take = min(n_park, (uint32_t)__popcll(idle));
                left0 = n_take;
                n_left = n_park - n_take;
            } else {
                n_take = n_left;
            }
            const uint32_t r = (turn == 2u ? 0u : left0) + rank;
            if (!live && rank < n_take) {
                STATE_LOAD(PARK_GET, o, d, thr, L, eta, prev_pdf, home);
                uint32_t px, py;
                path_key(a, home, &ka, &kb, &px, &py);
                live = true;
            }
            b_first = m;
            b_end = a.max_depth;
        }
#pragma unroll 1
        for (uint32_t bounce = b_first; bounce < b_end; ++bounce) {
            const uint32_t n_on = (uint32_t)__popcll(__ballot(live));
            if (n_on == 0u) break;
            if (lane == 0u) atomicAdd(&wave_cnt[wid][2u + bounce], n_on);
            if (bounce > 0u) tmax = K_INF;
            bool did_seg = false, did_shadow = false, survive = false;
            if (live) survive = bounce_step<ACCEL>(a, tb, ls, r_L, bounce, ka, kb, home, tmax, o, d, thr, L, eta, prev_pdf, did_seg, did_shadow);
            live = survive;
            const uint32_t n_sg = (uint32_t)__popcll(__ballot(did_seg)), n_sh = (uint32_t)__popcll(__ballot(did_shadow));
            if (lane == 0u) {
                atomicAdd(&wave_cnt[wid][0], n_sg);
                atomicAdd(&wave_cnt[wid][1], n_sh);
            }
        }
        if (turn == 0u) {  // park the survivors of tile A
            const unsigned long long bal = __ballot(live);
            n_park = (uint32_t)__popcll(bal);
            if (live) {
                const uint32_t r = ballot_rank(bal);
                STATE_STORE(PARK_PUT, o, d, thr, L, eta, prev_pdf, home);
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long *row = a.stats + region;
        const size_t stride = a.stat_stride;
        for (uint32_t k = 0; k < 2u + a.max_depth; ++k) {
            uint32_t n = 0;
            for (uint32_t w = 0; w < W; ++w) n += wave_cnt[w][k];
            row[k * stride] += n;
        }
    }
}

// ---- k_walk: ONE launch walks every remaining bounce (brute-force kernels) -----------------------------------------------
// Compaction is local to the segment, so nothing forces a grid-wide barrier between bounces: the workgroup that owns a
// segment carries its survivors from bounce to bounce on its own, ping-ponging between the two state buffers (release
// fence + workgroup barrier between bounces).  What it saves over one launch per bounce: the drain and ramp of every
// launch, the launches of the late depths in which most workgroups only find an empty segment, and most of the state
// READS -- the survivors a workgroup wrote a few microseconds ago are still in its XCD's L2.  Waves whose slots lie
// beyond the live prefix can never get work again (the prefix only shrinks) and leave for good.  The first trip of the
// loop may walk NB0 = 2 bounces in registers like k_bounce<.., 2>.  Same arithmetic, same keys: the film does not change.
#ifndef WALK_WAVES_PER_EU
#define WALK_WAVES_PER_EU 4
#endif
template <bool FIRST, int ACCEL, int NB0>
__global__ __launch_bounds__(SEG_BRUTE, WALK_WAVES_PER_EU) void k_walk(const RadArgs a) {
    static_assert(ACCEL == ACCEL_K_BRUTE || ACCEL == ACCEL_K_BRUTE_BIG, "k_walk: brute-force kernels only");
    constexpr uint32_t SEG = SEG_BRUTE, W = SEG / 64;
    __shared__ uint32_t wave_tot[2][W], wave_seg[2][W], wave_shd[2][W], wave_mid[2][W];  // double-buffered over the bounces
    __shared__ uint32_t tab_lds[ACCEL == ACCEL_K_BRUTE ? TAB_DW : 1];
    const uint32_t seg = xcd_swizzle(blockIdx.x, gridDim.x), tid = threadIdx.x, wid = tid >> 6, base = seg * SEG;
    uint32_t cnt_in = FIRST ? (a.n_paths > base ? min(a.n_paths - base, SEG) : 0u) : a.seg_in[seg];
    if (cnt_in == 0) {  // uniform across the workgroup
        if (tid == 0) a.seg_out[seg] = 0;
        return;
    }
    const uint32_t wave_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)tid) & ~63u;
    // a wave that leaves has published zero counts in both buffers first; s_barrier does not wait for terminated waves,
    // and it does wait for a wave that has neither arrived nor terminated, so the zeros are in place before anybody scans
    auto leave_wave = [&](uint32_t cnt) {
        if ((tid & 63u) == 0 && wave_first >= cnt) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                wave_tot[b][wid] = 0;
                wave_seg[b][wid] = 0;
                wave_shd[b][wid] = 0;
                wave_mid[b][wid] = 0;
            }
        }
        leave_if_idle(wave_first, cnt);
    };
    leave_wave(cnt_in);
    const uint32_t live_threads = (min(cnt_in, SEG) + 63u) & ~63u;  // waves present at the first trip
    const LdsScene ls = NO_LDS_SCENE;
    const Tables tb = make_tables<ACCEL>(a.sc, ls, tab_lds);
    if (ACCEL == ACCEL_K_BRUTE && FIRST) fill_tables_lds(a.sc, tab_lds, live_threads);
    const uint32_t cap = a.cap;
    Rsrc r_in = make_rsrc(a.in, a.state_cap * (N_STATE * 4u)), r_out = make_rsrc(a.out, a.state_cap * (N_STATE * 4u));
    const Rsrc r_L = make_rsrc(a.Lhome, cap * 16u);
    uint32_t depth = a.depth, trip = 0, left = 0;
    uint32_t ns_acc = 0, nh_acc = 0;
    for (;;) {
        const uint32_t buf = trip & 1u;
        const bool first = FIRST && trip == 0;
        const bool alive = tid < cnt_in;
        const uint32_t slot = base + tid;
        bool survive = false, did_seg = false, did_shadow = false;
        V3 o = {0, 0, 0}, d = {0, 0, 1}, thr = {1, 1, 1}, L = {0, 0, 0};
        float eta = 1.0f, prev_pdf = -1.0f, tmax = K_INF;
        uint32_t home = slot, ka = 0, kb = 0, px = 0, py = 0;
        if (alive) {
            if (first) {
                camera_start(a, home, &ka, &kb, &o, &d, &tmax);
            } else {
                const uint32_t v4 = state_voff(slot);
                constexpr uint32_t row = STATE_ROW_BYTES;
                STATE_LOAD(STATE_BLD, o, d, thr, L, eta, prev_pdf, home);
            }
        }
        // shading tables -> LDS, behind the state loads of the first trip so that the two memory round trips overlap
        if (ACCEL == ACCEL_K_BRUTE && !FIRST && trip == 0) fill_tables_lds(a.sc, tab_lds, live_threads);
        if (alive && !first) path_key(a, home, &ka, &kb, &px, &py);
        const uint32_t nb = (trip == 0) ? (uint32_t)NB0 : 1u;
        bool live = alive;
        uint32_t nseg_w = 0, nshd_w = 0, nmid_w = 0;
#pragma unroll 1
        for (uint32_t bounce = 0; bounce < nb; ++bounce) {
            const uint32_t dd = depth + bounce;
            if (bounce > 0) {
                if (dd >= a.max_depth) break;  // uniform
                nmid_w += (uint32_t)__popcll(__ballot(live));
                tmax = K_INF;
            }
            did_seg = false;
            did_shadow = false;
            survive = false;
            if (live) survive = bounce_step<ACCEL>(a, tb, ls, r_L, dd, ka, kb, home, tmax, o, d, thr, L, eta, prev_pdf, did_seg, did_shadow);
            live = survive;
            nseg_w += (uint32_t)__popcll(__ballot(did_seg));
            nshd_w += (uint32_t)__popcll(__ballot(did_shadow));
        }
        // ---- segment-local stream compaction (as in k_bounce)
        const unsigned long long bal = __ballot(survive);
        const uint32_t prefix = ballot_rank(bal);
        if ((tid & 63u) == 0) {
            wave_tot[buf][wid] = (uint32_t)__popcll(bal);
            wave_seg[buf][wid] = nseg_w;
            wave_shd[buf][wid] = nshd_w;
            wave_mid[buf][wid] = nmid_w;
        }
        __syncthreads();
        uint32_t off = 0, total = 0;
        WAVE_SCAN(W, wave_tot[buf], tid, wid, off, total);
        if (survive) {
            const uint32_t v4 = state_voff(base + off + prefix);
            constexpr uint32_t row = STATE_ROW_BYTES;
            STATE_STORE(STATE_BST, o, d, thr, L, eta, prev_pdf, home);
        }
        if (tid == 0) {  // wave 0 stays as long as the segment has a live path
            uint32_t mid = 0;
            for (uint32_t w = 0; w < W; ++w) {
                ns_acc += wave_seg[buf][w];
                nh_acc += wave_shd[buf][w];
                mid += wave_mid[buf][w];
            }
            unsigned long long *row = a.stats + seg;
            const size_t stride = a.stat_stride;
            row[(2 + min(depth, (uint32_t)MAX_DEPTH_STATS - 1)) * stride] += cnt_in;
            if (nb > 1 && depth + 1 < a.max_depth) row[(2 + min(depth + 1, (uint32_t)MAX_DEPTH_STATS - 1)) * stride] += mid;
        }
        left = total;
        depth += nb;
        if (total == 0 || depth >= a.max_depth) break;  // uniform: `total` is the same in every wave
        // the survivors just written are the next bounce's input: stores complete (release at workgroup scope; the waves
        // of a workgroup share the CU's vector L1), and everybody has finished reading the old input
        __threadfence_block();
        __syncthreads();
        const Rsrc t_r = r_in;
        r_in = r_out;
        r_out = t_r;
        cnt_in = total;
        ++trip;
        leave_wave(cnt_in);
    }
    if (tid == 0) {
        a.seg_out[seg] = left;
        unsigned long long *row = a.stats + seg;
        row[0] += ns_acc;
        row[a.stat_stride] += nh_acc;
    }
}

// ---- k_regen: persistent waves with path regeneration (brute-force kernels) -------------------------------------------
// The uniform primitive loop of the brute-force kernels does not care which paths share a wave, so nothing forces the
// wavefront organisation on them: here a lane carries ONE path from the camera to its end in registers, and a lane whose
// path ended takes the next unstarted path of its wave (one ballot + mbcnt per trip: the wave hands out the homes of its
// share in order).  No path state in memory at all, no compaction, no barrier after the table staging, one launch per
// pass; what a path leaves behind is its 16-byte Lhome record, and the film gather reads those in the same fixed order as
// before, so the film does not change by a bit.  The grid is the number of waves the GPU holds at once (host:
// regen_grid); wave w of W takes the 64-home groups w, w + W, w + 2 W, ... of the pass, so every wave samples the whole
// film and the waves finish together (no queue in memory: same-word returning atomics cost 0.3 us each here).
// Statistics: segments and shadow rays are counted per trip (wave-uniform popcounts); the depth rows come from a
// histogram of the paths' final depths (one LDS atomic per finished path), live[d] = paths with more than d bounces.
#ifndef REGEN_WG
#define REGEN_WG 256
#endif
#ifndef REGEN_WAVES_PER_EU
#define REGEN_WAVES_PER_EU 4
#endif
template <int ACCEL>
__global__ __launch_bounds__(REGEN_WG, REGEN_WAVES_PER_EU) void k_regen(const RadArgs a) {
    static_assert(ACCEL == ACCEL_K_BRUTE || ACCEL == ACCEL_K_BRUTE_BIG, "path regeneration: brute-force kernels only");
    constexpr uint32_t W = REGEN_WG / 64;
    __shared__ uint32_t tab_lds[ACCEL == ACCEL_K_BRUTE ? TAB_DW : 1];
    __shared__ uint32_t hist[W][MAX_DEPTH_STATS + 2];  // per wave: paths that ended after d + 1 bounces
    const uint32_t tid = threadIdx.x, wid = tid >> 6, lane = tid & 63u;
    const LdsScene ls = NO_LDS_SCENE;
    const Tables tb = make_tables<ACCEL>(a.sc, ls, tab_lds);
    hist[wid][lane] = 0;  // MAX_DEPTH_STATS + 2 == 64
    if (ACCEL == ACCEL_K_BRUTE)
        fill_tables_lds(a.sc, tab_lds, REGEN_WG);  // ends with the only barrier of the kernel
    else
        __syncthreads();
    const uint32_t gw = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * W + wid)), GW = gridDim.x * W;
    const Rsrc r_L = make_rsrc(a.Lhome, a.cap * 16u);
    uint32_t q = 0;  // wave-uniform: homes of this wave's share handed out so far
    bool live = false;
    V3 o = {0, 0, 0}, d = {0, 0, 1}, thr = {0, 0, 0}, L = {0, 0, 0};
    float eta = 1.0f, prev_pdf = -1.0f, tmax = K_INF;
    uint32_t home = 0, ka = 0, kb = 0, depth = 0;
    uint32_t nseg_w = 0, nshd_w = 0;
#pragma unroll 1
    for (;;) {
        const unsigned long long need = __ballot(!live);
        if (need) {  // uniform: hand the next homes of the share to the idle lanes
            const uint32_t v = q + ballot_rank(need);
            const uint32_t h0 = ((v >> 6) * GW + gw) * 64u + (v & 63u);
            if (!live && h0 < a.n_paths) {
                home = h0;
                camera_start(a, home, &ka, &kb, &o, &d, &tmax, &thr, &L, &eta, &prev_pdf);
                depth = 0;
                live = true;
            }
            q += (uint32_t)__popcll(need);
        }
        if (__ballot(live) == 0) break;  // the share is exhausted and every path of the wave has ended
        bool did_seg = false, did_shadow = false;
        if (live) {
            const bool survive =
                bounce_step<ACCEL>(a, tb, ls, r_L, depth, ka, kb, home, tmax, o, d, thr, L, eta, prev_pdf, did_seg, did_shadow);
            if (!survive) atomicAdd(&hist[wid][min(depth, (uint32_t)MAX_DEPTH_STATS)], 1u);
            live = survive;
            ++depth;
            tmax = K_INF;
        }
        nseg_w += (uint32_t)__popcll(__ballot(did_seg));
        nshd_w += (uint32_t)__popcll(__ballot(did_shadow));
    }
    // statistics row of this wave: live[d] = paths that entered depth d = paths that ended after more than d bounces
    unsigned long long *row = a.stats + gw;
    const size_t stride = a.stat_stride;
    if (lane == 0) {
        row[0] += nseg_w;
        row[stride] += nshd_w;
    }
    if (lane < min(a.max_depth, (uint32_t)MAX_DEPTH_STATS)) {
        uint32_t n = 0;
        for (uint32_t k = lane; k <= MAX_DEPTH_STATS; ++k) n += hist[wid][k];  // own wave's atomics: program order
        row[(2 + lane) * stride] += n;
    }
}

// ---- repack (BVH kernels, depth >= 2): deal the live paths evenly to as few workgroups as fill the GPU ----------
// Per-wave compaction keeps every path inside the 512 slots its wave owns.  When few paths are left (open scenes:
// 22 % after two bounces of the ring scene, 1 % after five) every workgroup still stages the whole scene in LDS for
// a handful of paths and runs with mostly empty waves: 330-1500 ps per path instead of 160.  k_scan_owners turns the
// owners' live counts into exclusive offsets (one workgroup; <= a few 10^4 counts) and picks the new shape: the
// paths go to G = clamp(ceil(total / REGION), min_wg, n_regions) workgroups (min_wg = one per CU: fewer would leave
// CUs idle, more would stage the scene more often), `quota` paths per wave.  k_repack_copy moves path j of owner i
// to its new slot in the spare state buffer (120 B per live path, a fraction of a BVH bounce).  Slot order changes,
// results do not (the film gathers by `home`).
__global__ __launch_bounds__(1024) void k_scan_owners(const uint32_t *cnt, uint32_t n_own, uint32_t wreg, uint32_t owners_per_wg,
                                                     uint32_t min_wg, uint32_t *offs, uint32_t *cnt_new, uint32_t *quota_out) {
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x, per = (n_own + 1023u) / 1024u;
    const uint32_t lo = min(t * per, n_own), hi = min(lo + per, n_own);
    uint32_t s = 0;
    for (uint32_t i = lo; i < hi; ++i) s += cnt[i];
    part[t] = s;
    __syncthreads();
    for (uint32_t w = 1; w < 1024; w <<= 1) {  // Hillis-Steele inclusive scan
        const uint32_t v = t >= w ? part[t - w] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const uint32_t total = part[1023];
    uint32_t run = part[t] - s;  // exclusive prefix of this thread's block of owners
    for (uint32_t i = lo; i < hi; ++i) {
        offs[i] = run;
        run += cnt[i];
    }
    const uint32_t n_wg = n_own / owners_per_wg, region = wreg * owners_per_wg;
    const uint32_t g = min(max((total + region - 1u) / region, min(min_wg, n_wg)), n_wg);
    const uint32_t act = g * owners_per_wg;                       // owners that receive paths
    const uint32_t quota = max((total + act - 1u) / act, 1u);     // <= wreg because g * region >= total
    if (t == 0) *quota_out = quota;
    for (uint32_t i = lo; i < hi; ++i) cnt_new[i] = total > i * quota ? min(total - i * quota, quota) : 0u;
}

// one workgroup per source owner
__global__ __launch_bounds__(256) void k_repack_copy(const float *__restrict__ in, float *__restrict__ out,
                                                     const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ offs,
                                                     const uint32_t *__restrict__ quota_p, uint32_t n_own, uint32_t wreg) {
    const uint32_t own = blockIdx.x;
    if (own >= n_own) return;
    const uint32_t n = cnt[own], dense0 = offs[own], src0 = own * wreg, quota = *quota_p;
    for (uint32_t j = threadIdx.x; j < n; j += 256u) {
        const uint32_t dense = dense0 + j, o2 = dense / quota, p2 = dense - o2 * quota;
        const float *s = in + (state_voff(src0 + j) >> 2);
        float *d = out + (state_voff(o2 * wreg + p2) >> 2);
        float v[N_STATE];
#pragma unroll
        for (int k = 0; k < N_STATE; ++k) v[k] = s[k * 64];
#pragma unroll
        for (int k = 0; k < N_STATE; ++k) d[k * 64] = v[k];
    }
}
