// kernels_radiance.h -- radiance-mode wavefront kernels (gfx950).
//
// Layout in HBM (DESIGN.md "Data layout"): path state is a tiled structure of arrays, N_STATE dwords per slot (the rows ST_* and
// state_voff below).  Slots are grouped in segments of SEG = workgroup size.  One bounce = one launch: workgroup g reads
// the live prefix of region g of the `in` state, advances every path by one bounce (closest hit,
// emission + MIS, next-event estimation with its shadow ray, BSDF sample, Russian roulette) and
// writes the survivors, compacted to the front of region g of the `out` state: brute-force scenes with a wave
// ballot + mbcnt prefix and a scan across the workgroup's waves through LDS (region = one segment), BVH scenes with
// a chunk queue and a slot reservation in LDS (region = REGION_SEGS_BVH segments).  No global atomics are on
// the path-state data path; paths that end write their radiance once to Lhome[home].
#pragma once
#include "device_scene.h"
#include "render_request.h"  // N_STATE, MAX_DEPTH_STATS, MAX_CHAIN, HIT_ROW0: the constants the host arithmetic shares with the kernels
#include "tile_cull.h"

// slots per compaction segment == threads per workgroup (seg_threads(ACCEL) below).  Measured on MI355X, cbox
// 512^2 x 256 spp (current kernel): 128 / 256 / 512 / 1024 -> 10.5 / 9.0 / 8.6 / 9.9 ms; the LDS-staged BVH wants
// the largest workgroup (ring: 39 ms at 1024, 78 ms at 256 when first measured).
#ifndef SEG_BRUTE
#define SEG_BRUTE 512
#endif
#ifndef SEG_BVH
#define SEG_BVH 1024
#endif
#ifndef SEG_WAVES_PER_EU
#define SEG_WAVES_PER_EU 8  // __launch_bounds__ hint for the brute-force kernels: 64 VGPRs, 8 waves per SIMD
#endif
// A workgroup owns a REGION of region_segs * SEG slots and walks its live prefix in chunks.
// Measured on MI355X: walking several chunks amortises the LDS staging of BVH scenes
// (ring: 47 -> 39 ms; best at 4 segments with the chunk queue) and the block prologue of the ultrasound kernel
// (3.9 -> 3.1 ms), but any loop around the bounce body pushes the brute-force radiance kernel over its 64-VGPR
// budget (2 / 4 segments: 13.6 / 12.0 ms against 8.2), so that variant keeps one chunk per workgroup.
#ifndef REGION_SEGS_BVH
#define REGION_SEGS_BVH 4
#endif
#ifndef REGION_SEGS_BRUTE
#define REGION_SEGS_BRUTE 1
#endif
#ifndef REGION_SEGS_US
#define REGION_SEGS_US 8
#endif
__host__ __device__ constexpr uint32_t rad_region_segs(int accel);
// (emitter primary rays, D15: every first-bounce echo has its own arrival time, and the workgroup's echo table catches more of them
// the more paths of a ray it sees before it is flushed -- 8 / 16 / 32 segments: 24.5 - 25.8 / 21.0 - 21.5 / 20.9 - 21.5 ms; with the
// integrator's own rays, whose first bounce is table-driven, 16 segments cost 2 - 4 %: 10.8 - 10.9 -> 11.0 - 11.2 ms)
#ifndef REGION_SEGS_US_EMIT
#define REGION_SEGS_US_EMIT 16
#endif
__host__ __device__ constexpr uint32_t us_region_segs(int, bool emit = false) { return emit ? REGION_SEGS_US_EMIT : REGION_SEGS_US; }

// (ACCEL_K_BRUTE, _BVH_GLOBAL, _BVH_LDS, _BRUTE_BIG: scene_request.h, where a scene's is chosen)
// k_bounce only: ACCEL_K_BRUTE_BIG with the rough / Fresnel conductor code (scenes that hold such a material).  A template
// argument of that kernel, never a pbrt_scene::accel_kernel: inside the kernel it is ACCEL_K_BRUTE_BIG + GLOSSY.
enum { ACCEL_K_BRUTE_GLOSSY = 4 };
// k_bounce only: ACCEL_K_BRUTE on a scene whose two primitive lists are class-ordered (DevScene::prim_ord): the walks read no run
// table (device_scene.h brute_intersect ORDERED).  Like _GLOSSY a template argument only; inside the kernel it is ACCEL_K_BRUTE.
enum { ACCEL_K_BRUTE_ORDERED = 5 };
__host__ __device__ constexpr int accel_base(int accel) {
    return accel == ACCEL_K_BRUTE_GLOSSY ? ACCEL_K_BRUTE_BIG : accel == ACCEL_K_BRUTE_ORDERED ? ACCEL_K_BRUTE : accel;
}
__host__ __device__ constexpr uint32_t rad_region_segs(int accel) {
    return (accel == ACCEL_K_BVH_GLOBAL || accel == ACCEL_K_BVH_LDS) ? REGION_SEGS_BVH : REGION_SEGS_BRUTE;
}
__host__ __device__ constexpr uint32_t seg_threads(int accel) {
    return (accel == ACCEL_K_BVH_GLOBAL || accel == ACCEL_K_BVH_LDS) ? SEG_BVH : SEG_BRUTE;
}
#ifndef BIG_WAVES_PER_EU
#define BIG_WAVES_PER_EU 8
#endif
__host__ __device__ constexpr uint32_t seg_waves_per_eu(int accel) {
    // _BIG (tables in global memory, cone code): round 1 gave these kernels the 128-register budget (4 spilled VGPRs at 64 then).
    // Built without SLP vectorisation the one-bounce variants fit 58 - 64 VGPRs and the two-bounce ones spill 4 - 8 at 64;
    // four 512-thread workgroups per CU instead of three: cone_room 512^2 x 256 10.21 -> 9.82 ms
    return (accel == ACCEL_K_BVH_GLOBAL || accel == ACCEL_K_BVH_LDS) ? SEG_BVH / 256 : (accel == ACCEL_K_BRUTE_BIG ? BIG_WAVES_PER_EU : SEG_WAVES_PER_EU);
}
// BVH kernels compact per WAVE: every wave owns REGION / (SEG / 64) slots of its workgroup's region, walks its own
// live prefix 64 paths at a time and packs its survivors with ballot + mbcnt alone -- no barrier after the scene is
// staged.  Traversal time varies a lot from wave to wave (measured: 2.7 of 4 possible waves per SIMD active with the
// per-chunk workgroup barrier), so the 16 waves of a workgroup must not wait for each other.  (The brute-force
// kernels keep the workgroup scan: there the barrier is cheap and private regions cost registers, DESIGN.md.)
__host__ __device__ constexpr bool rad_wave_private(int accel) {
    return accel == ACCEL_K_BVH_GLOBAL || accel == ACCEL_K_BVH_LDS;
}
// Radiance BVH kernels go one step further: the waves of a workgroup take their 64-path chunks from a queue in LDS
// (one returning ds_add per chunk) and reserve the slots of their survivors with another, so the region is one
// compaction domain again and the waves of a workgroup finish together -- with fixed 512-slot shares a wave with
// expensive rays kept its workgroup (and the 114 KB LDS image) alive while the other 15 had long left
// (measured: 2.3 of 4 possible waves per SIMD).
__host__ __device__ constexpr bool rad_dynamic(int accel) {
    return rad_wave_private(accel);
}
// live-path counters per region of the radiance kernels (one per region: the waves of a BVH workgroup share theirs)
__host__ __device__ constexpr uint32_t rad_owners_per_region(int) {
    return 1;
}
// statistics rows per region (per workgroup, or per wave)
__host__ __device__ constexpr uint32_t rad_rows_per_region(int accel) {
    return rad_wave_private(accel) ? seg_threads(accel) / 64 : 1;
}
#define TAB_DW (TAB_MAX * 16 + TAB_MAX * 8 + TAB_MAX * 12 + TAB_MAX + TAB_MAX)

struct RadArgs {
    DevScene sc;
    pbrt_camera cam;
    const float *in;   // [cap / 64][N_STATE][64] tiled SoA (state_voff)
    float *out;        // same layout
    float *Lhome;      // [cap] float4 records (r, g, b, 0) indexed by home
    const uint32_t *seg_in;
    uint32_t *seg_out;
    unsigned long long *stats;  // [k][stat_stride] per-segment rows: k = 0 segments, 1 shadow rays, 2 + d live paths entering depth d
    uint32_t stat_stride;
    uint32_t cap;        // slots of Lhome
    uint32_t state_cap;  // slots of the `in` / `out` state (<= cap: a pass whose bounces all run in one launch needs none)
    uint32_t n_paths;  // paths generated by the first bounce of this pass
    uint32_t depth, max_depth, rr_depth, seed;
    uint32_t nb;  // bounces this launch walks (the multi-bounce variants k_bounce<.., 2>; 2 .. MAX_CHAIN)
    uint32_t repack_mask;  // unused; kept so that the kernel-argument layout stays unchanged
    uint32_t merge_at;  // k_chain_pair: the bounce from which a wave walks the survivors of its two tiles together (1 .. max_depth - 1)
    // key mode 0 (render): home -> (region pixel, local sample)
    uint32_t key_mode;
    FilmKey key;
    // key mode 1 (Integrator.sample on caller rays): key = (index_offset + home, sample_index)
    uint32_t index_offset, sample_index;
    uint32_t lds_bytes;  // ACCEL_K_BVH_LDS: bytes of nodes + prims + ids staged per workgroup
    // key mode 0, ACCEL_K_BRUTE, npix_r % 64 == 0: the keep words of the camera tiles, [npix_r / 64] (k_tile_keep); nullptr: none
    const uint32_t *tile_keep;
};
// kernel-argument layout is part of a kernel's figures: the key stands where its ten members stood, nothing behind it moved
static_assert(offsetof(RadArgs, repack_mask) == 292 && offsetof(RadArgs, key_mode) == 300 && offsetof(RadArgs, key) == 304 &&
                  offsetof(RadArgs, index_offset) == 368 && offsetof(RadArgs, sample_index) == 372 && offsetof(RadArgs, tile_keep) == 384 &&
                  sizeof(RadArgs) == 392,
              "RadArgs keeps its bytes");

// Path state is tiled SoA: 64 consecutive slots (one wave) form a tile of N_STATE rows x 64 lanes = 3840 contiguous
// bytes, row k of a slot at byte  tile(slot) + k * 256 + lane * 4.  Accessed through buffer descriptors:
// `buffer_load_dword v, v_off, s[rsrc], 0 offen offset:k*256` folds the row into the 12-bit immediate, so the
// 15 + 15 state accesses of a bounce need no 64-bit VALU address arithmetic (the kernel is VALU-bound) and no
// SGPR per row (the kernel sits at the 80-SGPR occupancy limit).  A wave reads one contiguous 3840-byte tile.
// Requires N_STATE * cap * 4 < 4 GiB (checked by the host) and cap % 64 == 0.
// The rows of a path's record (the ONE place that says what they are; the wave-private LDS strip of k_chain_pair has the same rows):
//   ST_O, ST_D    3 rows each: ray origin, ray direction
//   ST_THR, ST_L  3 rows each: throughput rgb, radiance rgb
//   ST_ETA        eta.  Key mode 1 (Integrator.sample on caller rays): the record k_init_rays writes carries the ray's tmax here
//                 instead, and the bounce at depth 0 that reads it takes the row as tmax and starts from eta = 1
//   ST_PDF        pdf of the previous BSDF sample (< 0: the previous event was a delta lobe / the camera)
//   ST_HOME       home slot (uint32): index of the path's radiance record and of its pixel / sample
enum { ST_O = 0, ST_D = 3, ST_THR = 6, ST_L = 9, ST_ETA = 12, ST_PDF = 13, ST_HOME = 14 };
static_assert(ST_HOME == N_STATE - 1, "the rows of a path record");
#define STATE_TILE_BYTES (64u * N_STATE * 4u)
#define STATE_ROW_BYTES 256u
DEV uint32_t state_voff(uint32_t slot) { return (slot >> 6) * STATE_TILE_BYTES + (slot & 63u) * 4u; }
typedef __amdgpu_buffer_rsrc_t Rsrc;
DEV Rsrc make_rsrc(const void *p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, bytes, 0x00020000);
}
DEV float bld(Rsrc r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
DEV void bst(Rsrc r, uint32_t voff, uint32_t soff, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, voff, soff, 0);
}
// A record read or written row by row: get(row) is the row as a float, put(row, v) takes it.  Macros on macros, not functions or
// callables (as DAS_DELAYED, kernels_beamform.h): the 15 accesses then are the site's own statements on its own variables.  Functions
// with reference parameters and lambdas as get / put each moved the scalar spills of k_bounce chain instances
// (profiles/shared_path_start.md).  STATE_BLD / STATE_BST: the rows of a state tile through the site's descriptors r_in / r_out, at
// its byte offset v4 = state_voff(slot), with its `constexpr uint32_t row = STATE_ROW_BYTES`.
#define STATE_BLD(k) bld(r_in, v4 + (k) * row, 0)
#define STATE_BST(k, v) bst(r_out, v4 + (k) * row, 0, v)
#define STATE_LOAD(get, o, d, thr, L, eta, prev_pdf, home)             \
    {                                                                  \
        o = {get(ST_O + 0), get(ST_O + 1), get(ST_O + 2)};             \
        d = {get(ST_D + 0), get(ST_D + 1), get(ST_D + 2)};             \
        thr = {get(ST_THR + 0), get(ST_THR + 1), get(ST_THR + 2)};     \
        L = {get(ST_L + 0), get(ST_L + 1), get(ST_L + 2)};             \
        eta = get(ST_ETA);                                             \
        prev_pdf = get(ST_PDF);                                        \
        home = __float_as_uint(get(ST_HOME));                          \
    }
#define STATE_STORE(put, o, d, thr, L, eta, prev_pdf, home)            \
    {                                                                  \
        put(ST_O + 0, (o).x);                                          \
        put(ST_O + 1, (o).y);                                          \
        put(ST_O + 2, (o).z);                                          \
        put(ST_D + 0, (d).x);                                          \
        put(ST_D + 1, (d).y);                                          \
        put(ST_D + 2, (d).z);                                          \
        put(ST_THR + 0, (thr).x);                                      \
        put(ST_THR + 1, (thr).y);                                      \
        put(ST_THR + 2, (thr).z);                                      \
        put(ST_L + 0, (L).x);                                          \
        put(ST_L + 1, (L).y);                                          \
        put(ST_L + 2, (L).z);                                          \
        put(ST_ETA, eta);                                              \
        put(ST_PDF, prev_pdf);                                         \
        put(ST_HOME, __uint_as_float(home));                           \
    }

// Workgroup b runs on XCD b % 8 (round-robin dispatch), and consecutive regions are consecutive pixels of a row: on a film
// that is 8 segments wide (4096 px) XCD k would render column stripe k of EVERY row -- the XCDs with the spheres in their stripe
// finish last (cbox 4096^2: the later bounces 18-40 % slower than on the 512^2 film with the same paths).  Rotating the regions
// inside every aligned group of 8 by the sum of the base-8 digits of the group index deals every stripe to every XCD in turn.
// A permutation of [0, n): the last, partial group is left alone.
DEV uint32_t xcd_swizzle(uint32_t b, uint32_t n) {
    if ((b | 7u) >= n) return b;
    uint32_t g = b >> 3, rot = 0;
    while (g) {
        rot += g;
        g >>= 3;
    }
    return (b & ~7u) | ((b + rot) & 7u);
}

// The RNG key (ka, kb) and the pixel of the path whose home slot is `home`.  Key mode 0 inverts region_index (region_pixel, film_key.h),
// in every kernel: 8 x 8 pixel tiles per wave are coherent rays for the BVH kernels; for the brute-force kernels, whose
// primitive loop does not care, they keep the long paths of a chain launch (the pixels of the glass and the mirror sphere) together
// in the same waves instead of one or two lanes in every wave of a row: Cornell box, one launch per pass, 6.41 -> 6.25 ms.
// Args: RadArgs, WfArgs, or PathArgs (k_path: key mode 0 as a constant): key_mode, the film key, index_offset, sample_index
template <class Args>
DEV void path_key(const Args &a, uint32_t home, uint32_t *ka, uint32_t *kb, uint32_t *px, uint32_t *py) {
    if (a.key_mode == 0) {
        const FilmKey &k = a.key;
        uint32_t sl = udiv_fast(home, k.div_npix), pr = home - sl * k.npix_r, rx, ry;
        region_pixel(k, pr, &rx, &ry);
        *px = k.rx0 + rx;
        *py = k.ry0 + ry;
        *ka = *py * k.film_w + *px;
        *kb = k.s_first + sl;
    } else {
        *ka = a.index_offset + home;
        *kb = a.sample_index;
        *px = *py = 0;
    }
}
// The camera start of the path at `home`: its key, and the ray through its jittered film position (draw 0 of the key).
template <class Args>
DEV void camera_start(const Args &a, uint32_t home, uint32_t *ka, uint32_t *kb, V3 *o, V3 *d, float *tmax) {
    uint32_t px, py;
    path_key(a, home, ka, kb, &px, &py);
    F4 uj = rng4(*ka, *kb, 0, a.seed);
    float fx = (float)px + uj.x, fy = (float)py + uj.y;
    camera_ray(a.cam, film_coord(fx, a.key.film_w), film_coord(fy, a.key.film_h), o, d, tmax);
}
// ... and the state a path starts with, for the kernels whose lanes start more than one path
template <class Args>
DEV void camera_start(const Args &a, uint32_t home, uint32_t *ka, uint32_t *kb, V3 *o, V3 *d, float *tmax, V3 *thr, V3 *L,
                  float *eta, float *prev_pdf) {
    camera_start(a, home, ka, kb, o, d, tmax);
    *thr = {1, 1, 1};
    *L = {0, 0, 0};
    *eta = 1.0f;
    *prev_pdf = -1.0f;
}
// The keep word of a wave's camera tile (RadArgs::tile_keep != nullptr; base: the home of the workgroup's thread 0).  The wave's
// camera rays are the 8 x 8 tile of one sample (or, on a region whose width is no multiple of 8, a few tiles): the closest-hit walk
// of bounce 0 leaves out what the keep word of its 64 region indices rules out (one scalar load).
template <class Args>
DEV uint32_t camera_keep_word(const Args &a, uint32_t base, uint32_t tid) {
    const uint32_t home0 = base + ((uint32_t)__builtin_amdgcn_readfirstlane((int)tid) & ~63u);
    const uint32_t blk = (home0 - udiv_fast(home0, a.key.div_npix) * a.key.npix_r) >> 6;
    return load_uniform<uint32_t>(a.tile_keep + min(blk, (a.key.npix_r >> 6) - 1u));
}
// One 16-byte radiance record per finished path: three 4-byte row stores at a scattered `home` cost three 32-byte HBM sectors
// (measured: k_bounce WRITE_SIZE 1.23 x algorithmic), one dwordx4 store costs one.
DEV void store_record(Rsrc r_L, uint32_t home, V3 L) {
    typedef uint32_t __attribute__((ext_vector_type(4))) u32x4;
    const u32x4 rec = {__float_as_uint(L.x), __float_as_uint(L.y), __float_as_uint(L.z), 0u};
    __builtin_amdgcn_raw_buffer_store_b128(rec, r_L, home * 16u, 0, 0);
}
// Exclusive scan over the W waves' survivor counts `tot` (LDS, published before a barrier) on the scalar unit: one LDS read per
// lane, then v_readlane + s_add per wave (the per-lane form cost 40 VALU per wave-bounce).  Adds the counts of the waves below wave
// `wid` to `off` and all of them to `total` (names of the site's variables).  A macro like STATE_LOAD: as a function -- `tot` by
// pointer or its element by value, the sums by pointer or by reference -- it moved a VGPR or a scalar spill in k_bounce or k_walk
// (profiles/shared_path_start.md).
#define WAVE_SCAN(W, tot, tid, wid, off, total)                                                \
    {                                                                                          \
        const uint32_t t_lane = (tot)[(tid) & ((W) - 1)];                                      \
        const uint32_t wid_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)(wid));           \
        _Pragma("unroll") for (uint32_t w = 0; w < (W); ++w) {                                 \
            const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)t_lane, (int)w);       \
            off += (w < wid_s) ? t : 0u;                                                       \
            total += t;                                                                        \
        }                                                                                      \
    }
// A wave whose first slot (wave_first, scalar) lies at or beyond the cnt live ones ends here, once its LDS writes have landed:
// s_barrier does not wait for terminated waves.  s_endpgm behind the compiler's back keeps the kernel single-exit for the
// structurizer.
DEV void leave_if_idle(uint32_t wave_first, uint32_t cnt) {
    asm volatile("s_cmp_lt_u32 %0, %1\n\t"
                 "s_cbranch_scc1 .Llive_%=\n\t"
                 "s_waitcnt lgkmcnt(0)\n\t"
                 "s_endpgm\n"
                 ".Llive_%=:" ::"s"(wave_first), "s"(cnt) : "scc", "memory");
}

// LDS image of the BVH scene (device_scene.h TreeLds: node planes | leaf records), and the workgroup's traversal stacks (BvhStack)
struct LdsScene {
    TreeLds tree;
    BvhStack stk;
};
#define NO_TREE_LDS TreeLds{nullptr, 0u, 0u}
#ifndef BVH_STK_ROWS
#define BVH_STK_ROWS 4  // LDS rows of the traversal stacks of the fused kernels; deeper entries go to scratch memory
#endif
#define BVH_STK_DW(threads) (BVH_STK_ROWS * (threads))
__host__ __device__ constexpr uint32_t ilog2_c(uint32_t v) { return v <= 1u ? 0u : 1u + ilog2_c(v >> 1); }
// threads: the workgroup size, a power of two
#define MAKE_BVH_STACK(lds, threads) BvhStack{(LDS_AS uint32_t *)(lds) + threadIdx.x, ilog2_c(threads) + 0u, BVH_STK_ROWS}
// static LDS of a kernel that may walk a BVH: its traversal stacks (one dword for the brute-force variants)
#define BVH_STACK_LDS(ACCEL, THREADS)                                                                              \
    static_assert(((THREADS) & ((THREADS)-1)) == 0, "BVH stack rows are addressed by a shift");                    \
    __shared__ uint32_t bvh_stk_lds[((ACCEL) == ACCEL_K_BVH_GLOBAL || (ACCEL) == ACCEL_K_BVH_LDS) ? BVH_STK_DW(THREADS) : 1]
#define NO_LDS_SCENE {NO_TREE_LDS, BvhStack{nullptr, 0u, 0u}}

// SEGMENT: the ray is a segment between two points of the scene (next-event shadow ray): brute-force
// scenes then only walk the primitives that can occlude such a segment (DevScene::occ_prims).
// ORDERED: brute-force scenes whose lists are class-ordered (DevScene::prim_ord) walk them without the run tables.
template <int ACCEL, bool ANY, bool SEGMENT = false, bool ORDERED = false>
DEV bool scene_intersect(const DevScene &sc, const LdsScene &ls, V3 o, V3 d, float tmax, Hit *h, uint32_t keep = 0xffffffffu) {
    static_assert(!ORDERED || ACCEL == ACCEL_K_BRUTE || ACCEL == ACCEL_K_BRUTE_BIG, "ordered walk: brute-force kernels only");
    if (ACCEL == ACCEL_K_BRUTE || ACCEL == ACCEL_K_BRUTE_BIG)
        return brute_intersect<ANY, SEGMENT, ACCEL != ACCEL_K_BRUTE, ORDERED>(sc, o, d, tmax, h, keep);
    if (ACCEL == ACCEL_K_BVH_GLOBAL) return bvh_intersect<ANY>(TreeGlobal{sc.nodes, sc.lprims}, sc.prims, ls.stk, o, d, tmax, h);
    return bvh_intersect<ANY>(ls.tree, sc.prims, ls.stk, o, d, tmax, h);
}

// ACCEL_K_BRUTE: copy the (<= 32-entry) shading tables into LDS; layout [prims | mats | emitters | light_prims | light_cdf]
// fill: issued AFTER the workgroup's path-state loads so that both round trips overlap; ends with the barrier
// n_threads: the threads of the workgroup that take part (a multiple of 64; waves that left early do not)
DEV void fill_tables_lds(const DevScene &sc, uint32_t *lds, uint32_t n_threads) {
    uint32_t *p_prims = lds, *p_mats = lds + TAB_MAX * 16, *p_emit = p_mats + TAB_MAX * 8, *p_lp = p_emit + TAB_MAX * 12;
    float *p_lc = reinterpret_cast<float *>(p_lp + TAB_MAX);
    for (uint32_t t = threadIdx.x; t < TAB_MAX * 16; t += n_threads) {
        if (t < sc.n_prims * 16) p_prims[t] = reinterpret_cast<const uint32_t *>(sc.prims)[t];
        if (t < sc.n_mats * 8) p_mats[t] = reinterpret_cast<const uint32_t *>(sc.mats)[t];
        if (t < sc.n_emitters * 12) p_emit[t] = reinterpret_cast<const uint32_t *>(sc.emitters)[t];
        if (t < sc.n_light_prims) {
            p_lp[t] = sc.light_prims[t];
            p_lc[t] = sc.light_cdf[t];
        }
    }
    __syncthreads();
}
DEV Tables stage_tables_lds(const DevScene &sc, uint32_t *lds) {
    uint32_t *p_prims = lds, *p_mats = lds + TAB_MAX * 16, *p_emit = p_mats + TAB_MAX * 8, *p_lp = p_emit + TAB_MAX * 12;
    float *p_lc = reinterpret_cast<float *>(p_lp + TAB_MAX);
    Tables tb;
    tb.prims_by_slot = reinterpret_cast<const pbrt_prim *>(p_prims);
    tb.prims_by_id = tb.prims_by_slot;
    tb.mats = reinterpret_cast<const pbrt_material *>(p_mats);
    tb.emitters = reinterpret_cast<const pbrt_emitter *>(p_emit);
    tb.light_prims = p_lp;
    tb.light_cdf = p_lc;
    tb.n_emitters = sc.n_emitters;
    return tb;
}

template <int ACCEL>
DEV Tables make_tables(const DevScene &sc, const LdsScene &ls, uint32_t *tab_lds) {
    if (ACCEL == ACCEL_K_BRUTE) return stage_tables_lds(sc, tab_lds);
    return global_tables(sc);  // BVH: Hit::slot is the caller's index, the hit primitive's full record comes from global memory
}

// Stage the tree into LDS (cooperative): the 64-byte node records of the global image become the planes of TreeLds (quad k of
// node n -> plane k, 16 bytes per lane per step; the fourth quad keeps its first 8 bytes), the 40-byte leaf records follow as
// they are.  Ends with a barrier.
DEV TreeLds stage_tree_lds(const DevScene &sc, uint32_t *lds) {
    const uint32_t n = sc.n_nodes, plane = n * 16u, leaf_off = n * LDS_IMAGE_NODE_BYTES, prim_dw = sc.n_prims * 10u;
    LDS_AS char *img = reinterpret_cast<LDS_AS char *>((LDS_AS uint32_t *)lds);
    const u32x4 *src_n = reinterpret_cast<const u32x4 *>(sc.nodes);
    for (uint32_t i = threadIdx.x; i < n * 4u; i += blockDim.x) {
        const u32x4 q = src_n[i];
        const uint32_t node = i >> 2, k = i & 3u;
        if (k < 3u) {
            *reinterpret_cast<LDS_AS u32x4 *>(img + k * plane + node * 16u) = q;
        } else {
            const u32x2 h = {q.x, q.y};
            *reinterpret_cast<LDS_AS u32x2 *>(img + 3u * plane + node * 8u) = h;
        }
    }
    const u32x2 *src_p = reinterpret_cast<const u32x2 *>(sc.lprims);
    LDS_AS u32x2 *dst_p = reinterpret_cast<LDS_AS u32x2 *>(img + leaf_off);
    for (uint32_t i = threadIdx.x; i < prim_dw / 2u; i += blockDim.x) dst_p[i] = src_p[i];
    __syncthreads();
    return TreeLds{reinterpret_cast<const LDS_AS uint32_t *>(img), plane, leaf_off};
}

// The arithmetic of one bounce from the surface interaction on -- emission + MIS, emitter sampling (next-event estimation) up to its
// shadow segment, BSDF sample, Russian roulette: the ONE definition behind the fused kernels (bounce_step) and the streams
// (kernels_wavefront.h k_shade), whose films agree bit for bit because they run these statements in this order.  What becomes of
// the shadow segment is the caller's: segment(so, sdir, tmax) either traces it at once and says whether it got through, or stores it
// and says yes; contribute(A, B) then adds fma(A, B, L) or stores the two factors for the kernel that learns the visibility.
// Args: RadArgs or WfArgs (n_emitters, max_depth, rr_depth, seed).  Returns whether the path goes on.
// GLOSSY: the scene holds a ROUGHCONDUCTOR / CONDUCTOR_FRESNEL material (device_scene.h bsdf_sample); else their code is compiled out
template <bool GLOSSY, class Args, class Segment, class Contribute>
DEV bool shade_step(const Args &a, const Tables &tb, uint32_t depth, uint32_t ka, uint32_t kb, float t_hit, const pbrt_prim &P,
                    const SI &si, V3 &o, V3 &d, V3 &thr, V3 &L, float &eta, float &prev_pdf, Segment &&segment,
                    Contribute &&contribute) {
    bool survive = false;
    const uint32_t nE = a.sc.n_emitters;
    const int32_t emitter = P.emitter;
    const uint32_t mat_id = P.material;
    // ---- direct emission (one-sided area emitters), MIS against emitter sampling
    if (emitter >= 0) {
        const pbrt_emitter &E = tb.emitters[emitter];
        float cosl = -dot(si.ns, d);  // Frame::cos_theta(si.wi): the shading frame (== n on emitters)
        if (cosl > 0.0f) {
            float w = 1.0f;
            if (prev_pdf >= 0.0f) {
                float pdf_em = (t_hit * t_hit) / (cosl * E.area * (float)nE);
                w = mis_weight(prev_pdf, pdf_em);
            }
            L = {fma_(thr.x * E.radiance[0], w, L.x), fma_(thr.y * E.radiance[1], w, L.y), fma_(thr.z * E.radiance[2], w, L.z)};
        }
    }
    if (depth + 1 < a.max_depth) {
        const pbrt_material M = tb.mats[mat_id];
        Frame fr = make_frame(si.ns);
        V3 wi = to_local(fr, -d);
        // ---- emitter sampling (next-event estimation) + shadow segment
#ifdef PBRT_ABLATE_NEE  // diagnostic builds only (tools/ablate.sh): never defined in the shipped library
        if (false) {
#else
        if ((M.type == PBRT_MAT_DIFFUSE || (GLOSSY && M.type == PBRT_MAT_ROUGHCONDUCTOR)) && nE > 0) {
#endif
            F4 u = rng4(ka, kb, 1 + 2 * depth, a.seed);
            ESample es = sample_emitter(tb, si.p, u);
            if (es.valid) {
                V3 wo = to_local(fr, es.d);
                V3 f;
                float bpdf;
                bsdf_eval_pdf<GLOSSY>(M, wi, wo, &f, &bpdf);
                if (bpdf > 0.0f) {
                    V3 so = offset_origin(si.p, si.n, es.d);
                    V3 sv = es.q - so;
                    float sd = sqrtf(dot(sv, sv));
                    V3 sdir = sv * rcp_rn(sd);  // the reciprocal of a sqrtf result
                    if (segment(so, sdir, sd * (1.0f - K_SHADOW_EPS))) {
                        float mis = es.delta ? 1.0f : mis_weight(es.pdf, bpdf);
                        contribute(v3(thr.x * f.x, thr.y * f.y, thr.z * f.z), v3(es.weight.x * mis, es.weight.y * mis, es.weight.z * mis));
                    }
                }
            }
        }
        // ---- BSDF sampling, continuation ray, Russian roulette
        F4 ub = rng4(ka, kb, 2 + 2 * depth, a.seed);
        BSample bs = bsdf_sample<GLOSSY>(M, PBRT_USQ_REFERENCE, wi, si.n, si.ns, fr, ub.x, ub.y, ub.z);
        if (bs.valid) {
            thr = thr * bs.weight;
            eta *= bs.eta;
            V3 nd = to_world(fr, bs.wo);
            if (M.type == PBRT_MAT_ULTRA) nd = normalize(nd);
            o = offset_origin(si.p, si.n, nd);
            d = nd;
            prev_pdf = bs.delta ? -1.0f : bs.pdf;
            float tm = max3(thr);
            survive = true;
            if (depth + 1 >= a.rr_depth) {
                float q = fminf(tm * eta * eta, 0.95f);
                float rq = 1.0f / q;
                thr = thr * rq;
                if (!(ub.w < q)) survive = false;
            }
            if (tm == 0.0f) survive = false;
        }
    }
    return survive;
}

// One bounce of one path (the body shared by k_bounce and k_walk): closest hit, the surface interaction, shade_step with its
// shadow segment traced at once.  Returns whether the path goes on; a path that ends writes its radiance to Lhome[home].
// HAVE_HIT: the closest hit was found earlier (k_bounce_pool) and comes in through h_in; the step starts at the shading.
// keep: the primitives the closest-hit walk may leave out (device_scene.h brute_intersect); the shadow walk sees them all.
// GLOSSY: as shade_step.  Only k_bounce of the brute-force scenes has instances without it: every other kernel that comes through
// here (the diagnostic build's launch structures, on the _BIG tables) always carries the arms.
// ORDERED: as scene_intersect (the ACCEL_K_BRUTE_ORDERED instances of k_bounce).
// STORE: a path that ends writes its record here; without it the caller does, from the L the lane keeps (k_path: r_L is not read).
// Args: RadArgs, or PathArgs (k_path).
template <int ACCEL, bool HAVE_HIT = false, bool GLOSSY = ACCEL != ACCEL_K_BRUTE, bool ORDERED = false, bool STORE = true, class Args>
DEV bool bounce_step(const Args &a, const Tables &tb, const LdsScene &ls, Rsrc r_L, uint32_t depth, uint32_t ka, uint32_t kb,
                     uint32_t home, float tmax, V3 &o, V3 &d, V3 &thr, V3 &L, float &eta, float &prev_pdf, bool &did_seg,
                     bool &did_shadow, const Hit *h_in = nullptr, uint32_t keep = 0xffffffffu) {
    bool survive = false;
    Hit h;
    if (HAVE_HIT) h = *h_in;
    if (HAVE_HIT || scene_intersect<ACCEL, false, false, ORDERED>(a.sc, ls, o, d, tmax, &h, keep)) {
        did_seg = true;
        const pbrt_prim &P = tb.prims_by_slot[h.slot];
        const SI si = make_si<ACCEL != ACCEL_K_BRUTE>(P, o, d, h.t, h.u, h.v, a.sc.vnormals, h.slot);
        survive = shade_step<GLOSSY>(
            a, tb, depth, ka, kb, h.t, P, si, o, d, thr, L, eta, prev_pdf,
            [&](V3 so, V3 sdir, float smax) {
                did_shadow = true;
#ifdef PBRT_ABLATE_SHADOW  // diagnostic builds only (tools/ablate.sh)
                return smax > 0.0f;
#else
                Hit hs;
                return !scene_intersect<ACCEL, true, true, ORDERED>(a.sc, ls, so, sdir, smax, &hs);
#endif
            },
            [&](V3 A, V3 B) { L = {fma_(A.x, B.x, L.x), fma_(A.y, B.y, L.y), fma_(A.z, B.z, L.z)}; });
    }
    if (STORE && !survive) store_record(r_L, home, L);
    return survive;
}

// NB = 2: the multi-bounce variant (brute-force kernels only): the launch walks a.nb (2 .. MAX_CHAIN) bounces.  A path that
// survives a bounce of the launch goes straight on in registers -- no state write, no compaction, no state read in between -- and the
// lanes whose paths ended idle through the second bounce (87 % / 83 % of the lanes stay busy at depths 0 / 2 of the
// Cornell box, 20 % at depth 4 -- where the second bounce is the last one and only looks for emitters).  Same arithmetic
// per bounce, same RNG keys: the film does not change.  Which depths start a two-bounce launch is the host's fuse plan
// (pbrt_api.hip PBRT_DEFAULT_FUSE_PLAN: every pair).
// ACCEL_T: ACCEL_K_*, or ACCEL_K_BRUTE_GLOSSY for the instances of brute-force scenes with a ROUGHCONDUCTOR / CONDUCTOR_FRESNEL
// material; the fused BVH bounce of the diagnostic build always carries those arms.  ACCEL_K_BRUTE_ORDERED: the instances of
// ACCEL_K_BRUTE scenes with class-ordered lists.
template <bool FIRST, int ACCEL_T, int NB = 1>
// two-bounce variants of ACCEL_K_BRUTE at the 64-register budget: 8 waves per SIMD with ONE spilled VGPR (a 4-byte scratch store
// and load per bounce).  Without the budget the kernel takes 67 VGPRs = 7 waves, i.e. three 512-thread workgroups per CU instead of
// four: 6.99 - 7.03 -> 6.82 - 6.85 ms on the Cornell box.  (Before -fno-slp-vectorize the same budget spilled 5 VGPRs and wrote
// 700 MB of scratch per launch for +0.8 %: not taken then.)
#ifndef FUSED_WAVES_PER_EU
#define FUSED_WAVES_PER_EU 8
#endif
// ACCEL_K_BRUTE_GLOSSY: at the 64-register budget of their twins the GGX + Fresnel arms spill 18 - 38 VGPRs to scratch;
// those instances take the 128-register budget instead (4 waves per SIMD, two 512-thread workgroups per CU) and spill none.
// Measured on the rough tube of examples/ (512^2 x 256 spp): 4.06 - 4.13 ms at 8 against 3.80 - 3.84 ms at 4 (alpha 0.4), level at
// alpha 0.1 (profiles/rough_conductor.md).  One scene with one primitive: a scene with many may weigh occupancy higher.
#ifndef GLOSSY_WAVES_PER_EU
#define GLOSSY_WAVES_PER_EU 4
#endif
__global__ __launch_bounds__(seg_threads(accel_base(ACCEL_T)), ACCEL_T == ACCEL_K_BRUTE_GLOSSY ? GLOSSY_WAVES_PER_EU : NB > 1 ? (accel_base(ACCEL_T) == ACCEL_K_BRUTE ? FUSED_WAVES_PER_EU : BIG_WAVES_PER_EU) : seg_waves_per_eu(accel_base(ACCEL_T))) void k_bounce(const RadArgs a) {
    constexpr int ACCEL = accel_base(ACCEL_T);
    static_assert(NB == 1 || ACCEL == ACCEL_K_BRUTE || ACCEL == ACCEL_K_BRUTE_BIG, "fused bounces: brute-force kernels only");
    constexpr bool GL = ACCEL_T == ACCEL_K_BRUTE_GLOSSY || ACCEL == ACCEL_K_BVH_GLOBAL || ACCEL == ACCEL_K_BVH_LDS;
    constexpr bool ORD = ACCEL_T == ACCEL_K_BRUTE_ORDERED;
    // the per-bounce survivor counts of a chain are packed 10 bits each per WORKGROUP and summed by thread 0: one segment per region,
    // workgroup-level compaction (a -DREGION_SEGS_BRUTE build would silently lose them)
    static_assert(NB == 1 || (rad_region_segs(ACCEL) == 1 && !rad_wave_private(ACCEL) && seg_threads(ACCEL) <= 1023),
                  "chain launches: REGION == SEG, workgroup scan");
    constexpr uint32_t SEG = seg_threads(ACCEL);
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn_lds[];
    __shared__ uint32_t wave_tot[2][SEG / 64];  // double-buffered across the chunk loop: one barrier per chunk
    __shared__ uint32_t wave_seg[2][SEG / 64];
    __shared__ uint32_t wave_shd[2][SEG / 64];
    // multi-bounce launches: paths that went on to the launch's 2nd .. 6th bounce, 10 bits each (a workgroup has <= 512):
    // bounces 2 - 4 in wave_mid, 5 - 6 in wave_mid_hi
    __shared__ uint32_t wave_mid[2][NB > 1 ? SEG / 64 : 1], wave_mid_hi[2][NB > 1 ? SEG / 64 : 1];

    const uint32_t seg = xcd_swizzle(blockIdx.x, gridDim.x);  // region index
    const uint32_t tid = threadIdx.x;
    constexpr uint32_t REGION = rad_region_segs(ACCEL) * SEG;
    constexpr bool DYN = rad_dynamic(ACCEL);  // chunk queue + slot reservation in LDS (BVH kernels): the waves walk 64-path chunks on their own
    constexpr uint32_t W = SEG / 64;          // waves per workgroup
    constexpr uint32_t CH = DYN ? 64u : SEG;  // paths per chunk of the walk
    const uint32_t lane_c = DYN ? (tid & 63u) : tid;              // position inside the chunk
    const uint32_t row_id = DYN ? seg * W + (tid >> 6) : seg;     // statistics row
    const uint32_t base = seg * REGION;
    __shared__ uint32_t q_in, q_out, q_done;                  // DYN: next chunk, next free output slot, finished waves
    if (DYN && tid == 0) {
        q_in = 0;
        q_out = 0;
        q_done = 0;
    }
    uint32_t cnt_in;
    if (FIRST) {
        cnt_in = a.n_paths > base ? min(a.n_paths - base, REGION) : 0u;
    } else {
        cnt_in = a.seg_in[seg];
    }
    if (cnt_in == 0) {  // uniform across the workgroup
        if (tid == 0) a.seg_out[seg] = 0;
        return;
    }
    if (DYN) cnt_in = (uint32_t)__builtin_amdgcn_readfirstlane((int)cnt_in);
    // Waves without a live path leave at once instead of idling until the compaction barrier: their wave slots
    // are free for the next workgroup's waves (late bounces run at 10-50 % fill).  They publish a zero survivor
    // count first; s_barrier does not wait for terminated waves.
#ifndef PBRT_ABLATE_EARLY_EXIT
    constexpr bool early_exit = ACCEL == ACCEL_K_BRUTE && !FIRST && rad_region_segs(ACCEL) == 1 && !DYN;
#else
    constexpr bool early_exit = false;
#endif
    if (early_exit) {
        if ((tid & 63u) == 0) {  // every wave; the live ones overwrite their entries before the compaction barrier
            wave_tot[0][tid >> 6] = 0;
            wave_seg[0][tid >> 6] = 0;
            wave_shd[0][tid >> 6] = 0;
            if (NB > 1) {
                wave_mid[0][tid >> 6] = 0;
                wave_mid_hi[0][tid >> 6] = 0;
            }
        }
        leave_if_idle((uint32_t)__builtin_amdgcn_readfirstlane((int)tid) & ~63u, cnt_in);
    }
    const uint32_t live_threads = early_exit ? (min(cnt_in, SEG) + 63u) & ~63u : SEG;  // waves still present
    BVH_STACK_LDS(ACCEL, SEG);
    LdsScene ls = {NO_TREE_LDS, MAKE_BVH_STACK(bvh_stk_lds, SEG)};
    if (ACCEL == ACCEL_K_BVH_LDS) ls.tree = stage_tree_lds(a.sc, dyn_lds);  // ends with a barrier
    if (DYN && ACCEL != ACCEL_K_BVH_LDS) __syncthreads();               // publishes the queue words
    __shared__ uint32_t tab_lds[ACCEL == ACCEL_K_BRUTE ? TAB_DW : 1];
    const Tables tb = make_tables<ACCEL>(a.sc, ls, tab_lds);
    if (ACCEL == ACCEL_K_BRUTE && (FIRST || DYN)) fill_tables_lds(a.sc, tab_lds, SEG);  // (DYN: no barrier in the walk)

    const uint32_t cap = a.cap;
    const Rsrc r_in = make_rsrc(a.in, a.state_cap * (N_STATE * 4u)), r_out = make_rsrc(a.out, a.state_cap * (N_STATE * 4u));
    const Rsrc r_L = make_rsrc(a.Lhome, cap * 16u);
    uint32_t out_off = 0;      // survivors written so far (front of this region of the `out` state)
    uint32_t ns_acc = 0, nh_acc = 0, live_acc = 0, mid_acc = 0, mid_acc_hi = 0;
    const uint32_t nb_run = NB > 1 ? min(a.nb, (uint32_t)MAX_CHAIN) : 1u;  // bounces this launch walks
    // the region's live paths sit compacted at its front: walk them SEG at a time; dead slots cost nothing
    for (uint32_t it0 = 0; it0 < (REGION > SEG ? cnt_in : 1u); it0 += CH) {  // single trip when REGION == SEG
    if (DYN) {  // take the next 64-path chunk of the region from the workgroup's queue
        uint32_t nxt = 0;
        if ((tid & 63u) == 0) nxt = atomicAdd(&q_in, 64u);
        it0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)nxt);
        if (it0 >= cnt_in) break;
    }
    const uint32_t buf = (it0 / SEG) & 1u;
    const bool alive = it0 + lane_c < cnt_in;
    const uint32_t slot = base + it0 + lane_c;
    bool survive = false;
    bool did_seg = false, did_shadow = false;
    V3 o, d, thr, L;
    float eta, prev_pdf, tmax;
    uint32_t home = slot;
    uint32_t ka = 0, kb = 0, px = 0, py = 0;
    if (alive) {
        if (FIRST) {
            home = slot;
            camera_start(a, home, &ka, &kb, &o, &d, &tmax, &thr, &L, &eta, &prev_pdf);
        } else {
            const uint32_t v4 = state_voff(slot);
            constexpr uint32_t row = STATE_ROW_BYTES;
            STATE_LOAD(STATE_BLD, o, d, thr, L, eta, prev_pdf, home);
            tmax = (a.key_mode == 1 && a.depth == 0) ? eta : K_INF;  // caller rays: ST_ETA
            if (a.key_mode == 1 && a.depth == 0) eta = 1.0f;
        }
    }
    // shading tables -> LDS, behind the state loads so that the two memory round trips overlap
    if (ACCEL == ACCEL_K_BRUTE && !FIRST && !DYN && it0 == 0) fill_tables_lds(a.sc, tab_lds, live_threads);
    if (alive && !FIRST) path_key(a, home, &ka, &kb, &px, &py);
    bool live = alive;                        // the lane still carries a path
    uint32_t keep = 0xffffffffu;
    if (FIRST && ACCEL == ACCEL_K_BRUTE && !DYN && a.tile_keep) keep = camera_keep_word(a, base, tid);
    uint32_t nseg_w = 0, nshd_w = 0, nmid_w = 0, nmid_hi_w = 0;  // wave-uniform counts over the launch's bounces
#pragma unroll 1
    for (uint32_t bounce = 0; bounce < nb_run; ++bounce) {
    const uint32_t depth = a.depth + bounce;
    if (NB > 1 && bounce > 0) {
        if (depth >= a.max_depth) break;      // uniform
        const uint32_t n_on = (uint32_t)__popcll(__ballot(live));
        if (bounce <= 3)
            nmid_w += n_on << (10u * (bounce - 1u));
        else
            nmid_hi_w += n_on << (10u * (bounce - 4u));
        tmax = K_INF;
    }
    did_seg = false;
    did_shadow = false;
    survive = false;
    if (live) {
#ifdef PBRT_PROBE_EXTRA_VALU  // diagnostic builds only: N dependent full-rate VALU instructions per live wave-bounce
        {
            float probe = o.x;
#pragma unroll
            for (int k = 0; k < PBRT_PROBE_EXTRA_VALU; ++k) asm volatile("v_add_f32 %0, %0, %0" : "+v"(probe));
            if (probe == 12345.678f) o.x = probe;  // never true; keeps the chain alive
        }
#endif
        survive = bounce_step<ACCEL, false, GL, ORD>(a, tb, ls, r_L, depth, ka, kb, home, tmax, o, d, thr, L, eta, prev_pdf, did_seg, did_shadow,
                                                nullptr, keep);
    }
    keep = 0xffffffffu;  // the later bounces of the launch are no camera rays
    live = survive;
    nseg_w += (uint32_t)__popcll(__ballot(did_seg));
    nshd_w += (uint32_t)__popcll(__ballot(did_shadow));
    }  // bounces of this launch
    // ---- segment-local stream compaction: ballot + mbcnt inside the wave, LDS scan across waves
    const uint32_t wid = tid >> 6;
    const unsigned long long bal = __ballot(survive);
    const uint32_t prefix = ballot_rank(bal);
    uint32_t off = 0, total = 0;
    if (DYN) {  // reserve the survivors' slots in the region with one returning LDS atomic per wave and chunk
        const uint32_t cnt_w = (uint32_t)__popcll(bal);
        uint32_t got = 0;
        if ((tid & 63u) == 0 && cnt_w) got = atomicAdd(&q_out, cnt_w);
        off = (uint32_t)__builtin_amdgcn_readfirstlane((int)got);
        ns_acc += nseg_w;
        nh_acc += nshd_w;
        live_acc += (uint32_t)__popcll(__ballot(alive));
    } else {
    if ((tid & 63) == 0) {
        wave_tot[buf][wid] = (uint32_t)__popcll(bal);
        wave_seg[buf][wid] = nseg_w;
        wave_shd[buf][wid] = nshd_w;
        if (NB > 1) {
            wave_mid[buf][wid] = nmid_w;
            wave_mid_hi[buf][wid] = nmid_hi_w;
        }
    }
    __syncthreads();
        WAVE_SCAN(W, wave_tot[buf], tid, wid, off, total);
    }
    if (survive) {
        const uint32_t v4 = state_voff(base + out_off + off + prefix);
        constexpr uint32_t row = STATE_ROW_BYTES;
        STATE_STORE(STATE_BST, o, d, thr, L, eta, prev_pdf, home);
    }
    out_off += total;
    if (!DYN && tid == 0) {
        for (uint32_t w = 0; w < SEG / 64; ++w) {
            ns_acc += wave_seg[buf][w];
            nh_acc += wave_shd[buf][w];
            if (NB > 1) {
                mid_acc += wave_mid[buf][w];
                mid_acc_hi += wave_mid_hi[buf][w];
            }
        }
    }
    }  // chunk loop
    if (DYN) {
        if ((tid & 63u) == 0) {
            unsigned long long *row = a.stats + row_id;  // per-wave statistics rows
            const size_t stride = a.stat_stride;
            row[0] += ns_acc;
            row[stride] += nh_acc;
            row[(2 + min(a.depth, (uint32_t)MAX_DEPTH_STATS - 1)) * stride] += live_acc;
            // the last wave to finish publishes the region's survivor count (LDS atomics of one CU are ordered)
            if (atomicAdd(&q_done, 1u) == W - 1) a.seg_out[seg] = atomicAdd(&q_out, 0u);
        }
        return;
    }
    if (tid == 0) {
        a.seg_out[seg] = out_off;
        // per-region statistics rows (plain read-modify-write by the owning workgroup; launches of a
        // call are ordered on the stream).  NOT global atomics: 3 same-line atomics per workgroup
        // serialise at ~12 ns each and were the whole kernel time (DESIGN.md "What did not work").
        unsigned long long *row = a.stats + row_id;
        const size_t stride = a.stat_stride;
        row[0] += ns_acc;
        row[stride] += nh_acc;
        row[(2 + min(a.depth, (uint32_t)MAX_DEPTH_STATS - 1)) * stride] += cnt_in;
        if (NB > 1)
            for (uint32_t k = 1; k < nb_run; ++k) {
                const uint32_t n_on = k <= 3 ? (mid_acc >> (10u * (k - 1u))) & 1023u : (mid_acc_hi >> (10u * (k - 4u))) & 1023u;
                row[(2 + min(a.depth + k, (uint32_t)MAX_DEPTH_STATS - 1)) * stride] += n_on;
            }
    }
}

// ---- k_path: camera paths of an ACCEL_K_BRUTE scene walked to their end in ONE launch --------------------------------------------
// When the fuse plan walks every bounce of a pass in one launch (max_depth <= MAX_CHAIN) no path outlives the launch: there is
// nothing to compact, no state to write and no survivor count to publish.  k_path is that launch without the machinery:
// camera_start, camera_keep_word and bounce_step as k_bounce<true, .., 2> calls them, in the same order (same film, bit for bit), but
//   * no barrier after the one that ends the table staging: the waves of a workgroup end on their own, and their slots are free
//     for the next workgroup's waves at once;
//   * a lane keeps L when its path ends and the wave stores its 64 records after the bounce loop, 1 KiB contiguous;
//   * the waves add their counts to workgroup counters in LDS and the last one to arrive adds them to the workgroup's statistics
//     row (row = workgroup of the launch: stat_stride >= gridDim.x);
//   * an argument block of its own.  (DevScene stays whole -- brute_intersect takes it -- but its BVH members are never loaded.)
// THREADS: the workgroup size (PATH_THREADS is what the host launches); the pass is cut into workgroups of THREADS consecutive homes.
// Measured on MI355X, cbox 512^2 x 256 spp (profiles/path_kernel.md): 5.88 -> 5.70 ms per step against k_bounce<true, 5, 2>, the store
// after the loop alone 0.14 ms of it; 512 / 256 / 128 / 64 threads -> 5.71 / 5.71 / 5.98 / 6.04 ms (the table staging per workgroup).
#ifndef PATH_THREADS
#define PATH_THREADS 512
#endif
static_assert(SEG_BRUTE % PATH_THREADS == 0 && PATH_THREADS % 64 == 0, "a region of the brute-force kernels is whole k_path workgroups");
// k_path workgroups (and statistics rows) per region of the brute-force kernels
__host__ __device__ constexpr uint32_t path_groups_per_region() { return SEG_BRUTE / PATH_THREADS; }
struct PathArgs {
    DevScene sc;
    pbrt_camera cam;
    float *Lhome;               // [cap] float4 records (r, g, b, 0) indexed by home
    unsigned long long *stats;  // as RadArgs::stats; one row per workgroup of the launch
    const uint32_t *tile_keep;  // as RadArgs::tile_keep
    uint32_t stat_stride, cap, n_paths, max_depth, rr_depth, seed;
    FilmKey key;
    static constexpr uint32_t key_mode = 0, index_offset = 0, sample_index = 0;  // (path_key)
};
static_assert(offsetof(PathArgs, seed) == 252 && offsetof(PathArgs, key) == 256 && sizeof(PathArgs) == 320, "PathArgs keeps its bytes");
// what k_path reads of the arguments of a bounce launch (host)
static inline PathArgs path_args(const RadArgs &a) {
    PathArgs p;
    p.sc = a.sc;
    p.cam = a.cam;
    p.Lhome = a.Lhome;
    p.stats = a.stats;
    p.tile_keep = a.tile_keep;
    p.stat_stride = a.stat_stride;
    p.cap = a.cap;
    p.n_paths = a.n_paths;
    p.max_depth = a.max_depth;
    p.rr_depth = a.rr_depth;
    p.seed = a.seed;
    p.key = a.key;
    return p;
}
template <int ACCEL_T, int THREADS>
__global__ __launch_bounds__(THREADS, FUSED_WAVES_PER_EU) void k_path(const PathArgs a) {
    static_assert(ACCEL_T == ACCEL_K_BRUTE || ACCEL_T == ACCEL_K_BRUTE_ORDERED, "k_path: ACCEL_K_BRUTE scenes without glossy materials");
    constexpr bool ORD = ACCEL_T == ACCEL_K_BRUTE_ORDERED;
    constexpr uint32_t W = THREADS / 64;
    __shared__ uint32_t tab_lds[TAB_DW];
    __shared__ uint32_t wg_cnt[2 + MAX_CHAIN];  // segments, shadow rays, paths that went on to bounce 1 .. MAX_CHAIN - 1; [1 + MAX_CHAIN]: waves done
    const uint32_t wg = xcd_swizzle(blockIdx.x, gridDim.x);
    const uint32_t tid = threadIdx.x;
    const uint32_t base = wg * THREADS;
    if (base >= a.n_paths) return;  // uniform across the workgroup; its row gets nothing
    const uint32_t cnt_in = min(a.n_paths - base, (uint32_t)THREADS);
    if (tid < 2 + MAX_CHAIN) wg_cnt[tid] = 0;
    const LdsScene ls = NO_LDS_SCENE;
    const Tables tb = stage_tables_lds(a.sc, tab_lds);
    fill_tables_lds(a.sc, tab_lds, THREADS);  // ends with the only barrier of the kernel

    const bool alive = tid < cnt_in;
    const uint32_t home = base + tid;
    V3 o = {0, 0, 0}, d = {0, 0, 1}, thr = {1, 1, 1}, L = {0, 0, 0};
    float eta = 1.0f, prev_pdf = -1.0f, tmax = K_INF;
    uint32_t ka = 0, kb = 0;
    if (alive) camera_start(a, home, &ka, &kb, &o, &d, &tmax);
    uint32_t keep = 0xffffffffu;
    if (a.tile_keep) keep = camera_keep_word(a, base, tid);
    bool live = alive;
    uint32_t nseg_w = 0, nshd_w = 0;
    unsigned long long non_w = 0;  // paths of the wave that went on to bounce k (1 .. MAX_CHAIN - 1): 8 bits each
    static_assert(8 * (MAX_CHAIN - 1) <= 64, "the per-bounce counts of a wave (<= 64 each) are packed 8 bits each");
    const uint32_t nb_run = min(a.max_depth, (uint32_t)MAX_CHAIN);
#pragma unroll 1
    for (uint32_t depth = 0; depth < nb_run; ++depth) {
        if (depth > 0) {
            const uint32_t n_on = (uint32_t)__popcll(__ballot(live));
            if (n_on == 0) break;  // uniform: every path of the wave has ended
            non_w += (unsigned long long)n_on << (8u * (depth - 1u));
            tmax = K_INF;
        }
        bool did_seg = false, did_shadow = false, survive = false;
        if (live)
            survive = bounce_step<ACCEL_K_BRUTE, false, false, ORD, false>(a, tb, ls, Rsrc(), depth, ka, kb, home, tmax, o, d, thr, L, eta, prev_pdf,
                                                                           did_seg, did_shadow, nullptr, keep);
        keep = 0xffffffffu;  // the later bounces are no camera rays
        live = survive;
        nseg_w += (uint32_t)__popcll(__ballot(did_seg));
        nshd_w += (uint32_t)__popcll(__ballot(did_shadow));
    }
    // one record per path, 64 consecutive homes per wave
    if (alive) store_record(make_rsrc(a.Lhome, a.cap * 16u), home, L);
    // statistics: every wave adds its counts to the workgroup's, the last one to arrive adds those to the row (LDS atomics of one
    // CU are ordered, as the q_done of k_bounce's chunk queue relies on); nobody waits
    if ((tid & 63u) == 0) {
        if (nseg_w) atomicAdd(&wg_cnt[0], nseg_w);
        if (nshd_w) atomicAdd(&wg_cnt[1], nshd_w);
#pragma unroll
        for (uint32_t k = 1; k < MAX_CHAIN; ++k) {
            const uint32_t n_on = (uint32_t)(non_w >> (8u * (k - 1u))) & 255u;
            if (n_on) atomicAdd(&wg_cnt[1 + k], n_on);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (atomicAdd(&wg_cnt[1 + MAX_CHAIN], 1u) == W - 1) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            unsigned long long *row = a.stats + wg;
            const size_t stride = a.stat_stride;
            unsigned long long v[2 + MAX_CHAIN];
            uint32_t add[2 + MAX_CHAIN];
#pragma unroll
            for (uint32_t k = 0; k < 2 + MAX_CHAIN; ++k) {  // rows 0, 1: segments, shadow rays; 2 + dpt: paths entering depth dpt
                add[k] = k == 2 ? cnt_in : atomicAdd(&wg_cnt[k < 2 ? k : k - 1], 0u);
                if (k < 2 + nb_run) v[k] = row[k * stride];
            }
#pragma unroll
            for (uint32_t k = 0; k < 2 + MAX_CHAIN; ++k)
                if (k < 2 + nb_run) row[k * stride] = v[k] + add[k];
        }
    }
}

// The keep table of a radiance render of an ACCEL_K_BRUTE scene (RadArgs::tile_keep): word b = which of the <= 32 primitives the
// camera rays of region indices [64 b, 64 b + 63] can meet, bit i = primitive i of sc.prims (tile_cull.h decides, in double; a
// cleared bit is a proof that the float test rejects).  The rectangle of a block is the bounding box of its 64 pixels through
// region_pixel, as path_key hands them to a wave: one 8 x 8 tile when the region's width is a multiple of 8, a few tiles or a piece
// of the row-major tail otherwise.  One thread per word; a render runs it once, ahead of its first pass (microseconds).
struct TileKeepArgs {
    const pbrt_prim *prims;
    uint32_t n_prims;  // <= 32
    pbrt_camera cam;
    FilmKey key;
    uint32_t n_blocks;  // key.npix_r / 64
    uint32_t *keep;     // [n_blocks]
};
__global__ __launch_bounds__(64) void k_tile_keep(const TileKeepArgs a) {
    const uint32_t blk = blockIdx.x * 64u + threadIdx.x;
    if (blk >= a.n_blocks) return;
    uint32_t x0 = 0xffffffffu, y0 = 0xffffffffu, x1 = 0, y1 = 0;
    for (uint32_t k = 0; k < 64u; ++k) {
        uint32_t rx, ry;
        region_pixel(a.key, blk * 64u + k, &rx, &ry);
        x0 = min(x0, rx);
        x1 = max(x1, rx);
        y0 = min(y0, ry);
        y1 = max(y1, ry);
    }
    uint32_t word = 0;
    for (uint32_t i = 0; i < a.n_prims && i < 32u; ++i) {
        const pbrt_prim P = load_prim_uniform(a.prims + i);
        if (tile_cull_keep(a.cam, a.key.rx0 + x0, a.key.ry0 + y0, a.key.rx0 + x1, a.key.ry0 + y1, P)) word |= 1u << i;
    }
    word |= a.n_prims < 32u ? ~0u << a.n_prims : 0u;  // bits without a primitive stay set: a full word means "nothing culled"
    a.keep[blk] = word;
}

// column sums of the per-segment statistics: out[k] += sum_seg stats[k][seg].  grid (rows, REDUCE_SLICES): every block sums
// one slice of a row and adds it to the row's total with one 64-bit atomic (out is zeroed by the caller; a single block
// per row took 55 us for the 32 Ki rows of a 16 Mi-path pass, on the host's critical path of every call)
#define REDUCE_SLICES 32
__global__ __launch_bounds__(256) void k_reduce_stats(const unsigned long long *stats, uint32_t nseg, size_t stride,
                                                      unsigned long long *out) {
    __shared__ unsigned long long part[256];
    const unsigned long long *row = stats + (size_t)blockIdx.x * stride;
    const uint32_t per = (nseg + gridDim.y - 1) / gridDim.y, lo = min(blockIdx.y * per, nseg), hi = min(lo + per, nseg);
    unsigned long long s = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) s += row[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0 && part[0]) atomicAdd(&out[blockIdx.x], part[0]);
}

// The ultrasound acquisition's form (round 5): slice s of row r leaves its partial sum in out[r * REDUCE_SLICES + s] -- `out` is the
// context's pinned host page, written by the kernel itself, the host adds the slices -- and ZEROES the counters it has read, so that
// the next acquisition finds its rows clean.  No fill command in front of the counters and no copy command behind them: at one path
// per ray (USMain.py:36) those two were 9 of the 60 us an acquisition kept the device.
__global__ __launch_bounds__(256) void k_us_reduce_stats(unsigned long long *stats, uint32_t nseg, size_t stride,
                                                         unsigned long long *out) {
    __shared__ unsigned long long part[4];
    unsigned long long *row = stats + (size_t)blockIdx.x * stride;
    const uint32_t per = (nseg + gridDim.y - 1) / gridDim.y, lo = min(blockIdx.y * per, nseg), hi = min(lo + per, nseg);
    unsigned long long s = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) {
        s += row[i];
        row[i] = 0ull;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = part[0] + part[1] + part[2] + part[3];
}

// ---- film: deterministic gather of the pass's samples through the reconstruction filter -----------
struct FilmArgs {
    const float *Lhome;  // [cap] float4 records (r, g, b, 0)
    float *acc;          // [4][cw*ch] running sums (w*r, w*g, w*b, w)
    uint32_t cap;
    uint32_t cx0, cy0, cw, ch;     // crop
    FilmKey key;                   // the pass's: region, pixel order of Lhome (region_index), first sample
    uint32_t rh;                   // rows of the region
    uint32_t s_count, filter, seed;
};

DEV float filter_1d(uint32_t f, float x) {
    if (f == PBRT_FILTER_TENT) return fmaxf(0.0f, 1.0f - fabsf(x));
    const float alpha = -2.0f;
    return fmaxf(0.0f, expf(alpha * x * x) - expf(alpha * 4.0f));
}

__global__ __launch_bounds__(256) void k_film_accum(const FilmArgs a) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.cw * a.ch) return;
    const uint32_t iy = idx / a.cw, ix = idx - iy * a.cw;
    const int x = (int)(a.cx0 + ix), y = (int)(a.cy0 + iy);
    const uint32_t npx = a.cw * a.ch;
    float ar = a.acc[idx], ag = a.acc[npx + idx], ab = a.acc[2 * npx + idx], aw = a.acc[3 * npx + idx];
    const int R = a.filter == PBRT_FILTER_BOX ? 0 : (a.filter == PBRT_FILTER_TENT ? 1 : 2);
    const float ccx = (float)x + 0.5f, ccy = (float)y + 0.5f;
    for (uint32_t sl = 0; sl < a.s_count; ++sl) {
        const uint32_t s_idx = a.key.s_first + sl;
        const float4 *Ls = reinterpret_cast<const float4 *>(a.Lhome) + (size_t)sl * a.key.npix_r;
        for (int ny = y - R; ny <= y + R; ++ny)
            for (int nx = x - R; nx <= x + R; ++nx) {
                if (nx < 0 || ny < 0 || nx >= (int)a.key.film_w || ny >= (int)a.key.film_h) continue;
                float w = 1.0f;
                if (a.filter != PBRT_FILTER_BOX) {
                    F4 uj = rng4((uint32_t)ny * a.key.film_w + (uint32_t)nx, s_idx, 0, a.seed);
                    float px = (float)nx + uj.x, py = (float)ny + uj.y;
                    w = filter_1d(a.filter, ccx - px) * filter_1d(a.filter, ccy - py);
                }
                if (w > 0.0f) {
                    const uint32_t k = region_index((uint32_t)(nx - (int)a.key.rx0), (uint32_t)(ny - (int)a.key.ry0), a.key.rw, a.key.tile_rows);
                    const float4 Lk = Ls[k];
                    ar = fma_(w, Lk.x, ar);
                    ag = fma_(w, Lk.y, ag);
                    ab = fma_(w, Lk.z, ab);
                    aw += w;
                }
            }
    }
    a.acc[idx] = ar;
    a.acc[npx + idx] = ag;
    a.acc[2 * npx + idx] = ab;
    a.acc[3 * npx + idx] = aw;
}

// Tiled form for the tent / gaussian filters: a TILE x TILE pixel tile per workgroup (16; 8 when the crop has too
// few 16 x 16 tiles to fill the GPU -- the sample loop of a tile is sequential, and e.g. one rank's 512 x 64 band
// of an 8-GPU job at 2048 spp spent 4.9 of 13.5 ms in 128 workgroups).  Per sample index the
// workgroup evaluates the jitter hash ONCE per pixel of the haloed tile (not once per gathering
// neighbour: 1.3 instead of 9 / 25 hashes per thread) and stages (film x, film y, r, g, b) in LDS; every
// thread then gathers its (2R+1)^2 neighbourhood from LDS in the same fixed order as k_film_accum, so the
// sums are bit-identical.  Double-buffered: one barrier per sample.
#define FILM_RMAX 2
template <int FILM_TILE, int FILTER>  // the filter is a template parameter: radius and tap loops are compile-time
__global__ __launch_bounds__(FILM_TILE *FILM_TILE) void k_film_accum_tiled(const FilmArgs a) {
    constexpr int FILM_TW = FILM_TILE + 2 * FILM_RMAX;
    // LDS image of the haloed tile, one plane per component, rows padded to a stride that puts the rows a half-wave
    // reads at once (32 lanes: 2 rows of 16 / 4 rows of 8) on disjoint banks (AoS [entry][5] measured 39 % of the LDS
    // cycles in bank conflicts)
    constexpr int LS = FILM_TILE == 16 ? 48 : 40;
    static_assert(LS >= FILM_TW, "row stride covers the haloed row");
    __shared__ float tile[2][5][FILM_TW * LS];
    constexpr int R = FILTER == PBRT_FILTER_TENT ? 1 : 2;
    constexpr int TW = FILM_TILE + 2 * R;
    const uint32_t tid = threadIdx.y * FILM_TILE + threadIdx.x;
    const int tx0 = (int)(a.cx0 + blockIdx.x * FILM_TILE), ty0 = (int)(a.cy0 + blockIdx.y * FILM_TILE);  // film coords of the tile
    const int x = tx0 + (int)threadIdx.x, y = ty0 + (int)threadIdx.y;
    const bool inside = x < (int)(a.cx0 + a.cw) && y < (int)(a.cy0 + a.ch);
    const uint32_t npx = a.cw * a.ch;
    const uint32_t idx = inside ? (uint32_t)(y - (int)a.cy0) * a.cw + (uint32_t)(x - (int)a.cx0) : 0u;
    float ar = 0, ag = 0, ab = 0, aw = 0;
    if (inside) {
        ar = a.acc[idx];
        ag = a.acc[npx + idx];
        ab = a.acc[2 * npx + idx];
        aw = a.acc[3 * npx + idx];
    }
    const float ccx = (float)x + 0.5f, ccy = (float)y + 0.5f;
    // staging duty of this thread: haloed-tile entries tid, tid + NT, ... (NST of them); everything that does not
    // depend on the sample index is computed once, and the radiance record of sample sl + 1 is requested before
    // sample sl is staged and gathered, so the HBM / L2 round trip is off the per-sample critical path
    constexpr int NT = FILM_TILE * FILM_TILE, NST = (FILM_TW * FILM_TW + NT - 1) / NT;
    bool st_in[NST], st_valid[NST];
    uint32_t st_key[NST], st_k[NST];
    float st_x[NST], st_y[NST];
    int st_lds[NST];
#pragma unroll
    for (int j = 0; j < NST; ++j) {
        const int i = (int)tid + j * NT;
        const int nx = tx0 - R + i % TW, ny = ty0 - R + i / TW;
        st_lds[j] = (i / TW) * LS + i % TW;
        st_in[j] = i < TW * TW;
        st_valid[j] = st_in[j] && nx >= (int)a.key.rx0 && ny >= (int)a.key.ry0 && nx < (int)(a.key.rx0 + a.key.rw) && ny < (int)(a.key.ry0 + a.rh);
        st_key[j] = (uint32_t)ny * a.key.film_w + (uint32_t)nx;
        st_k[j] = st_valid[j] ? region_index((uint32_t)(nx - (int)a.key.rx0), (uint32_t)(ny - (int)a.key.ry0), a.key.rw, a.key.tile_rows) : 0u;
        st_x[j] = (float)nx;
        st_y[j] = (float)ny;
    }
    const float4 *Lrec = reinterpret_cast<const float4 *>(a.Lhome);
    const float4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    // radiance records of the next PF samples, requested PF iterations ahead: one iteration is shorter than an HBM / L2
    // round trip (with a distance of one the loop ran at 2.3 us per sample whatever the workgroup count)
#ifndef FILM_PF
#define FILM_PF 4
#endif
    constexpr int PF = FILM_PF;
    float4 Lq[PF][NST];
#pragma unroll
    for (int u = 0; u < PF; ++u)
#pragma unroll
        for (int j = 0; j < NST; ++j)
            Lq[u][j] = (st_valid[j] && (uint32_t)u < a.s_count) ? Lrec[(size_t)u * a.key.npix_r + st_k[j]] : zero4;
    for (uint32_t sl0 = 0; sl0 < a.s_count; sl0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const uint32_t sl = sl0 + (uint32_t)u;
            if (sl >= a.s_count) break;
            const uint32_t s_idx = a.key.s_first + sl;
            float(*T)[FILM_TW * LS] = tile[sl & 1];
#pragma unroll
            for (int j = 0; j < NST; ++j) {
                if (!st_in[j]) continue;
                const int i = st_lds[j];
                float px = 1e30f, py = 1e30f;  // outside the film / rendered region: weight 0
                if (st_valid[j]) {
                    F4 uj = rng4(st_key[j], s_idx, 0, a.seed);
                    px = st_x[j] + uj.x;
                    py = st_y[j] + uj.y;
                }
                T[0][i] = px;
                T[1][i] = py;
                T[2][i] = Lq[u][j].x;
                T[3][i] = Lq[u][j].y;
                T[4][i] = Lq[u][j].z;
            }
#pragma unroll
            for (int j = 0; j < NST; ++j)
                Lq[u][j] = (st_valid[j] && sl + PF < a.s_count) ? Lrec[(size_t)(sl + PF) * a.key.npix_r + st_k[j]] : zero4;
            __syncthreads();
            if (inside) {
                const int e0 = (int)threadIdx.y * LS + (int)threadIdx.x;
#pragma unroll
                for (int dy = 0; dy <= 2 * R; ++dy)
#pragma unroll
                    for (int dx = 0; dx <= 2 * R; ++dx) {
                        const int e = e0 + dy * LS + dx;
                        float w = filter_1d(FILTER, ccx - T[0][e]) * filter_1d(FILTER, ccy - T[1][e]);
                        if (w > 0.0f) {
                            ar = fma_(w, T[2][e], ar);
                            ag = fma_(w, T[3][e], ag);
                            ab = fma_(w, T[4][e], ab);
                            aw += w;
                        }
                    }
            }
        }
    }
    if (inside) {
        a.acc[idx] = ar;
        a.acc[npx + idx] = ag;
        a.acc[2 * npx + idx] = ab;
        a.acc[3 * npx + idx] = aw;
    }
}

__global__ __launch_bounds__(256) void k_film_resolve(const float *acc, float *out, uint32_t npx, uint32_t raw) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npx) return;
    float r = acc[idx], g = acc[npx + idx], b = acc[2 * npx + idx], w = acc[3 * npx + idx];
    if (raw) {
        out[4 * idx] = r;
        out[4 * idx + 1] = g;
        out[4 * idx + 2] = b;
        out[4 * idx + 3] = w;
    } else {
        float inv = w > 0.0f ? 1.0f / w : 0.0f;
        out[3 * idx] = r * inv;
        out[3 * idx + 1] = g * inv;
        out[3 * idx + 2] = b * inv;
    }
}

// upload of caller rays for Integrator.sample(): o,d [3][n] SoA + tmax -> state slots
// region: slots per live counter (a region, or the part of it one wave owns); n_cnt counters
__global__ __launch_bounds__(256) void k_init_rays(float *st, uint32_t *seg_cnt, uint32_t n_cnt, uint32_t region, uint32_t n,
                                                   const float *o, const float *d, const float *tmax) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_cnt) seg_cnt[i] = n > i * region ? min(n - i * region, region) : 0u;
    if (i >= n) return;
    float *s = st + (state_voff(i) >> 2);  // tiled SoA: row k at +64 * k floats
    s[(ST_O + 0) * 64] = o[i];
    s[(ST_O + 1) * 64] = o[n + i];
    s[(ST_O + 2) * 64] = o[2 * n + i];
    s[(ST_D + 0) * 64] = d[i];
    s[(ST_D + 1) * 64] = d[n + i];
    s[(ST_D + 2) * 64] = d[2 * n + i];
    s[(ST_THR + 0) * 64] = 1.0f;
    s[(ST_THR + 1) * 64] = 1.0f;
    s[(ST_THR + 2) * 64] = 1.0f;
    s[(ST_L + 0) * 64] = 0.0f;
    s[(ST_L + 1) * 64] = 0.0f;
    s[(ST_L + 2) * 64] = 0.0f;
    s[ST_ETA * 64] = tmax[i];  // a caller ray: the first bounce takes the row as tmax
    s[ST_PDF * 64] = -1.0f;
    s[ST_HOME * 64] = __uint_as_float(i);
}
