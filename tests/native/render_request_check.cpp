// Host check of csrc/render_request.h (tests/test_render_request_host.py builds and runs it under the sanitizers): the argument rules
// of a radiance render with their texts and their order, the rendered region and its film key against a per-pixel restatement, the
// pixel order against its inverse (csrc/film_key.h region_index / region_pixel) over every small region, the shape of a pass
// and its halving, the pass schedule, the fuse plan, the default pass size, the stream grids and the byte models of pbrt_stats
// against literals worked by hand.  Prints one JSON line: {"checks": N, "failures": M}.
#include <cstdio>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "render_request.h"

static int checks = 0, failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        ++checks;                                                     \
        if (!(cond)) {                                                \
            ++failures;                                               \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);   \
        }                                                             \
    } while (0)

// the refusal texts, as the driver's NEED lines always stringified them
static const char *T_NULL = "cam && f && d_out";
static const char *T_SIZES = "W > 0 && H > 0 && f->crop_w > 0 && f->crop_h > 0";
static const char *T_CROP = "(uint64_t)f->crop_x + f->crop_w <= W && (uint64_t)f->crop_y + f->crop_h <= H";
static const char *T_COUNTS = "f->spp > 0 && f->max_depth > 0 && f->filter <= PBRT_FILTER_GAUSSIAN";
static const char *T_FILM = "(uint64_t)W * H <= 0xffffffffull";
static const char *T_SHAPE = "unit * k < 0xfffffc00ull";
static const char *T_STATE = "wavefront || (uint64_t)cap * N_STATE * 4 < 0xffffffffull";
static const char *T_DEAD = "cap < WF_DEAD";

static const RenderLaunch BRUTE{true, true, 512, 1, 1, 4}, BRUTE_BIG{true, false, 512, 1, 1, 4}, BVH{false, false, 4096, 1, 16, 4};
static const uint32_t WF_DEAD_ = 0x40000000u, KMAX = 21;

static pbrt_camera camera(uint32_t W, uint32_t H) {
    pbrt_camera cam;
    std::memset(&cam, 0, sizeof cam);
    cam.film_w = W, cam.film_h = H;
    return cam;
}
static pbrt_film_desc film(uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t filter = PBRT_FILTER_TENT) {
    pbrt_film_desc f;
    std::memset(&f, 0, sizeof f);
    f.crop_x = x, f.crop_y = y, f.crop_w = w, f.crop_h = h, f.spp = 4, f.max_depth = 6, f.rr_depth = 5, f.filter = filter;
    return f;
}
static const char *text_of(const pbrt_camera *cam, const pbrt_film_desc *f, bool d_out = true) {
    RenderRequest rq;
    const char *why = render_request(&rq, cam, f, d_out, BRUTE);
    return why ? why : "";
}
static bool is(const char *got, const char *want) { return got && std::strcmp(got, want) == 0; }

static void rule_table() {
    pbrt_camera cam = camera(16, 16);
    pbrt_film_desc f = film(0, 0, 16, 16);
    CHECK(is(text_of(&cam, &f), ""));
    CHECK(is(text_of(nullptr, &f), T_NULL) && is(text_of(&cam, nullptr), T_NULL) && is(text_of(&cam, &f, false), T_NULL));
    struct Case {
        const char *want;
        uint32_t W, H, x, y, w, h, spp, depth, filter;
    };
    const uint32_t BIG = 0xfffffff8u;
    const Case cases[] = {
        {T_SIZES, 0, 16, 0, 0, 16, 16, 4, 6, 1},         {T_SIZES, 16, 0, 0, 0, 16, 16, 4, 6, 1},
        {T_SIZES, 16, 16, 0, 0, 0, 16, 4, 6, 1},         {T_SIZES, 16, 16, 0, 0, 16, 0, 4, 6, 1},
        {T_CROP, 16, 16, 1, 0, 16, 16, 4, 6, 1},         {T_CROP, 16, 16, 0, 1, 16, 16, 4, 6, 1},
        {T_CROP, 16, 16, BIG, 0, 16, 16, 4, 6, 1},       {T_CROP, 16, 16, 0, BIG, 16, 16, 4, 6, 1},  // both sums pass 2^32
        {T_CROP, 16, 16, 8, 0, BIG, 16, 4, 6, 1},        {T_CROP, 16, 16, 0, 8, 16, BIG, 4, 6, 1},
        {T_COUNTS, 16, 16, 0, 0, 16, 16, 0, 6, 1},       {T_COUNTS, 16, 16, 0, 0, 16, 16, 4, 0, 1},
        {T_COUNTS, 16, 16, 0, 0, 16, 16, 4, 6, 3},       {T_COUNTS, 16, 16, 0, 0, 16, 16, 4, 6, 0xffffffffu},
        {T_FILM, 65536, 65536, 0, 0, 16, 16, 4, 6, 1},   {T_FILM, 0xffffffffu, 2, 0, 0, 16, 2, 4, 6, 1},
        {"", 65535, 65537, 0, 0, 16, 16, 4, 6, 1},       {"", 0xffffffffu, 1, BIG, 0, 7, 1, 4, 6, 2},  // 2^32 - 1 pixels: taken
        // two rules broken: the earlier one speaks
        {T_SIZES, 0, 16, 0, 0, 16, 16, 0, 6, 1},         {T_SIZES, 16, 16, 20, 0, 0, 16, 4, 6, 1},
        {T_CROP, 16, 16, 0, 1, 16, 16, 4, 6, 7},         {T_CROP, 65536, 65536, 65530, 0, 16, 16, 4, 6, 1},
        {T_COUNTS, 65536, 65536, 0, 0, 16, 16, 0, 6, 1},
    };
    for (const Case &k : cases) {
        cam = camera(k.W, k.H);
        f = film(k.x, k.y, k.w, k.h, k.filter);
        f.spp = k.spp, f.max_depth = k.depth;
        CHECK(is(text_of(&cam, &f), k.want));
        if (*k.want) CHECK(is(text_of(nullptr, &f), T_NULL) && is(text_of(&cam, &f, false), T_NULL));  // the null rule is the first
    }
}

// the region of a crop: every film pixel within the filter's radius of a crop pixel, counted one by one
static void region_of(uint32_t W, uint32_t H, const pbrt_film_desc &f, const RenderLaunch &launch, uint32_t flags) {
    pbrt_camera cam = camera(W, H);
    pbrt_film_desc fd = f;
    fd.flags = flags;
    RenderRequest rq;
    CHECK(render_request(&rq, &cam, &fd, true, launch) == nullptr);
    const int64_t R = f.filter == PBRT_FILTER_BOX ? 0 : f.filter == PBRT_FILTER_TENT ? 1 : 2;
    CHECK(rq.radius == (uint32_t)R);
    uint64_t inside = 0, outside_hit = 0;
    int64_t x0 = W, y0 = H, x1 = -1, y1 = -1;
    for (int64_t y = 0; y < (int64_t)H; ++y)
        for (int64_t x = 0; x < (int64_t)W; ++x) {
            const bool near_crop = x >= (int64_t)f.crop_x - R && x < (int64_t)f.crop_x + f.crop_w + R && y >= (int64_t)f.crop_y - R &&
                                   y < (int64_t)f.crop_y + f.crop_h + R;
            const bool in_region = x >= rq.rx0 && x < (int64_t)rq.rx0 + rq.rw && y >= rq.ry0 && y < (int64_t)rq.ry0 + rq.rh;
            if (near_crop) {
                ++inside;
                x0 = std::min(x0, x), x1 = std::max(x1, x), y0 = std::min(y0, y), y1 = std::max(y1, y);
            }
            if (near_crop != in_region) ++outside_hit;
        }
    CHECK(outside_hit == 0 && inside == rq.npix_r);
    CHECK(rq.rx0 == x0 && rq.ry0 == y0 && rq.rw == x1 - x0 + 1 && rq.rh == y1 - y0 + 1);
    CHECK(rq.film_px == (uint64_t)f.crop_w * f.crop_h);
    CHECK(rq.tile_rows % 8 == 0 && rq.tile_rows <= rq.rh && rq.rh - rq.tile_rows < 8);
    CHECK(rq.stat_rows == 2 + std::min<uint32_t>(f.max_depth, 62));
    const bool wavefront = !launch.brute && !(flags & PBRT_FILM_NO_HIT_POOL);
    CHECK(rq.brute == launch.brute && rq.wavefront == wavefront && rq.hit_rows == (wavefront ? rq.stat_rows - 2 : 0));
    CHECK(rq.rows_per_region() == (wavefront ? launch.rows_streams : launch.rows_fused));
    CHECK(rq.out_floats == ((flags & PBRT_FILM_RAW_ACCUM) ? 4u : 3u));
    CHECK(rq.tile_keep == (launch.keep && inside % 64 == 0 && !(flags & PBRT_FILM_NO_TILE_CULL)));
    const FilmKey a = render_film_key(rq);
    CHECK(a.rx0 == rq.rx0 && a.ry0 == rq.ry0 && a.rw == rq.rw && a.tile_rows == rq.tile_rows && a.npix_r == inside && a.film_w == W && a.film_h == H);
    CHECK(a.s_first == 0);  // the pass loop's
    for (uint32_t n : {0u, 1u, a.rw - 1, a.rw, a.rw + 1, a.npix_r - 1, a.npix_r, a.npix_r + 1, 7u * a.npix_r + 3u, 0xffffffffu})
        CHECK(udiv_fast(n, a.div_npix) == n / a.npix_r && udiv_fast(n, a.div_rw) == n / a.rw);
}

// region_pixel is the inverse of region_index: every index of a region gives a pixel inside it, that pixel gives the index back, and
// every pixel is given exactly once -- bands only, bands with a row-major tail, row-major only, widths that are no multiple of 8
static void pixel_order() {
    std::vector<uint32_t> widths;
    for (uint32_t rw = 1; rw <= 17; ++rw) widths.push_back(rw);
    widths.push_back(64);
    for (uint32_t rw : widths)
        for (uint32_t rh = 1; rh <= 17; ++rh) {
            FilmKey k{};
            k.rx0 = 3, k.ry0 = 2;  // (region_pixel and region_index speak of the region's own pixels)
            k.rw = rw, k.npix_r = rw * rh, k.tile_rows = rh & ~7u;
            k.div_npix = make_fastdiv(k.npix_r), k.div_rw = make_fastdiv(rw);
            std::vector<uint32_t> given(k.npix_r, 0);
            for (uint32_t pr = 0; pr < k.npix_r; ++pr) {
                uint32_t rx = ~0u, ry = ~0u;
                region_pixel(k, pr, &rx, &ry);
                CHECK(rx < rw && ry < rh);
                if (rx >= rw || ry >= rh) continue;
                CHECK(region_index(rx, ry, rw, k.tile_rows) == pr);
                ++given[ry * rw + rx];
            }
            bool once = true;
            for (uint32_t g : given) once = once && g == 1;
            CHECK(once);
        }
}
static void regions() {
    const std::pair<uint32_t, uint32_t> films[] = {{1, 1}, {13, 7}, {16, 16}, {64, 64}, {45, 9}};
    for (auto [W, H] : films)
        for (uint32_t filter = PBRT_FILTER_BOX; filter <= PBRT_FILTER_GAUSSIAN; ++filter) {
            std::vector<pbrt_film_desc> crops = {film(0, 0, W, H, filter), film(0, 0, 1, 1, filter), film(W - 1, H - 1, 1, 1, filter),
                                                 film(0, H / 2, std::min(W, 13u), std::min(H - H / 2, 7u), filter),   // left edge
                                                 film(W - std::min(W, 13u), 0, std::min(W, 13u), std::min(H, 7u), filter),   // right, top
                                                 film(W / 3, H - std::min(H, 7u), W - W / 3, std::min(H, 7u), filter),       // bottom
                                                 film(W / 2, H / 2, 1, 1, filter), film(W / 4, H / 4, (W + 1) / 2, (H + 1) / 2, filter)};
            for (const pbrt_film_desc &f : crops) {
                region_of(W, H, f, BRUTE, 0);
                region_of(W, H, f, BRUTE, PBRT_FILM_NO_TILE_CULL | PBRT_FILM_RAW_ACCUM);
                region_of(W, H, f, BRUTE_BIG, 0);
                region_of(W, H, f, BVH, 0);
                region_of(W, H, f, BVH, PBRT_FILM_NO_HIT_POOL);
            }
        }
    for (uint32_t depth : {1u, 2u, 61u, 62u, 63u, 0xffffffffu}) {
        pbrt_film_desc f = film(0, 0, 16, 16);
        f.max_depth = depth;
        region_of(16, 16, f, BVH, 0);
    }
}

static void pass_shapes() {
    std::mt19937_64 rng(7);
    auto draw = [&](uint64_t hi) { return (uint64_t)(rng() % hi); };
    for (int it = 0; it < 20000; ++it) {
        const uint32_t region = (it & 1) ? 4096u : 512u * (1u + (uint32_t)draw(16));
        const uint64_t unit = 1 + draw(it % 3 ? 1u << 12 : 1u << 26);
        const uint32_t per_call = 1 + (uint32_t)draw(it % 5 ? 300 : 70000);
        const uint64_t pass_paths = draw(it % 7 ? 1ull << 28 : 1ull << 34);
        const bool equal = it & 2;
        const uint64_t k0 = std::max<uint64_t>(1, std::min<uint64_t>(per_call, pass_paths / unit));  // the unrounded k
        PassShape ps;
        const char *why = pass_shape(&ps, pass_paths, per_call, unit, region, equal);
        if (why) {
            CHECK(is(why, T_SHAPE) && unit * (equal ? (per_call + (per_call + k0 - 1) / k0 - 1) / ((per_call + k0 - 1) / k0) : k0) >= 0xfffffc00ull);
            continue;
        }
        const uint64_t k = ps.per_pass;
        CHECK(k >= 1 && k <= per_call && unit * k < 0xfffffc00ull);
        CHECK(ps.cap % region == 0 && ps.cap >= unit * k && ps.cap - unit * k < region && (uint64_t)ps.nseg * region == ps.cap);
        const uint64_t passes = (per_call + k - 1) / k;
        CHECK(passes * k >= per_call && (passes - 1) * k < per_call);
        if (equal)
            CHECK(k <= k0 && passes == (per_call + k0 - 1) / k0);  // as many passes as the unrounded k takes, none of them larger
        else
            CHECK(k == k0);
        // the halving: strictly smaller sizes, down to the smallest pass or a pass of one unit; a fixed size never halves
        uint64_t pp = pass_paths;
        CHECK(!pass_halve(&pp, true, ps, unit) && pp == pass_paths);
        PassShape cur = ps;
        int steps = 0;
        for (; steps < 80; ++steps) {
            const uint64_t before = pp;
            if (!pass_halve(&pp, false, cur, unit)) {
                CHECK(pp == before && (cur.per_pass <= 1 || pp <= PASS_MIN_PATHS));
                break;
            }
            CHECK(pp < before && pp >= PASS_MIN_PATHS && pp <= std::max<uint64_t>(PASS_MIN_PATHS, unit * cur.per_pass / 2));
            if (pass_shape(&cur, pp, per_call, unit, region, equal)) break;
        }
        CHECK(steps < 80);
    }
    PassShape ps;  // ends at PASS_MIN_PATHS when a unit is small: 64 Mi, 32 Mi, ..., 1 Mi
    uint64_t pp = 64u << 20;
    int n = 0;
    while (pass_shape(&ps, pp, 1u << 20, 256, 512, true) == nullptr && pass_halve(&pp, false, ps, 256)) ++n;
    CHECK(n == 6 && pp == PASS_MIN_PATHS);
    // the bound: the first unit * k that is refused, and the last that is taken
    CHECK(is(pass_shape(&ps, ~0ull, 1, 0xfffffc00ull, 512, false), T_SHAPE) && pass_shape(&ps, ~0ull, 1, 0xfffffbffull, 512, false) == nullptr);
    CHECK(ps.cap == 0xfffffc00u && ps.nseg == 0xfffffc00u / 512);
    CHECK(is(pass_shape(&ps, ~0ull, 0x3fffff, 1024, 512, true), T_SHAPE));
    // a single pass of n paths, as pbrt_integrator_sample takes it
    for (uint32_t n1 : {1u, 511u, 512u, 513u, 4095u, 4096u, 4097u}) {
        CHECK(pass_shape(&ps, n1, 1, n1, 512, false) == nullptr && ps.per_pass == 1 && ps.cap == (n1 + 511) / 512 * 512 && ps.nseg == ps.cap / 512);
    }
    // what the kernels address
    CHECK(pass_addressing(71582788, false, 15, WF_DEAD_) == nullptr && is(pass_addressing(71582789, false, 15, WF_DEAD_), T_STATE));  // 2^32 / 60
    CHECK(pass_addressing(97612893, false, 11, WF_DEAD_) == nullptr && is(pass_addressing(97612894, false, 11, WF_DEAD_), T_STATE));
    CHECK(pass_addressing(WF_DEAD_ - 4096, true, 15, WF_DEAD_) == nullptr && is(pass_addressing(WF_DEAD_, true, 15, WF_DEAD_), T_DEAD));
    CHECK(pass_addressing(0xfffff000u, false, 15, WF_DEAD_) != nullptr && pass_addressing(0x3ffff000u, true, 15, WF_DEAD_) == nullptr);
}

// the pass loop the driver always ran
static std::vector<std::pair<uint32_t, uint32_t>> passes_restated(uint32_t spp, uint32_t s_pass, bool probe) {
    std::vector<std::pair<uint32_t, uint32_t>> out;
    uint32_t s_step = s_pass, passes = 0;
    for (uint32_t s0 = 0; s0 < spp; ++passes) {
        const bool probing = probe && passes == 0;
        const uint32_t sc = probing ? PROBE_SPP : std::min(s_step, spp - s0);
        out.push_back({s0, sc});
        s0 += sc;
        if (probing) {
            const uint32_t rem = spp - s0;
            s_step = div_up(rem, div_up(rem, s_pass));
        }
    }
    return out;
}
static std::vector<std::pair<uint32_t, uint32_t>> passes_of(uint32_t spp, uint32_t s_pass, bool probe) {
    std::vector<std::pair<uint32_t, uint32_t>> out;
    for (PassSchedule p{spp, s_pass, probe}; p.next();) {
        out.push_back({p.s0, p.sc});
        CHECK(p.passes == out.size() && p.probing() == (probe && out.size() == 1));
    }
    return out;
}
static void schedules() {
    for (uint32_t spp = 1; spp <= 64; ++spp)
        for (uint32_t s_pass = 1; s_pass <= spp; ++s_pass)
            for (bool probe : {false, true}) {
                if (probe && (spp < 8 * PROBE_SPP || s_pass < PROBE_SPP)) continue;  // (fuse_plan never asks for such a probe)
                const auto got = passes_of(spp, s_pass, probe);
                CHECK(got == passes_restated(spp, s_pass, probe));
                uint32_t sum = 0, lo = ~0u, hi = 0;
                for (size_t i = 0; i < got.size(); ++i) {
                    CHECK(got[i].first == sum && got[i].second >= 1);
                    sum += got[i].second;
                    if (i == 0 && probe) {
                        CHECK(got[i].second == PROBE_SPP);
                    } else if (i + 1 < got.size() || got.size() == (probe ? 2u : 1u)) {  // (the last pass may be short)
                        lo = std::min(lo, got[i].second), hi = std::max(hi, got[i].second);
                    }
                }
                CHECK(sum == spp && (lo > hi || hi - lo <= 1) && got.back().second <= std::max(hi, got.back().second));
                if (hi) CHECK(got.back().second <= hi && hi <= s_pass);
            }
    using L = std::vector<std::pair<uint32_t, uint32_t>>;
    CHECK((passes_of(13, 2, false) == L{{0, 2}, {2, 2}, {4, 2}, {6, 2}, {8, 2}, {10, 2}, {12, 1}}));
    CHECK((passes_of(12, 2, false) == L{{0, 2}, {2, 2}, {4, 2}, {6, 2}, {8, 2}, {10, 2}}));
    CHECK((passes_of(16, 16, true) == L{{0, 2}, {2, 14}}));
    CHECK((passes_of(16, 3, true) == L{{0, 2}, {2, 3}, {5, 3}, {8, 3}, {11, 3}, {14, 2}}));
    CHECK((passes_of(16, 3, false) == L{{0, 3}, {3, 3}, {6, 3}, {9, 3}, {12, 3}, {15, 1}}));
    CHECK((passes_of(256, 100, true) == L{{0, 2}, {2, 85}, {87, 85}, {172, 84}}));
}

static FusePlan plan_of(const RenderLaunch &launch, uint32_t flags, bool hint_valid, uint32_t hint, uint32_t spp, uint32_t s_pass, bool may_probe = true) {
    pbrt_camera cam = camera(16, 16);
    pbrt_film_desc f = film(0, 0, 16, 16);
    f.flags = flags, f.spp = spp;
    RenderRequest rq;
    CHECK(render_request(&rq, &cam, &f, true, launch) == nullptr);
    return fuse_plan(rq, hint_valid, hint, s_pass, may_probe);
}
static bool same(const FusePlan &p, uint32_t plan, bool probe, uint32_t source) { return p.plan == plan && p.probe == probe && p.source == source; }
static void plans() {
    // chain_len: plan 0 one bounce per launch, pairs, all ones up to MAX_CHAIN, never past max_depth
    const uint32_t ALL = 0xffffffffu;
    for (uint32_t d = 0; d < 40; ++d) CHECK(chain_len(0, d, 64) == 1);
    CHECK(chain_len(0x15, 0, 6) == 2 && chain_len(0x15, 1, 6) == 1 && chain_len(0x15, 2, 6) == 2 && chain_len(0x15, 4, 6) == 2 && chain_len(0x15, 4, 5) == 1);
    CHECK(chain_len(ALL, 0, 6) == 6 && chain_len(ALL, 0, 32) == 6 && chain_len(ALL, 6, 32) == 6 && chain_len(ALL, 30, 32) == 2 && chain_len(ALL, 31, 32) == 1);
    CHECK(chain_len(ALL, 0, 1) == 1 && chain_len(ALL, 0, 2) == 2 && chain_len(ALL, 0, ALL) == 6 && chain_len(ALL, 28, ALL) == 5 && chain_len(ALL, 40, ALL) == 1);
    CHECK(chain_len(0x1f, 0, 6) == 6 && chain_len(0x1f, 0, 7) == 6 && chain_len(0x0f, 0, 6) == 5 && chain_len(0x0f, 5, 6) == 1);
    // plan_from_survival: the survival rows of the measurements
    const unsigned long long cbox[8] = {10000, 8700, 6699, 5560, 4726, 945, 0, 0};  // 0.87 / 0.77 / 0.83 / 0.85 / 0.20
    CHECK(plan_from_survival(cbox, 6) == 0x1f);  // (the last bounce is always taken along)
    CHECK(plan_from_survival(cbox, 7) == 0x2f && plan_from_survival(cbox, 5) == 0x0f);
    const unsigned long long open_a[8] = {10000, 3700, 1073, 354, 0, 0, 0, 0};  // 0.37 / 0.29 / 0.33: nothing but the last bounce
    const unsigned long long open_b[8] = {10000, 4900, 1421, 469, 0, 0, 0, 0};  // 0.49 / 0.29 / 0.33: pairs at depth 0
    CHECK(plan_from_survival(open_a, 4) == 0x4 && plan_from_survival(open_b, 4) == 0x5 && plan_from_survival(open_b, 6) == 0x1);
    const unsigned long long cbox16[8] = {4096, 3529, 2776, 2304, 1952, 383, 0, 0};  // the Cornell box at 16 x 16 x 16
    CHECK(plan_from_survival(cbox16, 6) == 0x1f);
    unsigned long long full[64];
    for (auto &v : full) v = 1000;
    CHECK(plan_from_survival(full, 1) == 0 && plan_from_survival(full, 2) == 1 && plan_from_survival(full, 32) == 0x7fffffffu &&
          plan_from_survival(full, ALL) == 0x7fffffffu && plan_from_survival(full, 62) == 0x7fffffffu);
    const unsigned long long none[4] = {0, 0, 0, 0};
    CHECK(plan_from_survival(none, 6) == 0);
    // the plan of a call and where it came from
    CHECK(same(plan_of(BVH, 0, false, 0, 64, 64), 0, false, PBRT_PLAN_STREAMS));
    CHECK(same(plan_of(BVH, PBRT_FILM_FUSE_PLAN(0x3), true, 0x1f, 64, 64), 0, false, PBRT_PLAN_STREAMS));
    CHECK(same(plan_of(BRUTE, PBRT_FILM_FUSE_PLAN(0x3), true, 0x1f, 64, 64), 0x3, false, PBRT_PLAN_CALLER));
    CHECK(same(plan_of(BRUTE, PBRT_FILM_FUSE_PLAN(0), false, 0, 64, 64), 0, false, PBRT_PLAN_CALLER));
    CHECK(same(plan_of(BRUTE, 0, true, 0x1f, 64, 64), 0x1f, false, PBRT_PLAN_LEARNT));
    CHECK(same(plan_of(BRUTE, 0, false, 0x1f, 16, 16), PBRT_DEFAULT_FUSE_PLAN, true, PBRT_PLAN_PROBED));
    CHECK(same(plan_of(BRUTE, 0, false, 0x1f, 16, 2), PBRT_DEFAULT_FUSE_PLAN, true, PBRT_PLAN_PROBED));
    CHECK(same(plan_of(BRUTE, 0, false, 0x1f, 15, 15), PBRT_DEFAULT_FUSE_PLAN, false, PBRT_PLAN_DEFAULT));  // too few samples
    CHECK(same(plan_of(BRUTE, 0, false, 0x1f, 64, 1), PBRT_DEFAULT_FUSE_PLAN, false, PBRT_PLAN_DEFAULT));   // passes of one sample
    CHECK(same(plan_of(BRUTE, 0, false, 0x1f, 64, 64, false), PBRT_DEFAULT_FUSE_PLAN, false, PBRT_PLAN_DEFAULT));
    CHECK(same(plan_of(BRUTE, 0, true, 0x5, 64, 64, false), 0x5, false, PBRT_PLAN_LEARNT));
    // the diagnostic build's fused BVH bounce: no plan to learn
    CHECK(same(plan_of(BVH, PBRT_FILM_NO_HIT_POOL, true, 0x1f, 64, 64), 0, false, PBRT_PLAN_DEFAULT));
    CHECK(same(plan_of(BVH, PBRT_FILM_NO_HIT_POOL | PBRT_FILM_FUSE_PLAN(1), false, 0, 64, 64), 0, false, PBRT_PLAN_CALLER));
    CHECK(PBRT_DEFAULT_FUSE_PLAN == 0x15u && PROBE_SPP == 2);
}

static void default_pass_sizes() {
    const uint64_t GB = 1000000000ull, Mi = 1u << 20;
    // 512 Mi paths of 340 B each, twice over as the rule counts them, fit two thirds of 288 GB free -- on a device of which that is half
    CHECK(stream_default_pass_paths(288 * GB, 576 * GB, 0, 0, 0, 340) == 512 * Mi);
    CHECK(stream_default_pass_paths(288 * GB, 288 * GB, 0, 0, 0, 340) == 256 * Mi);  // never above half of the device
    CHECK(stream_default_pass_paths(0, 288 * GB, 0, 0, 0, 340) == PASS_MIN_PATHS);   // (the query failed: nothing counts as free)
    CHECK(stream_default_pass_paths(10 * GB, 288 * GB, 183 * GB, 0, 183 * GB, 340) == 256 * Mi);  // what is held is re-used
    uint64_t last = 0;
    for (uint64_t free_gb = 0; free_gb <= 400; ++free_gb)
        for (uint64_t limit_gb : {0ull, 1ull, 8ull, 64ull, 300ull}) {
            const uint64_t held = (free_gb % 3) * GB, other = (free_gb % 5) * GB / 2, total = 288 * GB;
            const uint64_t p = stream_default_pass_paths(free_gb * GB, total, held, limit_gb * GB, held + other, 340);
            CHECK(p >= PASS_MIN_PATHS && p <= 512 * Mi && (p & (p - 1)) == 0);
            if (p > PASS_MIN_PATHS) {
                CHECK((double)p * 340 <= (2.0 / 3.0) * (double)(free_gb * GB + held) && (double)p * 340 <= 0.5 * (double)total);
                if (limit_gb) CHECK((double)p * 340 + (double)other + 64e6 <= (double)(limit_gb * GB));
            }
            if (limit_gb == 0 && held == 0) {
                CHECK(p >= last);  // monotone in what is free (held the same)
                last = p;
            }
        }
    for (uint64_t limit_gb = 1; limit_gb < 40; ++limit_gb)  // monotone in the limit
        CHECK(stream_default_pass_paths(288 * GB, 288 * GB, 0, limit_gb * GB, 0, 340) <= stream_default_pass_paths(288 * GB, 288 * GB, 0, (limit_gb + 1) * GB, 0, 340));
    // the fused kernels: 64 Mi paths of 136 B want 9.1 GB
    CHECK(fused_default_pass_paths(64 * Mi, 136, 0) == 64 * Mi && fused_default_pass_paths(64 * Mi, 136, 16 * GB) == 64 * Mi);
    CHECK(fused_default_pass_paths(64 * Mi, 136, 8 * GB) == 32 * Mi && fused_default_pass_paths(64 * Mi, 136, 1 * GB) == 4 * Mi);
    CHECK(fused_default_pass_paths(64 * Mi, 136, 1) == PASS_MIN_PATHS && fused_default_pass_paths(16 * Mi, 120, 2 * GB) == 8 * Mi);
}

static void grids() {
    // k_trace's workgroups: never more than regions, at least regions / KMAX, else mult per CU
    CHECK(wf_trace_grid(1, 8, 256, KMAX) == 1 && wf_trace_grid(KMAX, 8, 256, KMAX) == KMAX && wf_trace_grid(KMAX + 1, 8, 256, KMAX) == KMAX + 1);
    CHECK(wf_trace_grid(2048, 8, 256, KMAX) == 2048 && wf_trace_grid(2049, 8, 256, KMAX) == 2048 && wf_trace_grid(2048 * KMAX, 8, 256, KMAX) == 2048);
    CHECK(wf_trace_grid(2048 * KMAX + 1, 8, 256, KMAX) == 2049 && wf_trace_grid(1u << 20, 2, 256, KMAX) == 49933);
    CHECK(wf_trace_grid(100, 0, 256, KMAX) == 5 && wf_trace_grid(100, 2, 32, KMAX) == 64 && wf_trace_grid(0x3ffff, 8, 256, KMAX) == 12483);
    for (uint32_t nr : {1u, 20u, 21u, 22u, 1000u, 262143u})
        for (uint32_t mult : {1u, 2u, 8u}) {
            const uint32_t G = wf_trace_grid(nr, mult, 256, KMAX);
            CHECK(G >= 1 && G <= nr && (uint64_t)G * KMAX >= nr);
        }
    // the parts of a split pass tile [0, nreg)
    for (uint32_t nreg : {1u, 7u, 64u, 127u, 128u, 1000u, 0xfffffu, 0x3fffffffu / 4096u, 0xffffffffu})
        for (uint32_t parts = 1; parts <= 8; ++parts) {
            uint32_t at = 0, lo = ~0u, hi = 0;
            for (uint32_t h = 0; h < parts; ++h) {
                uint32_t r0, rn;
                wf_part(nreg, parts, h, &r0, &rn);
                CHECK(r0 == at);
                at += rn;
                lo = std::min(lo, rn), hi = std::max(hi, rn);
            }
            CHECK(at == nreg && hi - lo <= 1);
        }
    // k_trace's workgroup: 64 KB of LDS, two workgroups per CU while image + 1 KB + three rows fit half of it
    WfShape w = wf_shape(65536, 0, 20, true);
    CHECK(w.threads == 1024 && w.rows == 7 && w.lds == 7 * 4096 && w.packet);
    w = wf_shape(0, 0, 22, true);  // (no limit known: 64 KB) and a tree too deep for the packet walk's 64-entry stack
    CHECK(w.rows == 7 && !w.packet && wf_shape(65536, 0, 21, true).packet && !wf_shape(65536, 0, 21, false).packet);
    w = wf_shape(65536, 19456, 10, true);  // 19456 + 1024 + 12288 = 32768: still two per CU, three rows
    CHECK(w.rows == 3 && w.lds == 19456 + 3 * 4096);
    w = wf_shape(65536, 19472, 10, true);  // one workgroup per CU: (65536 - 19472 - 1024) / 4096 = 10 rows fit, 8 are used
    CHECK(w.rows == 8 && w.lds == 19472 + 8 * 4096);
    w = wf_shape(65536, 48000, 10, true);
    CHECK(w.rows == 4 && w.lds == 48000 + 4 * 4096);
    w = wf_shape(163840, 114000, 10, true);  // gfx950: 160 KB
    CHECK(w.rows == 8 && w.lds == 114000 + 8 * 4096);
    CHECK(wf_shape(163840, 60000, 10, true).rows == 5 && wf_shape(65536, 56000, 10, true).rows == 2);
}

static void byte_models() {
    uint64_t total, bounce, trace;
    unsigned long long two[64] = {100, 60}, six[64] = {4096, 3529, 2776, 2304, 1952, 383};
    // two depths, one launch per bounce: 60 survivors written and read (60 B), 40 + 60 radiance records (12 B); the film: 100
    // samples gathered (12 B), 10 pixels accumulated (32 B a pass) and resolved (28 B)
    radiance_model_bytes(two, 62, 100, 10, 1, 0, 2, nullptr, &total, &bounce);
    CHECK(bounce == 3600 + 480 + 3600 + 720 && total == 8400 + 1200 + 320 + 280);
    radiance_model_bytes(two, 62, 100, 10, 3, 0x1, 2, nullptr, &total, &bounce);  // both bounces in one launch, three passes
    CHECK(bounce == 1200 && total == 1200 + 1200 + 960 + 280);
    // six depths (the Cornell box at 16 x 16 x 16): one launch, and one per bounce
    radiance_model_bytes(six, 62, 4096, 256, 1, 0x1f, 6, nullptr, &total, &bounce);
    CHECK(bounce == 49152 && total == 113664);
    radiance_model_bytes(six, 62, 4096, 256, 1, 0, 6, nullptr, &total, &bounce);
    CHECK(bounce == 218544 + 387336 + 310464 + 259584 + 158928 + 27576 && bounce == 1362432 && total == 1426944);
    radiance_model_bytes(six, 62, 4096, 256, 6, 0x1f, 6, nullptr, &total, &bounce);
    CHECK(bounce == 49152 && total == 154624);
    // hits: rays read 24 B, the paths that hit their state
    unsigned long long hits2[64] = {80, 30};
    radiance_model_bytes(two, 62, 100, 10, 1, 0, 2, hits2, &total, &bounce);
    CHECK(bounce == 3600 + 480 + (60 * 24 + 30 * 60) + 720);
    // the streams, two depths with 50 shadow rays, and six with 2000
    CHECK(wavefront_model_bytes(two, hits2, 62, 50, &trace) == 18280 && trace == 4360);
    CHECK(wavefront_model_bytes(two, hits2, 62, 50, nullptr) == 18280);
    unsigned long long live6[64] = {1000, 900, 500, 300, 100, 10}, hits6[64] = {950, 600, 400, 200, 50, 5};
    CHECK(wavefront_model_bytes(live6, hits6, 62, 2000, &trace) == 553280 && trace == 141160);
    hits6[0] = 5000;  // (never more hits than rays)
    CHECK(wavefront_model_bytes(live6, hits6, 62, 2000, &trace) == 553280);
    // what pbrt_stats reports: statistics rows [segments, shadow rays, live per depth ..., hits per depth from HIT_ROW0]
    unsigned long long hstats[2 + 2 * MAX_DEPTH_STATS] = {0};
    hstats[1] = 2000;
    std::memcpy(hstats + 2, live6, 6 * 8);
    std::memcpy(hstats + HIT_ROW0, hits6, 6 * 8);
    pbrt_camera cam = camera(10, 10);
    pbrt_film_desc f = film(0, 0, 10, 10, PBRT_FILTER_BOX);
    RenderRequest rq;
    CHECK(render_request(&rq, &cam, &f, true, BVH) == nullptr);
    ModelBytes m = render_model_bytes(rq, hstats, 1000, 2, 0);
    CHECK(m.bounce == 553280 && m.trace == 141160 && m.total == 553280 + 12000 + 6400 + 2800);
    std::memset(hstats, 0, sizeof hstats);
    std::memcpy(hstats + 2, six, 6 * 8);
    CHECK(render_request(&rq, &cam, &f, true, BRUTE) == nullptr);
    m = render_model_bytes(rq, hstats, 4096, 1, 0x1f);
    CHECK(m.bounce == 49152 && m.trace == 0 && m.total == 49152 + 49152 + 3200 + 2800);
    CHECK(N_STATE == 15 && MAX_DEPTH_STATS == 62 && MAX_CHAIN == 6 && HIT_ROW0 == 64);
}

int main() {
    rule_table();
    regions();
    pixel_order();
    pass_shapes();
    schedules();
    plans();
    default_pass_sizes();
    grids();
    byte_models();
    std::printf("{\"checks\": %d, \"failures\": %d}\n", checks, failures);
    return failures ? 1 : 0;
}
