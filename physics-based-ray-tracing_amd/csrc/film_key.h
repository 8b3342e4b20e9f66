// The film key: which pixel and which sample the path at a home slot is.  One member of every argument block of the radiance kernels
// that turns a home slot or a region index into a pixel (RadArgs, WfArgs, PathArgs, FilmArgs, TileKeepArgs), with the pixel order of
// the rendered region and its inverse beside it.  Plain C++ (no HIP), so that tests/native/render_request_check.cpp can build it on
// its own; under hipcc the functions are device functions too.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define FILM_KEY_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define FILM_KEY_FN inline
#endif

// Exact unsigned division by a launch-uniform divisor (Granlund-Montgomery round-up multiplier, the
// branch-free 33-bit form):  n / d == (((n - hi) >> 1) + hi) >> shift  with hi = mulhi(n, magic), for every
// 32-bit n and d >= 2; d == 1 is flagged.  5 VALU instead of the ~20 of a division by a runtime value.
struct FastDiv {
    uint32_t magic, shift, is_one, pad;
};
inline FastDiv make_fastdiv(uint32_t d) {  // host
    FastDiv f = {0, 0, 0, 0};
    if (d <= 1) {
        f.is_one = 1;
        return f;
    }
    uint32_t L = 31;
    while (!(d >> L)) --L;  // floor(log2 d)
    if ((d & (d - 1)) == 0) {
        f.shift = L - 1;  // magic 0: ((n - 0) >> 1) >> (L - 1)
        return f;
    }
    const uint64_t num = 1ull << (32 + L);
    uint64_t m = num / d;
    const uint64_t rem = num % d;
    m += m;
    if (2 * rem >= d) m += 1;
    f.magic = (uint32_t)(m + 1);
    f.shift = L;
    return f;
}
FILM_KEY_FN uint32_t udiv_fast(uint32_t n, FastDiv f) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t hi = __umulhi(n, f.magic);
#else
    const uint32_t hi = (uint32_t)(((uint64_t)n * f.magic) >> 32);
#endif
    const uint32_t q = (((n - hi) >> 1) + hi) >> f.shift;
    return f.is_one ? n : q;
}

// The ONE place that says what the members mean and who fills them.  A render (key mode 0) cuts a pass into homes: home = sl *
// npix_r + pr is sample s_first + sl of the pixel with region index pr (region_index below).
//   rx0, ry0, rw        the rendered region on the film: the crop and the margin its filter reads, clipped to the film (its height
//                       is FilmArgs::rh: only the film gather asks)
//   npix_r              pixels of the region, rw * rh: homes per sample, and the stride of a sample's block of radiance records
//   tile_rows           rows of the region in 8-row bands, rh & ~7 (region_index)
//   film_w, film_h      the camera's film: the RNG key of a pixel is py * film_w + px, and a film position is a pixel over these
//   div_npix, div_rw    home / npix_r and (index or index / 8) / rw without a division by a runtime value
//   s_first             the first sample index of the pass
// Filled on the host: all but s_first by render_film_key (render_request.h) once per render, s_first by the pass loop.
// Integrator.sample on caller rays (key mode 1) reads none of it and carries the stand-ins of sample_key (pbrt_api.hip).
struct FilmKey {
    uint32_t rx0, ry0, rw, npix_r, s_first, film_w, film_h, tile_rows;
    FastDiv div_npix, div_rw;
};
static_assert(sizeof(FilmKey) == 64 && alignof(FilmKey) == 4 && offsetof(FilmKey, tile_rows) == 28 && offsetof(FilmKey, div_npix) == 32 &&
                  offsetof(FilmKey, div_rw) == 48,
              "the film key keeps the bytes of the ten members it replaced");

// Pixel order inside the rendered region (index k of a pixel = its slot within one sample's block of `Lhome` and
// of the first-bounce state).  The region is cut into bands of 8 rows and a band is walked column by column, so
// the 64 consecutive paths of a wave are an 8 x 8 pixel tile, not a 64 x 1 strip -- on a BVH their primary rays
// visit fewer distinct nodes (every lane of a wave pays for the union; path_key).  The rh % 8 rows below the last
// full band keep the row-major order; tile_rows = rh & ~7 (0: plain row-major everywhere).
FILM_KEY_FN uint32_t region_index(uint32_t xx, uint32_t yy, uint32_t rw, uint32_t tile_rows) {
    return yy < tile_rows ? (yy >> 3) * (8u * rw) + (xx << 3) + (yy & 7u) : yy * rw + xx;
}
// ... and its inverse: the pixel (rx, ry) of the region whose index is pr (one division either way)
FILM_KEY_FN void region_pixel(const FilmKey &k, uint32_t pr, uint32_t *rx, uint32_t *ry) {
    const bool tiled = pr < k.tile_rows * k.rw;
    const uint32_t num = tiled ? pr >> 3 : pr;
    const uint32_t q = udiv_fast(num, k.div_rw);
    *rx = num - q * k.rw;
    *ry = tiled ? (q << 3) + (pr & 7u) : q;
}
