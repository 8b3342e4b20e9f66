// The two Doppler steps (include/pbrt_hip.h "colour and power Doppler", DESIGN D24) -- the slow-time autocorrelation of an ensemble of
// I/Q frames and the maps made of it -- as their host-pointer and _dev entry points hand them to the launch (pbrt_api.hip
// doppler_*_enqueue).  Per step one maker, as in img_request.h: every rule of the step, null pointers included, written once and in the
// order the entry points refuse by; `empty`, a call without a pixel; the launch shape next to the limit that guards it; and the
// smoothing weights, which the host makes and the kernel takes by value.  -> nullptr and *rq filled, or the text of the first rule that
// failed.  Plain host code (no HIP): tests/native/doppler_request_check.cpp builds it on its own.
#pragma once
#include "img_request.h"

#define DOPPLER_MAX_FRAMES 64u  // k_doppler_autocorr: the ensemble length, a run-time loop count
#define DOPPLER_MAX_DEGREE 3u   // k_doppler_autocorr: an instance per number of coefficients, 0 (no filter) .. 4
#define DOPPLER_MAX_K 15u       // k_doppler_maps: the longest smoothing window per axis
#define DOPPLER_TILE_X 8u       // k_doppler_maps: a workgroup's tile of output pixels, 8 rows (x) of 32 (z, the fastest axis)
#define DOPPLER_TILE_Z 32u

struct DopplerWeights { float wx[DOPPLER_MAX_K], wz[DOPPLER_MAX_K]; };  // the windows of a request, [kx] and [kz] used, the rest 0

// a k-point window in f64, normalised to sum 1, rounded once to f32 (k odd, 1 .. DOPPLER_MAX_K)
static inline void doppler_window(uint32_t window, uint32_t k, float *w) {
    double h[DOPPLER_MAX_K], sum = 0.0;
    for (uint32_t i = 0; i < k; ++i) {
        h[i] = window == PBRT_DOPPLER_HAMMING && k > 1u ? 0.54 - 0.46 * std::cos(2.0 * 3.14159265358979323846 * (double)i / (double)(k - 1u)) : 1.0;
        sum += h[i];
    }
    for (uint32_t i = 0; i < DOPPLER_MAX_K; ++i) w[i] = i < k ? (float)(h[i] / sum) : 0.0f;
}

struct DopplerAcfRequest {
    bool empty;
    uint32_t N, P, n_coef;  // frames, pixels of a frame, coefficients of the wall filter (0: none)
    ImgLaunch launch;       // k_doppler_autocorr: one thread per pixel
};
static inline const char *doppler_acf_request(DopplerAcfRequest *rq, const pbrt_doppler_params *p, const void *frames, const void *q,
                                              const void *acf) {
    IMG_RULE(p != nullptr);
    IMG_RULE(frames && acf);
    IMG_RULE(p->n_frames >= 2u && p->n_frames <= DOPPLER_MAX_FRAMES);
    const bool wall = p->wall_degree != PBRT_DOPPLER_WALL_NONE;
    IMG_RULE(!wall || p->wall_degree <= DOPPLER_MAX_DEGREE);
    IMG_RULE(!wall || p->wall_degree + 1u < p->n_frames);
    IMG_RULE(!wall || q);
    const uint64_t P = (uint64_t)p->nx * p->nz;  // (one thread per pixel: 2^24 workgroups at the most)
    IMG_RULE(P < 0xffffffffull && P * p->n_frames < 0xffffffffull);
    const uint32_t n_coef = wall ? p->wall_degree + 1u : 0u;
    IMG_RULE(!img_overlap(frames, (size_t)P * p->n_frames * 8, acf, (size_t)P * 12));
    IMG_RULE(!wall || !img_overlap(q, (size_t)n_coef * p->n_frames * 4, acf, (size_t)P * 12));
    *rq = DopplerAcfRequest{P == 0, p->n_frames, (uint32_t)P, n_coef, ImgLaunch{img_div_up(P, 256), 1u, 256u, 0}};
    return nullptr;
}

struct DopplerMapsRequest {
    bool empty;
    uint32_t nx, nz, kx, kz, tiles_z;  // tiles_z: tiles along z; the tiles of a row of tiles are neighbours in the grid
    float scale;                       // nyquist_velocity / pi
    DopplerWeights w;
    ImgLaunch launch;  // k_doppler_maps: a workgroup per tile; LDS: three planes of the tile with its halo, three of its z-smoothed rows, the weights
};
static inline size_t doppler_maps_lds(uint32_t kx, uint32_t kz) {
    const size_t rows = DOPPLER_TILE_X + (kx - 1u), cols = DOPPLER_TILE_Z + (kz - 1u);
    return (3u * rows * cols + 3u * rows * DOPPLER_TILE_Z + 2u * (DOPPLER_MAX_K + 1u)) * 4;  // 20.7 KB at 15 x 15
}
static inline const char *doppler_maps_request(DopplerMapsRequest *rq, const pbrt_doppler_params *p, const void *acf, const void *velocity,
                                               const void *amplitude) {
    IMG_RULE(p != nullptr);
    IMG_RULE(acf && velocity && amplitude);
    IMG_RULE((p->kx & 1u) == 1u && p->kx <= DOPPLER_MAX_K && (p->kz & 1u) == 1u && p->kz <= DOPPLER_MAX_K);
    IMG_RULE(p->window == PBRT_DOPPLER_BOXCAR || p->window == PBRT_DOPPLER_HAMMING);
    IMG_RULE(std::isfinite(p->nyquist_velocity) && p->nyquist_velocity > 0.0f);
    const uint64_t P = (uint64_t)p->nx * p->nz;
    const uint32_t tiles_x = img_div_up(p->nx, DOPPLER_TILE_X), tiles_z = img_div_up(p->nz, DOPPLER_TILE_Z);
    IMG_RULE(P < 0xffffffffull && (uint64_t)tiles_x * tiles_z < 0x7fffffffull);  // (the grid below)
    IMG_RULE(!img_overlap(acf, (size_t)P * 12, velocity, (size_t)P * 4) && !img_overlap(acf, (size_t)P * 12, amplitude, (size_t)P * 4) &&
             !img_overlap(velocity, (size_t)P * 4, amplitude, (size_t)P * 4));
    *rq = DopplerMapsRequest{P == 0, p->nx, p->nz, p->kx, p->kz, tiles_z, (float)((double)p->nyquist_velocity / 3.14159265358979323846),
                             DopplerWeights{}, ImgLaunch{tiles_x * tiles_z, 1u, 256u, doppler_maps_lds(p->kx, p->kz)}};
    doppler_window(p->window, p->kx, rq->w.wx);
    doppler_window(p->window, p->kz, rq->w.wz);
    return nullptr;
}
