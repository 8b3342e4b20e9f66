// One beamform request: "beamform this channel data on these pixels by this method", as every pbrt_das_* / pbrt_bf_* / pbrt_iq_* /
// pbrt_scan_* entry point hands it to the launch (pbrt_api.hip beamform_host, beamform_dev, first_arrival_dev, das_enqueue), and
// the rules its four public parameter blocks must keep -- each written once; and the shape of the launch grid, which the kernels
// read as well.  Plain host code when a host compiler reads it (no HIP), so that tests/native/bf_request_check.cpp can build it on its own.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/pbrt_hip.h"

#define DAS_TILE 8u
#define DAS_XCDS 8u
#define DAS_BANDS (2u * DAS_XCDS)

struct BfRequest {
    const pbrt_das_params *das;
    uint32_t method;  // one numbering everywhere: PBRT_SCAN_DAS (0), PBRT_BF_PDAS, PBRT_BF_FDMAS, PBRT_SCAN_IQ
    float pw;         // the launch argument of the method: p (p-DAS, F-DMAS does not read it), the demodulation frequency (I/Q), else 0
    bool probe;       // the elements are a table [n_elements][4] of pbrt_us_array_elements, not positions [n_elements]
    bool tab;         // the pixels are two tables [nx][nz] (pbrt_scan_*), not the axes x[nx], z[nz]
    // the receive window (pbrt_apod_*, DESIGN D22): PBRT_APOD_*, and what the kernel reads of it, w = a0 + (1 - a0) cos(pi t(u; alpha)).
    // PBRT_APOD_BOXCAR (every other block): a0 = 1, alpha = 1, which no kernel reads
    uint32_t window;
    float a0, alpha;
};

// tiles of DAS_TILE pixels along an axis of n
static inline uint32_t das_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + DAS_TILE - 1u) / DAS_TILE); }

// ---- the launch grid of the beamformers: one text for das_enqueue and for the kernels (tests/native/bf_request_check.cpp walks it) ----
// (BF_HD: what the kernels call too; das_grid is the host's alone -- no kernel sizes a grid)
#ifdef __HIPCC__
#define BF_HD __host__ __device__ __forceinline__
#else
#define BF_HD static inline
#endif
// Which tile does workgroup b take?  Workgroup b runs on XCD b % 8, and every XCD has its own 4 MB L2: the z-tiles are cut into 16
// bands and XCD k takes the bands k and 15 - k -- an XCD then reads one eighth of the samples (a pixel at depth z reads around
// sample 2 z fs / c), and, the receive cone widening linearly with depth, a shallow band and its deep mirror together always hold
// the same number of pixels that see an element: the same work on every XCD.  (Measured neutral at the sizes of USMain.py, 151
// against 148 us: the 4.2 MB that are read at all stay cached either way; kept for larger acquisitions.)
// -> (tx, tz), or false for a slot beyond the XCD's share.  m = z-tiles of the largest share.
// tab: the scan is a pair of pixel tables px[nx][nz], pz[nx][nz] (the pbrt_scan_* entry points, DESIGN D21) instead of the axes
// x[nx], z[nz] -- the strides (1, 0) / (0, 1) of the axes against (nz, 1) of the tables differ in this one bit: pixel (ix, iz) reads
// entry tab ? ix * nz + iz : ix of gx and tab ? ix * nz + iz : iz of gz, once per lane, and everything after that is per pixel already.
struct DasGrid {
    uint32_t ntx, ntz, m, tab;
};
BF_HD uint32_t das_band_lo(uint32_t band, uint32_t ntz) { return (band * ntz + DAS_BANDS - 1u) / DAS_BANDS; }
BF_HD bool das_tile_of(const DasGrid g, uint32_t b, uint32_t *tx, uint32_t *tz) {
    const uint32_t xcd = b % DAS_XCDS, i = b / DAS_XCDS;
    const uint32_t lo1 = das_band_lo(xcd, g.ntz), n1 = das_band_lo(xcd + 1u, g.ntz) - lo1;
    const uint32_t lo2 = das_band_lo(DAS_BANDS - 1u - xcd, g.ntz), n2 = das_band_lo(DAS_BANDS - xcd, g.ntz) - lo2;
    const uint32_t t = i / g.m, r = i - t * g.m;
    *tx = t;
    *tz = r < n1 ? lo1 + r : lo2 + (r - n1);
    return t < g.ntx && r < n1 + n2;
}
// the grid of a scan of nx x nz pixels -> the number of workgroups: every XCD gets as many slots per tile column as the largest
// share (bands k and 15 - k) has z-tiles
static inline uint32_t das_grid(DasGrid *g, uint32_t nx, uint32_t nz, bool tab) {
    *g = DasGrid{das_tiles(nx), das_tiles(nz), 0u, tab ? 1u : 0u};
    for (uint32_t k = 0; k < DAS_XCDS; ++k) {
        const uint32_t share = (das_band_lo(k + 1u, g->ntz) - das_band_lo(k, g->ntz)) +
                               (das_band_lo(DAS_BANDS - k, g->ntz) - das_band_lo(DAS_BANDS - 1u - k, g->ntz));
        g->m = share > g->m ? share : g->m;
    }
    return DAS_XCDS * g->ntx * (g->m ? g->m : 1u);
}
#undef BF_HD

// a rule of the makers below: its own text is the refusal
#define BF_RULE(cond)              \
    do {                           \
        if (!(cond)) return #cond; \
    } while (0)

// -> nullptr and *rq filled, or the text of the first rule that failed.  `p` is read by PBRT_BF_PDAS only, `demod_freq` by PBRT_SCAN_IQ only.
static inline const char *bf_request(BfRequest *rq, const pbrt_das_params *das, uint32_t method, float p, float demod_freq, uint32_t probe,
                                     bool tab) {
    BF_RULE(das != nullptr);
    BF_RULE(method == PBRT_SCAN_DAS || method == PBRT_BF_PDAS || method == PBRT_BF_FDMAS || method == PBRT_SCAN_IQ);
    BF_RULE(probe <= 1u);
    BF_RULE(method != PBRT_BF_PDAS || (std::isfinite(p) && p >= 1.0f && p <= 8.0f));
    BF_RULE(method != PBRT_SCAN_IQ || (std::isfinite(demod_freq) && demod_freq >= 0.0f));
    BF_RULE(das->n_angles > 0 && das->n_elements > 0 && das->time_samples > 1 && das->fs > 0.0f && das->sound_speed > 0.0f);
    BF_RULE(das->interpolation <= PBRT_DAS_LINEAR && das->f_number >= 0.0f);
    BF_RULE(das->nx > 0 && das->nz > 0 && (uint64_t)das->nx * das->nz < 0xffffffffull);
    // (the launch grid, das_grid above: every XCD gets the z-tiles of the largest share, at most all of them and one per band)
    BF_RULE((uint64_t)das_tiles(das->nx) * (das_tiles(das->nz) + DAS_BANDS) * DAS_XCDS < 0x7fffffffull);
    *rq = BfRequest{das, method, method == PBRT_SCAN_IQ ? demod_freq : method == PBRT_SCAN_DAS ? 0.0f : p, probe != 0u, tab,
                    PBRT_APOD_BOXCAR, 1.0f, 1.0f};
    return nullptr;
}

// the five public blocks: the methods each admits, then the rules above (the first four make a boxcar request)
static inline const char *bf_request(BfRequest *rq, const pbrt_das_params *p, bool probe) {  // pbrt_das_*[_probe]
    return bf_request(rq, p, PBRT_SCAN_DAS, 0.0f, 0.0f, probe ? 1u : 0u, false);
}
static inline const char *bf_request(BfRequest *rq, const pbrt_bf_params *p) {  // (plain delay-and-sum has its own calls)
    BF_RULE(p != nullptr);
    BF_RULE(p->method == PBRT_BF_PDAS || p->method == PBRT_BF_FDMAS);
    return bf_request(rq, &p->das, p->method, p->p, 0.0f, p->probe, false);
}
static inline const char *bf_request(BfRequest *rq, const pbrt_iq_params *p) {
    BF_RULE(p != nullptr);
    return bf_request(rq, &p->das, PBRT_SCAN_IQ, 0.0f, p->demod_freq, p->probe, false);
}
static inline const char *bf_request(BfRequest *rq, const pbrt_scan_params *p) {
    BF_RULE(p != nullptr);
    return bf_request(rq, &p->das, p->method, p->p, p->demod_freq, p->probe, true);
}
// the block with a receive window: the window's own rules, then every rule of its pbrt_scan_params
static inline const char *bf_request(BfRequest *rq, const pbrt_apod_params *p) {
    BF_RULE(p != nullptr);
    BF_RULE(p->tables <= 1u);
    BF_RULE(p->window == PBRT_APOD_BOXCAR || p->window == PBRT_APOD_TUKEY || p->window == PBRT_APOD_HANN || p->window == PBRT_APOD_HAMMING);
    BF_RULE(p->window != PBRT_APOD_TUKEY || (std::isfinite(p->alpha) && p->alpha > 0.0f && p->alpha <= 1.0f));
    BF_RULE(p->window == PBRT_APOD_BOXCAR || p->scan.das.f_number > 0.0f);  // (no aperture, nothing to be a window of)
    if (const char *why = bf_request(rq, &p->scan.das, p->scan.method, p->scan.p, p->scan.demod_freq, p->scan.probe, p->tables != 0u)) return why;
    rq->window = p->window;
    rq->a0 = p->window == PBRT_APOD_BOXCAR ? 1.0f : p->window == PBRT_APOD_HAMMING ? 0.54f : 0.5f;
    rq->alpha = p->window == PBRT_APOD_TUKEY ? p->alpha : 1.0f;
    return nullptr;
}
