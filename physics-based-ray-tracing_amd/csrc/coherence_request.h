// One spatial-coherence request (include/pbrt_hip.h "spatial coherence", DESIGN D26): the I/Q beamform request of its
// pbrt_scan_params, made by bf_request, then the rules of the two kinds -- each written once -- and the lag rule that the host and
// k_coherence_beamform share.  Plain host code (no HIP), so that tests/native/coherence_request_check.cpp can build it on its own.
#pragma once
#include "bf_request.h"

#define COH_MAX_E 256u   // the most elements: a wave's planes of delayed samples in LDS
#define COH_MAX_H 4u     // the largest half kernel: 2 H + 1 = 9 samples per element
#define COH_MAX_LAG 64u  // the most lags summed

#ifdef __HIPCC__
#define COH_HD __host__ __device__
#else
#define COH_HD
#endif

// the number of lags M summed for an aperture of N elements: min(max(1, floor(lag_prop N)), N - 1, 64), 0 for N < 2
COH_HD static inline uint32_t coherence_lags(uint32_t N, float lag_prop) {
    if (N < 2u) return 0u;
    const float want = floorf(lag_prop * (float)N);  // lag_prop in (0, 1], N <= COH_MAX_E: in [0, 256]
    uint32_t M = (uint32_t)want;
    M = M < 1u ? 1u : M;
    M = M > N - 1u ? N - 1u : M;
    return M > COH_MAX_LAG ? COH_MAX_LAG : M;
}

struct CoherenceRequest {
    BfRequest bf;  // the I/Q request: das, PBRT_SCAN_IQ, pw = the demodulation frequency, probe, tab; a boxcar window
    uint32_t kind, half_kernel;
    float lag_prop, gamma;
    uint32_t width;      // floats per pixel of the image: 1 (SLSC) or 2 (CF)
    uint32_t lds_bytes;  // dynamic LDS of a workgroup: 4 waves x min(E, 256) x (2 H + 1) pairs
};

// -> nullptr and *rq filled, or the text of the first rule that failed
static inline const char *coherence_request(CoherenceRequest *rq, const pbrt_coherence_params *p) {
    BF_RULE(p != nullptr);
    BF_RULE(p->scan.method == PBRT_SCAN_IQ);
    BF_RULE(p->tables <= 1u);
    BF_RULE(p->kind == PBRT_COH_SLSC || p->kind == PBRT_COH_CF);
    BF_RULE(p->scan.das.n_elements <= COH_MAX_E);
    BF_RULE(p->kind != PBRT_COH_SLSC || (std::isfinite(p->lag_prop) && p->lag_prop > 0.0f && p->lag_prop <= 1.0f));
    BF_RULE(p->kind != PBRT_COH_SLSC || p->half_kernel <= COH_MAX_H);
    BF_RULE(p->kind != PBRT_COH_CF || (std::isfinite(p->gamma) && p->gamma >= 0.0f && p->gamma <= 4.0f));
    BF_RULE(p->kind != PBRT_COH_CF || p->half_kernel == 0u);
    if (const char *why = bf_request(&rq->bf, &p->scan.das, p->scan.method, p->scan.p, p->scan.demod_freq, p->scan.probe, p->tables != 0u)) return why;
    rq->kind = p->kind;
    rq->half_kernel = p->half_kernel;
    rq->lag_prop = p->lag_prop;
    rq->gamma = p->gamma;
    rq->width = p->kind == PBRT_COH_CF ? 2u : 1u;
    rq->lds_bytes = 4u * p->scan.das.n_elements * (2u * p->half_kernel + 1u) * 8u;
    return nullptr;
}
