// One Capon request (include/pbrt_hip.h "Capon", DESIGN D23): the I/Q beamform request of its pbrt_scan_params, made by bf_request, then
// the rules of the method itself -- each written once -- and the subarray rule that the host and k_capon_beamform share.  Plain host
// code (no HIP), so that tests/native/capon_request_check.cpp can build it on its own.
#pragma once
#include "bf_request.h"

#define CAPON_MAX_L 32u   // the longest subarray: R is at most 32 x 32 in LDS
#define CAPON_MAX_E 256u  // the most elements: a wave's row of delayed samples in LDS

#ifdef __HIPCC__
#define CAPON_HD __host__ __device__
#else
#define CAPON_HD
#endif

// the subarray length L and the number of subarrays M of an aperture of N elements (N = 0: L = 1, M = 0)
struct CaponLM {
    uint32_t L, M;
};
CAPON_HD static inline CaponLM capon_lm(uint32_t N, float l_prop) {
    const float want = floorf(l_prop * (float)N);  // l_prop in [0, 0.5], N <= CAPON_MAX_E: in [0, 128]
    uint32_t L = (uint32_t)want;
    L = L < 1u ? 1u : L;
    L = L > CAPON_MAX_L ? CAPON_MAX_L : L;
    return CaponLM{L, N ? N - L + 1u : 0u};
}

struct CaponRequest {
    BfRequest bf;  // the I/Q request: das, PBRT_SCAN_IQ, pw = the demodulation frequency, probe, tab; a boxcar window
    float l_prop, delta_l;
};

// -> nullptr and *rq filled, or the text of the first rule that failed
static inline const char *capon_request(CaponRequest *rq, const pbrt_capon_params *p) {
    BF_RULE(p != nullptr);
    BF_RULE(p->scan.method == PBRT_SCAN_IQ);
    BF_RULE(p->tables <= 1u);
    BF_RULE(std::isfinite(p->l_prop) && p->l_prop >= 0.0f && p->l_prop <= 0.5f);
    BF_RULE(std::isfinite(p->delta_l) && p->delta_l > 0.0f && p->delta_l <= 1e3f);
    BF_RULE(p->scan.das.n_elements <= CAPON_MAX_E);
    if (const char *why = bf_request(&rq->bf, &p->scan.das, p->scan.method, p->scan.p, p->scan.demod_freq, p->scan.probe, p->tables != 0u)) return why;
    rq->l_prop = p->l_prop;
    rq->delta_l = p->delta_l;
    return nullptr;
}
