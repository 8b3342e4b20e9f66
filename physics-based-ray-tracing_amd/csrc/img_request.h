// The seven image steps around the beamformer -- pulse, envelope, log compression, axial FIR, rf2iq, I/Q envelope, scan conversion --
// as their host-pointer and _dev entry points hand them to the launch (pbrt_api.hip *_enqueue).  Per step one maker: every rule of the
// step, null pointers included, written once and in the order the entry points refuse by; `empty`, a call without an output element;
// the launch shape (grid, block, dynamic LDS bytes) next to the limit that guards it.  -> nullptr and *rq filled, or the text of the
// first rule that failed.  Plain host code (no HIP): tests/native/img_request_check.cpp builds it on its own.  What needs the device
// stays with the driver: the tap-table cache, the LDS attribute, the timers and the launches.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/pbrt_hip.h"

#define FIR_MAX_K 1024       // k_axial_fir, k_rf2iq: taps h[2K + 1]
#define RF2IQ_MAX_D 8        // k_rf2iq: 40 KB of LDS at D = 8, K = 1024
#define ENV_MAX_N 4096       // k_hilbert_env: a workgroup holds a column and its tap table in LDS
#define ENV_MAX_BLOCKS 256u  // k_env_max: the words every block of k_log_compress folds
#define PULSE_MAX_K 1024     // k_apply_pulse
constexpr uint32_t env_even_len(uint32_t Mp) { return 2u * Mp + 16u; }  // entries of one compact table of k_hilbert_env_even (kernels too)

struct ImgLaunch { uint32_t gx, gy, block; size_t lds; };  // grid (gx, gy), threads per workgroup, dynamic LDS bytes
enum ImgForm { IMG_FORM_HOST, IMG_FORM_DEV };
static inline uint32_t img_div_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }
static inline bool img_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + nb && pb < pa + na;
}
static inline size_t img_fir_lds(uint32_t K) { return (size_t)(2 * K + 1 + 256 + 2 * K) * 4; }  // fir_256: taps [2K + 1], 256 + 2K staged samples
#define IMG_RULE(cond) do { if (!(cond)) return #cond; } while (0)  // a rule of the makers below: its own text is the refusal

struct PulseRequest {
    bool empty;
    uint32_t n_traces, T, K;  // K: half-width of the pulse in samples
    float fs, frequency, sigma;
    ImgLaunch launch;  // k_apply_pulse: one workgroup per 256 samples of a trace
};
static inline const char *pulse_request(PulseRequest *rq, uint32_t n_traces, uint32_t T, float fs, float frequency, float sigma, const void *in,
                                        const void *out) {
    IMG_RULE(in && out && !img_overlap(in, (size_t)n_traces * T * 4, out, (size_t)n_traces * T * 4));
    IMG_RULE(fs > 0.0f && frequency > 0.0f && sigma > 0.0f);
    IMG_RULE((uint64_t)n_traces * T < 0xffffffffull && n_traces <= 65535u);  // (n_traces is the grid's second dimension)
    const double K = std::ceil(2.5 * (double)sigma * (double)fs);  // (held to the limit before it is narrowed: no width wraps into it)
    IMG_RULE(K <= PULSE_MAX_K);
    *rq = PulseRequest{n_traces == 0 || T == 0, n_traces, T, (uint32_t)K, fs, frequency, sigma,
                       ImgLaunch{img_div_up(T, 256), n_traces, 256u, img_fir_lds((uint32_t)K)}};
    return nullptr;
}

struct EnvRequest {
    bool empty;
    uint32_t nx, nz, np, G, mp;  // np: the column rounded up to 4; G: entries of its tap table; mp: half the column rounded up to 4
    bool even;  // k_hilbert_env_even: half of the taps of an even column length are zero, it leaves their multiply-adds out
    ImgLaunch launch;       // one workgroup per column; a thread carries four outputs: whole waves for the quads of a column
    ImgLaunch taps_launch;  // k_hilbert_taps: one thread per entry of the tap table and of the four compact tables behind it
};
// lds_limit: dynamic LDS a workgroup may have (0: 64 KB); env_general: every column length through k_hilbert_env (A/B and test)
static inline const char *env_request(EnvRequest *rq, ImgForm form, uint32_t nx, uint32_t nz, const void *rf, const void *env,
                                      uint32_t lds_limit, bool env_general) {
    IMG_RULE(rf && env && nz <= ENV_MAX_N && (uint64_t)nx * nz < 0xffffffffull);
    // the one rule the two forms differ in: pbrt_envelope stages rf and env apart and so takes rf == env
    IMG_RULE(form == IMG_FORM_HOST || !img_overlap(rf, (size_t)nx * nz * 4, env, (size_t)nx * nz * 4));
    const uint32_t np = (nz + 3u) & ~3u, G = 2u * np + 8u, mp = ((nz >> 1) + 3u) & ~3u;
    const size_t lds_even = (size_t)(2u * mp + 4u * env_even_len(mp)) * 4;  // (its four tap tables: 3.3 x the column; 80 KB at 4096 samples)
    const bool even = (nz & 1u) == 0u && nz >= 8u && lds_even <= (lds_limit ? lds_limit : 65536u) && !env_general;
    const uint32_t threads = std::min(256u, img_div_up(img_div_up(nz, 4u), 64u) * 64u);  // (638 samples: 160 quads, three waves)
    *rq = EnvRequest{nx == 0 || nz == 0, nx, nz, np, G, mp, even, ImgLaunch{nx, 1u, threads, even ? lds_even : (size_t)(3u * np + 8u) * 4},
                     ImgLaunch{img_div_up(G + 4u * env_even_len(mp), 256), 1u, 256u, 0}};
    return nullptr;
}

struct LogRequest {
    bool empty;
    uint32_t n, nb;  // nb: blocks of the maximum, one word each
    float dynamic_range_db;
    ImgLaunch max_launch, launch;  // k_env_max, k_log_compress
};
static inline const char *log_request(LogRequest *rq, uint32_t n, const void *env, float dynamic_range_db, const void *out) {
    IMG_RULE(env && out && dynamic_range_db > 0.0f);
    const uint32_t nb = std::max(1u, std::min<uint32_t>(img_div_up(n, 1024), ENV_MAX_BLOCKS));
    *rq = LogRequest{n == 0, n, nb, dynamic_range_db, ImgLaunch{nb, 1u, 256u, 0}, ImgLaunch{img_div_up(n, 256), 1u, 256u, 0}};
    return nullptr;
}

struct IqEnvRequest { bool empty; uint32_t n; ImgLaunch launch; };  // k_iq_modulus: one thread per pixel
static inline const char *iq_env_request(IqEnvRequest *rq, uint32_t n, const void *iq, const void *env) {
    IMG_RULE(iq && env && !img_overlap(iq, (size_t)n * 8, env, (size_t)n * 4));
    *rq = IqEnvRequest{n == 0, n, ImgLaunch{img_div_up(n, 256), 1u, 256u, 0}};
    return nullptr;
}

struct FirRequest { bool empty; uint32_t nx, nz, K, per_col; ImgLaunch launch; };  // k_axial_fir; per_col: workgroups of a column, 256 outputs each
static inline const char *fir_request(FirRequest *rq, uint32_t nx, uint32_t nz, uint32_t K, const void *taps, const void *in, const void *out) {
    IMG_RULE(taps && in && out && !img_overlap(in, (size_t)nx * nz * 4, out, (size_t)nx * nz * 4));
    IMG_RULE(K <= FIR_MAX_K && nz > 0);
    const uint32_t per_col = img_div_up(nz, 256);
    IMG_RULE((uint64_t)nx * nz < 0xffffffffull && (uint64_t)nx * per_col < 0x7fffffffull);  // (the grid below)
    *rq = FirRequest{nx == 0, nx, nz, K, per_col, ImgLaunch{nx * per_col, 1u, 256u, img_fir_lds(K)}};
    return nullptr;
}

struct Rf2iqRequest {
    bool empty;
    uint32_t n_traces, T, D, K, Td, per_trace;  // Td: samples of a decimated trace; per_trace: its workgroups, 256 outputs each
    float fs, t0, demod_freq;
    ImgLaunch launch;  // k_rf2iq: the taps and two planes of 256 D + 2K mixed samples in LDS, <= 40 KB
};
static inline const char *rf2iq_request(Rf2iqRequest *rq, uint32_t n_traces, uint32_t T, float fs, float t0, float demod_freq, uint32_t D,
                                        uint32_t K, const void *taps, const void *in, const void *out) {
    IMG_RULE(taps && in && out);
    IMG_RULE(T > 0 && D >= 1u && D <= RF2IQ_MAX_D && K <= FIR_MAX_K);
    IMG_RULE(std::isfinite(fs) && fs > 0.0f && std::isfinite(t0));
    IMG_RULE(std::isfinite(demod_freq) && demod_freq >= 0.0f);
    const uint32_t Td = img_div_up(T, D), per_trace = img_div_up(Td, 256);
    IMG_RULE((uint64_t)n_traces * T < 0xffffffffull && (uint64_t)n_traces * per_trace < 0x7fffffffull);  // (the grid below)
    IMG_RULE(!img_overlap(in, (size_t)n_traces * T * 4, out, (size_t)n_traces * Td * 8));
    *rq = Rf2iqRequest{n_traces == 0, n_traces, T, D, K, Td, per_trace, fs, t0, demod_freq,
                       ImgLaunch{n_traces * per_trace, 1u, 256u, (size_t)(2 * K + 1 + 2 * (256 * D + 2 * K)) * 4}};
    return nullptr;
}

struct ScanConvertRequest {
    bool empty;  // (never: the rules ask for a pixel)
    const pbrt_scan_convert_params *p;
    size_t n_src, n_dst;
    ImgLaunch launch;  // k_scan_convert: one thread per pixel
};
static inline const char *scan_convert_request(ScanConvertRequest *rq, const pbrt_scan_convert_params *p, const void *src, const void *x,
                                               const void *z, const void *dst) {
    IMG_RULE(p && src && x && z && dst);
    IMG_RULE(p->n_theta >= 2u && p->n_rho >= 2u && p->nx > 0 && p->nz > 0);
    IMG_RULE((uint64_t)p->n_theta * p->n_rho < 0xffffffffull && (uint64_t)p->nx * p->nz < 0xffffffffull);
    IMG_RULE(std::isfinite(p->theta0) && std::isfinite(p->dtheta) && std::isfinite(p->rho0) && std::isfinite(p->drho));
    IMG_RULE(std::isfinite(p->ox) && std::isfinite(p->oz) && p->dtheta != 0.0 && p->drho != 0.0);
    const size_t n_src = (size_t)p->n_theta * p->n_rho, n_dst = (size_t)p->nx * p->nz;
    IMG_RULE(!img_overlap(src, n_src * 4, dst, n_dst * 4));
    *rq = ScanConvertRequest{n_dst == 0, p, n_src, n_dst, ImgLaunch{img_div_up(n_dst, 256), 1u, 256u, 0}};
    return nullptr;
}
