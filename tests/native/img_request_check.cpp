// Host check of the image-step requests (csrc/img_request.h; tests/test_img_request_host.py builds and runs it under the sanitizers).
// Per step -- pulse, envelope, log compression, axial FIR, rf2iq, I/Q envelope, scan conversion: every rule refuses its case with a
// text that names the argument and accepts the neighbouring boundary case (the envelope's overlap: refused for the _dev form, accepted
// for the host form); `empty` is "no output element" over a sweep; every accepted request of a sweep over the admitted ranges, ends
// included, has grid dimensions below 2^31 (the pulse's second one at most 65535), blocks that are multiples of 64 and at most 256,
// and dynamic LDS within 64 KB (the envelope's even kernel: within the limit handed in); and the launch shapes equal literals worked
// out by hand from the expressions the driver carried before the header (none is computed with the header under test).
// No pointer is read: the arrays are addresses far apart.  Prints one JSON line: {"checks": N, "failures": M}.
#include <cstdio>
#include <cstring>
#include <limits>

#include "img_request.h"

static int checks = 0, failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        ++checks;                                                     \
        if (!(cond)) {                                                \
            ++failures;                                               \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);   \
        }                                                             \
    } while (0)
// a refusal whose text holds `token`; an accepted call
#define REFUSED(call, token)                                                                                  \
    do {                                                                                                      \
        const char *why_ = (call);                                                                            \
        ++checks;                                                                                             \
        if (!why_ || !std::strstr(why_, token)) {                                                             \
            ++failures;                                                                                       \
            std::fprintf(stderr, "line %d: %s -> %s, expected a refusal with %s\n", __LINE__, #call, why_ ? why_ : "accepted", token); \
        }                                                                                                     \
    } while (0)
#define ACCEPTED(call)                                                                       \
    do {                                                                                     \
        const char *why_ = (call);                                                           \
        ++checks;                                                                            \
        if (why_) {                                                                          \
            ++failures;                                                                      \
            std::fprintf(stderr, "line %d: %s -> refused: %s\n", __LINE__, #call, why_);     \
        }                                                                                    \
    } while (0)

static void *at(uint64_t a) { return reinterpret_cast<void *>(static_cast<uintptr_t>(a)); }
static void *const A = at(0x10000), *const B = at(1ull << 38), *const H = at(1ull << 40), *const X = at(1ull << 41), *const Z = at(1ull << 42);
static const float NaN = std::numeric_limits<float>::quiet_NaN(), Inf = std::numeric_limits<float>::infinity();

static bool is(const ImgLaunch &l, uint32_t gx, uint32_t gy, uint32_t block, size_t lds) {
    return l.gx == gx && l.gy == gy && l.block == block && l.lds == lds;
}
// what every accepted, non-empty launch keeps
static void check_launch(const ImgLaunch &l, size_t lds_max = 65536) {
    CHECK(l.gx >= 1u && l.gx < 0x80000000u && l.gy >= 1u && l.gy <= 65535u);
    CHECK(l.block % 64u == 0u && l.block >= 64u && l.block <= 256u);
    CHECK(l.lds <= lds_max);
}

// K = ceil(2.5 sigma fs) at fs = 1 MHz: sigma = (k - 0.5) / 2.5e6 lands in the middle of (k - 1, k]
static float sigma_for(uint32_t k) { return (float)(((double)k - 0.5) / 2.5e6); }

static void pulse() {
    PulseRequest rq;
    const float fs = 1e6f, f = 5e6f, s = sigma_for(10);
    ACCEPTED(pulse_request(&rq, 2, 16, fs, f, s, A, B));
    CHECK(rq.K == 10u && !rq.empty && rq.n_traces == 2u && rq.T == 16u && rq.fs == fs && rq.frequency == f && rq.sigma == s);
    REFUSED(pulse_request(&rq, 2, 16, fs, f, s, nullptr, B), "in && out");
    REFUSED(pulse_request(&rq, 2, 16, fs, f, s, A, nullptr), "in && out");
    REFUSED(pulse_request(&rq, 2, 16, fs, f, s, A, A), "img_overlap");
    REFUSED(pulse_request(&rq, 2, 16, fs, f, s, A, at(0x10000 + 127)), "img_overlap");  // 2 x 16 floats: the last byte
    ACCEPTED(pulse_request(&rq, 2, 16, fs, f, s, A, at(0x10000 + 128)));
    ACCEPTED(pulse_request(&rq, 2, 16, fs, f, s, at(0x10000 + 128), A));
    REFUSED(pulse_request(&rq, 2, 16, 0.0f, f, s, A, B), "fs > 0.0f");
    REFUSED(pulse_request(&rq, 2, 16, NaN, f, s, A, B), "fs > 0.0f");
    REFUSED(pulse_request(&rq, 2, 16, fs, 0.0f, s, A, B), "frequency > 0.0f");
    REFUSED(pulse_request(&rq, 2, 16, fs, f, 0.0f, A, B), "sigma > 0.0f");
    REFUSED(pulse_request(&rq, 2, 16, fs, f, -s, A, B), "sigma > 0.0f");
    REFUSED(pulse_request(&rq, 2, 16, fs, f, NaN, A, B), "sigma > 0.0f");
    REFUSED(pulse_request(&rq, 65536, 16, fs, f, s, A, B), "n_traces <= 65535u");
    ACCEPTED(pulse_request(&rq, 65535, 16, fs, f, s, A, B));
    REFUSED(pulse_request(&rq, 65535, 65537, fs, f, s, A, B), "n_traces * T");  // 2^32 - 1 samples
    ACCEPTED(pulse_request(&rq, 65535, 65536, fs, f, s, A, B));
    REFUSED(pulse_request(&rq, 2, 16, fs, f, sigma_for(PULSE_MAX_K + 1), A, B), "K <= PULSE_MAX_K");
    REFUSED(pulse_request(&rq, 2, 16, fs, f, Inf, A, B), "K <= PULSE_MAX_K");
    REFUSED(pulse_request(&rq, 2, 16, 3e38f, f, 3e38f, A, B), "K <= PULSE_MAX_K");  // (a width no 32-bit count holds)
    ACCEPTED(pulse_request(&rq, 2, 16, fs, f, sigma_for(PULSE_MAX_K), A, B));
    CHECK(rq.K == 1024u);
    // two violations: the first in the order of the entry points
    REFUSED(pulse_request(&rq, 65536, 16, 0.0f, f, s, A, B), "fs > 0.0f");
    REFUSED(pulse_request(&rq, 65536, 16, fs, f, s, nullptr, B), "in && out");
    for (uint32_t nt = 0; nt < 3; ++nt)
        for (uint32_t T = 0; T < 3; ++T) {
            ACCEPTED(pulse_request(&rq, nt, T, fs, f, s, A, B));
            CHECK(rq.empty == ((uint64_t)nt * T == 0));
        }
    // launch shapes, by hand: grid (ceil(T / 256), n_traces), 256 threads, (2K + 1 + 256 + 2K) * 4 bytes
    ACCEPTED(pulse_request(&rq, 320, 638, 41e6f, f, 2e-7f, A, B));  // 2.5 * 2e-7 * 41e6 = 20.5
    CHECK(rq.K == 21u && is(rq.launch, 3, 320, 256, 1364));
    ACCEPTED(pulse_request(&rq, 1, 256, fs, f, 1e-9f, A, B));  // 0.0025
    CHECK(rq.K == 1u && is(rq.launch, 1, 1, 256, 1044));
    ACCEPTED(pulse_request(&rq, 65535, 257, fs, f, 4.094e-4f, A, B));  // 1023.5
    CHECK(rq.K == 1024u && is(rq.launch, 2, 65535, 256, 17412));
    ACCEPTED(pulse_request(&rq, 5, 65536, 33554432.0f, f, 2.384185791015625e-7f, A, B));  // 2^25 * 2^-22 * 2.5 = 20, exactly
    CHECK(rq.K == 20u && is(rq.launch, 256, 5, 256, 1348));
    for (uint32_t k = 1; k <= PULSE_MAX_K; ++k)
        for (uint32_t nt : {1u, 320u, 65535u})
            for (uint32_t T : {1u, 256u, 257u, 65536u}) {
                ACCEPTED(pulse_request(&rq, nt, T, fs, f, sigma_for(k), A, B));
                CHECK(rq.K == k && rq.launch.gy == nt && rq.launch.lds == (size_t)(4 * k + 257) * 4);
                check_launch(rq.launch);
            }
}

static void envelope() {
    EnvRequest rq;
    for (ImgForm form : {IMG_FORM_HOST, IMG_FORM_DEV}) {
        ACCEPTED(env_request(&rq, form, 2, 8, A, B, 65536, false));
        CHECK(!rq.empty && rq.nx == 2u && rq.nz == 8u);
        REFUSED(env_request(&rq, form, 2, 8, nullptr, B, 65536, false), "rf && env");
        REFUSED(env_request(&rq, form, 2, 8, A, nullptr, 65536, false), "rf && env");
        REFUSED(env_request(&rq, form, 2, ENV_MAX_N + 1, A, B, 65536, false), "nz <= ENV_MAX_N");
        ACCEPTED(env_request(&rq, form, 2, ENV_MAX_N, A, B, 65536, false));
        REFUSED(env_request(&rq, form, 1u << 20, ENV_MAX_N, A, B, 65536, false), "nx * nz");  // 2^32 samples
        REFUSED(env_request(&rq, form, 65535, 65537, A, B, 65536, false), "nz <= ENV_MAX_N");
        REFUSED(env_request(&rq, form, 0xffffffffu, 1, A, B, 65536, false), "nx * nz");         // 2^32 - 1
        ACCEPTED(env_request(&rq, form, 0xfffffffeu, 1, A, B, 65536, false));
        ACCEPTED(env_request(&rq, form, (1u << 20) - 1u, ENV_MAX_N, A, B, 65536, false));
        REFUSED(env_request(&rq, form, 0, ENV_MAX_N + 1, A, B, 65536, false), "nz <= ENV_MAX_N");  // a rule comes before `empty`
        ACCEPTED(env_request(&rq, form, 2, 8, A, at(0x10000 + 64), 65536, false));                 // 2 x 8 floats: adjacent
        for (uint32_t nx = 0; nx < 3; ++nx)
            for (uint32_t nz = 0; nz < 3; ++nz) {
                ACCEPTED(env_request(&rq, form, nx, nz, A, B, 65536, false));
                CHECK(rq.empty == ((uint64_t)nx * nz == 0));
            }
    }
    // the one rule the forms differ in
    REFUSED(env_request(&rq, IMG_FORM_DEV, 2, 8, A, A, 65536, false), "img_overlap");
    REFUSED(env_request(&rq, IMG_FORM_DEV, 2, 8, A, at(0x10000 + 63), 65536, false), "img_overlap");
    REFUSED(env_request(&rq, IMG_FORM_DEV, 2, 8, at(0x10000 + 63), A, 65536, false), "img_overlap");
    ACCEPTED(env_request(&rq, IMG_FORM_HOST, 2, 8, A, A, 65536, false));
    ACCEPTED(env_request(&rq, IMG_FORM_HOST, 2, 8, A, at(0x10000 + 4), 65536, false));
    // launch shapes, by hand.  Np = nz rounded up to 4, G = 2 Np + 8, Mp = nz / 2 rounded up to 4; the even kernel (nz even, >= 8,
    // its LDS within the limit): (2 Mp + 4 (2 Mp + 16)) * 4 bytes; the general one: (3 Np + 8) * 4; threads: the quads of a column
    // in whole waves, at most 256; the tap-table kernel: ceil((G + 4 (2 Mp + 16)) / 256) blocks of 256
    ACCEPTED(env_request(&rq, IMG_FORM_DEV, 100, 638, A, B, 65536, false));
    CHECK(rq.even && rq.np == 640u && rq.G == 1288u && rq.mp == 320u && is(rq.launch, 100, 1, 192, 13056) && is(rq.taps_launch, 16, 1, 256, 0));
    ACCEPTED(env_request(&rq, IMG_FORM_DEV, 100, 637, A, B, 65536, false));
    CHECK(!rq.even && rq.np == 640u && rq.mp == 320u && is(rq.launch, 100, 1, 192, 7712) && is(rq.taps_launch, 16, 1, 256, 0));
    ACCEPTED(env_request(&rq, IMG_FORM_DEV, 100, 638, A, B, 65536, true));  // PBRT_ENV_GENERAL
    CHECK(!rq.even && is(rq.launch, 100, 1, 192, 7712));
    ACCEPTED(env_request(&rq, IMG_FORM_HOST, 3, 8, A, B, 65536, false));  // the shortest even column: Np = 8, G = 24, Mp = 4
    CHECK(rq.even && rq.np == 8u && rq.G == 24u && rq.mp == 4u && is(rq.launch, 3, 1, 64, 416) && is(rq.taps_launch, 1, 1, 256, 0));
    ACCEPTED(env_request(&rq, IMG_FORM_HOST, 3, 6, A, B, 65536, false));  // even, but below 8
    CHECK(!rq.even && is(rq.launch, 3, 1, 64, 128));
    ACCEPTED(env_request(&rq, IMG_FORM_HOST, 1, 1, A, B, 65536, false));  // Np = 4, G = 16, Mp = 0
    CHECK(!rq.even && rq.np == 4u && rq.G == 16u && rq.mp == 0u && is(rq.launch, 1, 1, 64, 80) && is(rq.taps_launch, 1, 1, 256, 0));
    ACCEPTED(env_request(&rq, IMG_FORM_DEV, 7, 4096, A, B, 65536, false));  // Mp = 2048: 82176 bytes, over the limit
    CHECK(!rq.even && is(rq.launch, 7, 1, 256, 49184) && is(rq.taps_launch, 97, 1, 256, 0));
    ACCEPTED(env_request(&rq, IMG_FORM_DEV, 7, 4096, A, B, 0, false));  // (no limit known: 64 KB)
    CHECK(!rq.even && is(rq.launch, 7, 1, 256, 49184));
    ACCEPTED(env_request(&rq, IMG_FORM_DEV, 7, 4096, A, B, 163840, false));
    CHECK(rq.even && is(rq.launch, 7, 1, 256, 82176));
    ACCEPTED(env_request(&rq, IMG_FORM_DEV, 7, 3264, A, B, 65536, false));  // Mp = 1632: (3264 + 4 * 3280) * 4 = 65536, the last one within
    CHECK(rq.even && is(rq.launch, 7, 1, 256, 65536));
    ACCEPTED(env_request(&rq, IMG_FORM_DEV, 7, 3266, A, B, 65536, false));  // Mp = 1636: 65696; Np = 3268
    CHECK(!rq.even && is(rq.launch, 7, 1, 256, 39248));
    for (uint32_t limit : {65536u, 32768u, 163840u, 0u})
        for (uint32_t nz = 1; nz <= ENV_MAX_N; ++nz)
            for (int general = 0; general < 2; ++general) {
                ACCEPTED(env_request(&rq, IMG_FORM_DEV, nz % 5u == 0u ? 0x000fffffu : 100u, nz, A, B, limit, general != 0));
                check_launch(rq.launch, rq.even ? (limit ? limit : 65536u) : 65536u);
                check_launch(rq.taps_launch);
                CHECK(rq.launch.block * 4u >= std::min(nz, 1024u) && (!rq.even || (nz % 2u == 0u && nz >= 8u && !general)));
                CHECK(rq.taps_launch.gx * 256u >= rq.G + 4u * (2u * rq.mp + 16u) && rq.np >= nz && rq.np < nz + 4u && 2u * rq.mp >= nz - (nz & 1u));
            }
}

static void log_compression() {
    LogRequest rq;
    ACCEPTED(log_request(&rq, 16, A, 50.0f, B));
    CHECK(!rq.empty && rq.n == 16u && rq.dynamic_range_db == 50.0f);
    ACCEPTED(log_request(&rq, 16, A, 50.0f, A));  // in place: no rule against it
    REFUSED(log_request(&rq, 16, nullptr, 50.0f, B), "env && out");
    REFUSED(log_request(&rq, 16, A, 50.0f, nullptr), "env && out");
    REFUSED(log_request(&rq, 16, A, 0.0f, B), "dynamic_range_db > 0.0f");
    REFUSED(log_request(&rq, 16, A, -1.0f, B), "dynamic_range_db > 0.0f");
    REFUSED(log_request(&rq, 16, A, NaN, B), "dynamic_range_db > 0.0f");
    REFUSED(log_request(&rq, 0, A, 0.0f, B), "dynamic_range_db > 0.0f");  // a rule comes before `empty`
    ACCEPTED(log_request(&rq, 16, A, 1e-30f, B));
    ACCEPTED(log_request(&rq, 16, A, Inf, B));
    for (uint32_t n = 0; n < 3; ++n) {
        ACCEPTED(log_request(&rq, n, A, 50.0f, B));
        CHECK(rq.empty == (n == 0));
    }
    // by hand: the maximum over max(1, min(ceil(n / 1024), 256)) blocks, the compression over ceil(n / 256) blocks, 256 threads
    ACCEPTED(log_request(&rq, 5000, A, 50.0f, B));
    CHECK(rq.nb == 5u && is(rq.max_launch, 5, 1, 256, 0) && is(rq.launch, 20, 1, 256, 0));
    ACCEPTED(log_request(&rq, 1, A, 50.0f, B));
    CHECK(rq.nb == 1u && is(rq.max_launch, 1, 1, 256, 0) && is(rq.launch, 1, 1, 256, 0));
    ACCEPTED(log_request(&rq, 262144, A, 50.0f, B));
    CHECK(rq.nb == 256u && is(rq.max_launch, 256, 1, 256, 0) && is(rq.launch, 1024, 1, 256, 0));
    ACCEPTED(log_request(&rq, 262145, A, 50.0f, B));
    CHECK(rq.nb == 256u && is(rq.max_launch, 256, 1, 256, 0) && is(rq.launch, 1025, 1, 256, 0));
    ACCEPTED(log_request(&rq, 0xffffffffu, A, 50.0f, B));
    CHECK(rq.nb == 256u && is(rq.launch, 16777216, 1, 256, 0));
    for (uint64_t n = 1; n <= 0xffffffffull; n = n * 3 + 1) {
        ACCEPTED(log_request(&rq, (uint32_t)n, A, 50.0f, B));
        check_launch(rq.max_launch);
        check_launch(rq.launch);
        CHECK(rq.nb == rq.max_launch.gx && rq.nb <= ENV_MAX_BLOCKS && (uint64_t)rq.launch.gx * 256u >= n);
    }
}

static void iq_envelope() {
    IqEnvRequest rq;
    ACCEPTED(iq_env_request(&rq, 16, A, B));
    CHECK(!rq.empty && rq.n == 16u);
    REFUSED(iq_env_request(&rq, 16, nullptr, B), "iq && env");
    REFUSED(iq_env_request(&rq, 16, A, nullptr), "iq && env");
    REFUSED(iq_env_request(&rq, 0, nullptr, B), "iq && env");  // a rule comes before `empty`
    REFUSED(iq_env_request(&rq, 16, A, A), "img_overlap");
    REFUSED(iq_env_request(&rq, 16, A, at(0x10000 + 127)), "img_overlap");  // 16 pairs: 128 bytes
    ACCEPTED(iq_env_request(&rq, 16, A, at(0x10000 + 128)));
    REFUSED(iq_env_request(&rq, 16, at(0x10000 + 63), A), "img_overlap");   // 16 moduli: 64 bytes
    ACCEPTED(iq_env_request(&rq, 16, at(0x10000 + 64), A));
    for (uint32_t n = 0; n < 3; ++n) {
        ACCEPTED(iq_env_request(&rq, n, A, B));
        CHECK(rq.empty == (n == 0));
    }
    ACCEPTED(iq_env_request(&rq, 5000, A, B));  // by hand: one thread per pixel, 256 a block
    CHECK(is(rq.launch, 20, 1, 256, 0));
    ACCEPTED(iq_env_request(&rq, 256, A, B));
    CHECK(is(rq.launch, 1, 1, 256, 0));
    ACCEPTED(iq_env_request(&rq, 257, A, B));
    CHECK(is(rq.launch, 2, 1, 256, 0));
    ACCEPTED(iq_env_request(&rq, 0xffffffffu, A, B));
    CHECK(is(rq.launch, 16777216, 1, 256, 0));
}

static void axial_fir() {
    FirRequest rq;
    ACCEPTED(fir_request(&rq, 2, 8, 2, H, A, B));
    CHECK(!rq.empty && rq.nx == 2u && rq.nz == 8u && rq.K == 2u);
    REFUSED(fir_request(&rq, 2, 8, 2, nullptr, A, B), "taps && in && out");
    REFUSED(fir_request(&rq, 2, 8, 2, H, nullptr, B), "taps && in && out");
    REFUSED(fir_request(&rq, 2, 8, 2, H, A, nullptr), "taps && in && out");
    REFUSED(fir_request(&rq, 2, 8, 2, H, A, A), "img_overlap");
    REFUSED(fir_request(&rq, 2, 8, 2, H, A, at(0x10000 + 63)), "img_overlap");
    ACCEPTED(fir_request(&rq, 2, 8, 2, H, A, at(0x10000 + 64)));
    REFUSED(fir_request(&rq, 2, 8, FIR_MAX_K + 1, H, A, B), "K <= FIR_MAX_K");
    ACCEPTED(fir_request(&rq, 2, 8, FIR_MAX_K, H, A, B));
    ACCEPTED(fir_request(&rq, 2, 8, 0, H, A, B));
    REFUSED(fir_request(&rq, 2, 0, 2, H, A, B), "nz > 0");
    REFUSED(fir_request(&rq, 0, 0, 2, H, A, B), "nz > 0");
    ACCEPTED(fir_request(&rq, 2, 1, 2, H, A, B));
    REFUSED(fir_request(&rq, 65535, 65537, 2, H, A, B), "nx * nz");  // 2^32 - 1 samples
    ACCEPTED(fir_request(&rq, 65536, 65535, 2, H, A, B));
    CHECK(rq.per_col == 256u && is(rq.launch, 16777216, 1, 256, 1060));
    REFUSED(fir_request(&rq, 0x7fffffffu, 1, 2, H, A, B), "nx * per_col");  // 2^31 - 1 workgroups
    ACCEPTED(fir_request(&rq, 0x7ffffffeu, 1, 2, H, A, B));
    CHECK(is(rq.launch, 0x7ffffffeu, 1, 256, 1060));
    REFUSED(fir_request(&rq, 0x7fffffffu, 2, 2, H, A, B), "nx * per_col");
    for (uint32_t nx = 0; nx < 3; ++nx)
        for (uint32_t nz = 1; nz < 3; ++nz) {
            ACCEPTED(fir_request(&rq, nx, nz, 2, H, A, B));
            CHECK(rq.empty == (nx == 0));
        }
    // by hand: ceil(nz / 256) workgroups a column, 256 threads, (2K + 1 + 256 + 2K) * 4 bytes
    ACCEPTED(fir_request(&rq, 100, 638, 16, H, A, B));
    CHECK(rq.per_col == 3u && is(rq.launch, 300, 1, 256, 1284));
    ACCEPTED(fir_request(&rq, 1, 256, 0, H, A, B));
    CHECK(rq.per_col == 1u && is(rq.launch, 1, 1, 256, 1028));
    ACCEPTED(fir_request(&rq, 7, 257, FIR_MAX_K, H, A, B));
    CHECK(rq.per_col == 2u && is(rq.launch, 14, 1, 256, 17412));
    for (uint32_t K = 0; K <= FIR_MAX_K; ++K)
        for (uint32_t nz : {1u, 255u, 256u, 257u, 638u, 65535u})
            for (uint32_t nx : {1u, 100u, 65536u}) {
                ACCEPTED(fir_request(&rq, nx, nz, K, H, A, B));
                check_launch(rq.launch);
                CHECK((uint64_t)rq.per_col * 256u >= nz && rq.launch.gx == nx * rq.per_col && rq.launch.lds == (size_t)(4 * K + 257) * 4);
            }
}

static void rf2iq() {
    Rf2iqRequest rq;
    const float fs = 40e6f, fd = 5e6f;
    ACCEPTED(rf2iq_request(&rq, 2, 16, fs, 0.0f, fd, 2, 2, H, A, B));
    CHECK(!rq.empty && rq.n_traces == 2u && rq.T == 16u && rq.D == 2u && rq.K == 2u && rq.Td == 8u && rq.fs == fs && rq.t0 == 0.0f && rq.demod_freq == fd);
    REFUSED(rf2iq_request(&rq, 2, 16, fs, 0.0f, fd, 2, 2, nullptr, A, B), "taps && in && out");
    REFUSED(rf2iq_request(&rq, 2, 16, fs, 0.0f, fd, 2, 2, H, nullptr, B), "taps && in && out");
    REFUSED(rf2iq_request(&rq, 2, 16, fs, 0.0f, fd, 2, 2, H, A, nullptr), "taps && in && out");
    REFUSED(rf2iq_request(&rq, 2, 0, fs, 0.0f, fd, 2, 2, H, A, B), "T > 0");
    REFUSED(rf2iq_request(&rq, 0, 0, fs, 0.0f, fd, 2, 2, H, A, B), "T > 0");
    ACCEPTED(rf2iq_request(&rq, 2, 1, fs, 0.0f, fd, 2, 2, H, A, B));
    REFUSED(rf2iq_request(&rq, 2, 16, fs, 0.0f, fd, 0, 2, H, A, B), "D >= 1u");
    ACCEPTED(rf2iq_request(&rq, 2, 16, fs, 0.0f, fd, 1, 2, H, A, B));
    REFUSED(rf2iq_request(&rq, 2, 16, fs, 0.0f, fd, RF2IQ_MAX_D + 1, 2, H, A, B), "D <= RF2IQ_MAX_D");
    ACCEPTED(rf2iq_request(&rq, 2, 16, fs, 0.0f, fd, RF2IQ_MAX_D, 2, H, A, B));
    REFUSED(rf2iq_request(&rq, 2, 16, fs, 0.0f, fd, 2, FIR_MAX_K + 1, H, A, B), "K <= FIR_MAX_K");
    ACCEPTED(rf2iq_request(&rq, 2, 16, fs, 0.0f, fd, 2, FIR_MAX_K, H, A, B));
    ACCEPTED(rf2iq_request(&rq, 2, 16, fs, 0.0f, fd, 2, 0, H, A, B));
    REFUSED(rf2iq_request(&rq, 2, 16, 0.0f, 0.0f, fd, 2, 2, H, A, B), "fs > 0.0f");
    REFUSED(rf2iq_request(&rq, 2, 16, Inf, 0.0f, fd, 2, 2, H, A, B), "isfinite(fs)");
    REFUSED(rf2iq_request(&rq, 2, 16, NaN, 0.0f, fd, 2, 2, H, A, B), "isfinite(fs)");
    REFUSED(rf2iq_request(&rq, 2, 16, fs, NaN, fd, 2, 2, H, A, B), "isfinite(t0)");
    REFUSED(rf2iq_request(&rq, 2, 16, fs, -Inf, fd, 2, 2, H, A, B), "isfinite(t0)");
    ACCEPTED(rf2iq_request(&rq, 2, 16, fs, -1.0f, fd, 2, 2, H, A, B));
    REFUSED(rf2iq_request(&rq, 2, 16, fs, 0.0f, -1.0f, 2, 2, H, A, B), "demod_freq >= 0.0f");
    REFUSED(rf2iq_request(&rq, 2, 16, fs, 0.0f, NaN, 2, 2, H, A, B), "isfinite(demod_freq)");
    REFUSED(rf2iq_request(&rq, 2, 16, fs, 0.0f, Inf, 2, 2, H, A, B), "isfinite(demod_freq)");
    ACCEPTED(rf2iq_request(&rq, 2, 16, fs, 0.0f, 0.0f, 2, 2, H, A, B));
    REFUSED(rf2iq_request(&rq, 65535, 65537, fs, 0.0f, fd, 2, 2, H, A, B), "n_traces * T");
    ACCEPTED(rf2iq_request(&rq, 65536, 65535, fs, 0.0f, fd, 1, 2, H, A, B));
    CHECK(rq.Td == 65535u && rq.per_trace == 256u && is(rq.launch, 16777216, 1, 256, 2100));
    REFUSED(rf2iq_request(&rq, 0x7fffffffu, 1, fs, 0.0f, fd, 2, 2, H, A, B), "n_traces * per_trace");
    ACCEPTED(rf2iq_request(&rq, 0x7ffffffeu, 1, fs, 0.0f, fd, 2, 2, H, A, B));
    REFUSED(rf2iq_request(&rq, 2, 16, fs, 0.0f, fd, 2, 2, H, A, A), "img_overlap");
    REFUSED(rf2iq_request(&rq, 2, 16, fs, 0.0f, fd, 2, 2, H, A, at(0x10000 + 127)), "img_overlap");  // in: 2 x 16 floats
    ACCEPTED(rf2iq_request(&rq, 2, 16, fs, 0.0f, fd, 2, 2, H, A, at(0x10000 + 128)));
    REFUSED(rf2iq_request(&rq, 2, 16, fs, 0.0f, fd, 4, 2, H, at(0x10000 + 63), A), "img_overlap");    // out: 2 x 4 pairs
    ACCEPTED(rf2iq_request(&rq, 2, 16, fs, 0.0f, fd, 4, 2, H, at(0x10000 + 64), A));
    for (uint32_t nt = 0; nt < 3; ++nt)
        for (uint32_t T = 1; T < 3; ++T) {
            ACCEPTED(rf2iq_request(&rq, nt, T, fs, 0.0f, fd, 2, 2, H, A, B));
            CHECK(rq.empty == (nt == 0));
        }
    // by hand: Td = ceil(T / D), ceil(Td / 256) workgroups a trace, 256 threads, (2K + 1 + 2 (256 D + 2K)) * 4 bytes
    ACCEPTED(rf2iq_request(&rq, 320, 638, fs, 0.0f, fd, 4, 16, H, A, B));
    CHECK(rq.Td == 160u && rq.per_trace == 1u && is(rq.launch, 320, 1, 256, 8580));
    ACCEPTED(rf2iq_request(&rq, 3, 4097, fs, 0.0f, fd, 1, 0, H, A, B));
    CHECK(rq.Td == 4097u && rq.per_trace == 17u && is(rq.launch, 51, 1, 256, 2052));
    ACCEPTED(rf2iq_request(&rq, 2, 16, fs, 0.0f, fd, 8, 1024, H, A, B));
    CHECK(rq.Td == 2u && rq.per_trace == 1u && is(rq.launch, 2, 1, 256, 40964));
    ACCEPTED(rf2iq_request(&rq, 5, 2049, fs, 0.0f, fd, 8, 3, H, A, B));
    CHECK(rq.Td == 257u && rq.per_trace == 2u && is(rq.launch, 10, 1, 256, 16460));
    for (uint32_t D = 1; D <= RF2IQ_MAX_D; ++D)
        for (uint32_t K : {0u, 1u, 16u, 1023u, 1024u})
            for (uint32_t T : {1u, 255u, 256u, 257u, 638u, 65536u})
                for (uint32_t nt : {1u, 320u, 65535u}) {
                    ACCEPTED(rf2iq_request(&rq, nt, T, fs, 0.0f, fd, D, K, H, A, B));
                    check_launch(rq.launch);
                    CHECK((uint64_t)rq.Td * D >= T && (uint64_t)(rq.Td - 1u) * D < T && (uint64_t)rq.per_trace * 256u >= rq.Td);
                    CHECK(rq.launch.gx == nt * rq.per_trace && rq.launch.lds == (size_t)(6 * K + 1 + 512 * D) * 4);
                }
}

static void scan_conversion() {
    ScanConvertRequest rq;
    const pbrt_scan_convert_params ok{4, 4, 2, 8, -0.3, 0.2, 0.01, 0.01, 0.0, 0.0, 0.0f, 0};
    const double dNaN = std::numeric_limits<double>::quiet_NaN(), dInf = std::numeric_limits<double>::infinity();
    ACCEPTED(scan_convert_request(&rq, &ok, A, X, Z, B));
    CHECK(!rq.empty && rq.p == &ok && rq.n_src == 16u && rq.n_dst == 16u && is(rq.launch, 1, 1, 256, 0));
    REFUSED(scan_convert_request(&rq, nullptr, A, X, Z, B), "p && src");
    REFUSED(scan_convert_request(&rq, &ok, nullptr, X, Z, B), "p && src");
    REFUSED(scan_convert_request(&rq, &ok, A, nullptr, Z, B), "p && src");
    REFUSED(scan_convert_request(&rq, &ok, A, X, nullptr, B), "p && src");
    REFUSED(scan_convert_request(&rq, &ok, A, X, Z, nullptr), "p && src");
    REFUSED(scan_convert_request(&rq, &ok, A, X, Z, A), "img_overlap");
    REFUSED(scan_convert_request(&rq, &ok, A, X, Z, at(0x10000 + 63)), "img_overlap");
    ACCEPTED(scan_convert_request(&rq, &ok, A, X, Z, at(0x10000 + 64)));
    pbrt_scan_convert_params p;
#define EDIT(field, value, token)                                     \
    p = ok;                                                           \
    p.field = value;                                                  \
    REFUSED(scan_convert_request(&rq, &p, A, X, Z, B), token)
#define EDIT_OK(field, value)                                         \
    p = ok;                                                           \
    p.field = value;                                                  \
    ACCEPTED(scan_convert_request(&rq, &p, A, X, Z, B))
    EDIT(n_theta, 1, "n_theta >= 2u");
    EDIT(n_rho, 1, "n_rho >= 2u");
    EDIT_OK(n_theta, 2);
    EDIT_OK(n_rho, 2);
    EDIT(nx, 0, "nx > 0");
    EDIT(nz, 0, "nz > 0");
    EDIT(theta0, dNaN, "isfinite(p->theta0)");
    EDIT(dtheta, dInf, "isfinite(p->dtheta)");
    EDIT(rho0, -dInf, "isfinite(p->rho0)");
    EDIT(drho, dNaN, "isfinite(p->drho)");
    EDIT(ox, dInf, "isfinite(p->ox)");
    EDIT(oz, dNaN, "isfinite(p->oz)");
    EDIT(dtheta, 0.0, "dtheta != 0.0");
    EDIT(drho, 0.0, "drho != 0.0");
    EDIT_OK(dtheta, -0.2);
    EDIT_OK(drho, 1e-300);
    p = ok, p.n_theta = 65535, p.n_rho = 65537;
    REFUSED(scan_convert_request(&rq, &p, A, X, Z, B), "n_theta * p->n_rho");
    p = ok, p.n_theta = 65536, p.n_rho = 65535;
    ACCEPTED(scan_convert_request(&rq, &p, A, X, Z, B));
    p = ok, p.nx = 65535, p.nz = 65537;
    REFUSED(scan_convert_request(&rq, &p, A, X, Z, B), "nx * p->nz");
    // by hand: one thread per pixel, 256 a block
    p = ok, p.nx = 65535, p.nz = 65536;
    ACCEPTED(scan_convert_request(&rq, &p, A, X, Z, B));
    CHECK(!rq.empty && rq.n_dst == 0xffff0000ull && is(rq.launch, 16776960, 1, 256, 0));
    check_launch(rq.launch);
    p = ok, p.nx = 100, p.nz = 638;
    ACCEPTED(scan_convert_request(&rq, &p, A, X, Z, B));
    CHECK(is(rq.launch, 250, 1, 256, 0));
    p = ok, p.nx = 1, p.nz = 1;
    ACCEPTED(scan_convert_request(&rq, &p, A, X, Z, B));
    CHECK(!rq.empty && is(rq.launch, 1, 1, 256, 0));
    p = ok, p.nx = 257, p.nz = 1;
    ACCEPTED(scan_convert_request(&rq, &p, A, X, Z, B));
    CHECK(is(rq.launch, 2, 1, 256, 0));
}

int main() {
    CHECK(FIR_MAX_K == 1024 && RF2IQ_MAX_D == 8 && ENV_MAX_N == 4096 && ENV_MAX_BLOCKS == 256u && PULSE_MAX_K == 1024);
    CHECK(env_even_len(0) == 16u && env_even_len(320) == 656u && env_even_len(2048) == 4112u);
    pulse();
    envelope();
    log_compression();
    iq_envelope();
    axial_fir();
    rf2iq();
    scan_conversion();
    std::printf("{\"checks\": %d, \"failures\": %d}\n", checks, failures);
    return failures ? 1 : 0;
}
