// Host check of the spatial-coherence request in csrc/coherence_request.h (tests/test_coherence_request_host.py builds and runs it under
// the sanitizers): the maker of a pbrt_coherence_params takes every valid block and fills the request (the I/Q request of bf_request,
// kind, half_kernel, lag_prop, gamma, the width of a pixel and the dynamic LDS of a workgroup), refuses every single violation of its
// own rules (a method other than PBRT_SCAN_IQ, tables > 1, a kind other than SLSC and CF -- a zeroed block among them --, more than
// COH_MAX_E elements; SLSC: lag_prop not finite or outside (0, 1], half_kernel > 4; CF: gamma not finite or outside [0, 4], half_kernel
// != 0) and everything a pbrt_scan_params refuses; and the lag rule coherence_lags, which the host and the kernel share, on its table.
// Prints one JSON line: {"checks": N, "failures": M}.  With the argument "lags": the table `N lag_prop M` of coherence_lags for every
// N <= 256 and the lag_props that follow on the command line, for tests/test_coherence_restatement.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "coherence_request.h"

static int checks = 0, failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        ++checks;                                                     \
        if (!(cond)) {                                                \
            ++failures;                                               \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);   \
        }                                                             \
    } while (0)

static const float NaN = std::numeric_limits<float>::quiet_NaN(), Inf = std::numeric_limits<float>::infinity();

static pbrt_coherence_params valid(uint32_t kind) {
    pbrt_coherence_params c;
    std::memset(&c, 0, sizeof c);
    pbrt_das_params &d = c.scan.das;
    d.n_angles = 2, d.n_elements = 64, d.time_samples = 16;
    d.fs = 5e6f, d.sound_speed = 1540.0f, d.t0 = 0.0f, d.f_number = 1.0f;
    d.interpolation = PBRT_DAS_LINEAR, d.compound_mean = 0, d.nx = 5, d.nz = 7;
    c.scan.method = PBRT_SCAN_IQ, c.scan.p = 2.0f, c.scan.demod_freq = 2e6f, c.scan.probe = 0u;
    c.tables = 0u, c.kind = kind, c.half_kernel = kind == PBRT_COH_SLSC ? 1u : 0u, c.lag_prop = 0.3f, c.gamma = 1.0f;
    return c;
}
static bool refused(const char *why) { return why != nullptr && why[0] != '\0'; }
static bool mentions(const char *why, const char *word) { return why != nullptr && std::strstr(why, word) != nullptr; }

// one edit of a valid request of `kind`: taken, or refused (with a rule text that names `word`)
template <class Edit>
static void rule(uint32_t kind, bool taken, Edit edit, const char *word = nullptr) {
    pbrt_coherence_params c = valid(kind);
    edit(c);
    CoherenceRequest rq;
    const char *why = coherence_request(&rq, &c);
    CHECK(refused(why) == !taken);
    if (!taken && word) CHECK(mentions(why, word));
}

static uint32_t lags_by_hand(uint32_t N, float lag_prop) {
    if (N < 2u) return 0u;
    const float prod = lag_prop * (float)N;
    uint32_t M = 0;
    while ((float)(M + 1u) <= prod) ++M;  // floor of a non-negative product
    if (M < 1u) M = 1u;
    if (M > N - 1u) M = N - 1u;
    return M > 64u ? 64u : M;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::strcmp(argv[1], "lags") == 0) {
        for (int k = 2; k < argc; ++k) {
            const float lp = std::strtof(argv[k], nullptr);
            for (uint32_t N = 0; N <= COH_MAX_E; ++N) std::printf("%u %.9g %u\n", N, (double)lp, coherence_lags(N, lp));
        }
        return 0;
    }
    CHECK(COH_MAX_E == 256u && COH_MAX_H == 4u && COH_MAX_LAG == 64u);
    CHECK(PBRT_COH_SLSC != 0u && PBRT_COH_CF != 0u && PBRT_COH_SLSC != PBRT_COH_CF);
    CHECK(sizeof(pbrt_coherence_params) == sizeof(pbrt_scan_params) + 20u);

    // ---- every valid block: both kinds x both probes x both scan kinds x both interpolations x settings -> the request as filled ----
    for (uint32_t probe = 0; probe <= 1u; ++probe)
        for (uint32_t tables = 0; tables <= 1u; ++tables)
            for (uint32_t interp = 0; interp <= 1u; ++interp) {
                for (float lp : {1e-6f, 0.1f, 0.3f, 1.0f})
                    for (uint32_t H = 0; H <= COH_MAX_H; ++H) {
                        pbrt_coherence_params c = valid(PBRT_COH_SLSC);
                        c.scan.probe = probe, c.tables = tables, c.scan.das.interpolation = interp, c.lag_prop = lp, c.half_kernel = H;
                        c.gamma = NaN;  // (gamma is read by CF only)
                        CoherenceRequest rq;
                        std::memset(&rq, 0xff, sizeof rq);
                        CHECK(coherence_request(&rq, &c) == nullptr);
                        CHECK(rq.bf.das == &c.scan.das && rq.bf.method == PBRT_SCAN_IQ && rq.bf.pw == 2e6f);
                        CHECK(rq.bf.probe == (probe != 0) && rq.bf.tab == (tables != 0) && rq.bf.window == PBRT_APOD_BOXCAR);
                        CHECK(rq.kind == PBRT_COH_SLSC && rq.half_kernel == H && rq.lag_prop == lp && rq.width == 1u);
                        CHECK(rq.lds_bytes == 4u * 64u * (2u * H + 1u) * 8u);
                    }
                for (float g : {0.0f, -0.0f, 0.5f, 1.0f, 2.0f, 4.0f}) {
                    pbrt_coherence_params c = valid(PBRT_COH_CF);
                    c.scan.probe = probe, c.tables = tables, c.scan.das.interpolation = interp, c.gamma = g;
                    c.lag_prop = NaN;  // (lag_prop is read by SLSC only)
                    CoherenceRequest rq;
                    std::memset(&rq, 0xff, sizeof rq);
                    CHECK(coherence_request(&rq, &c) == nullptr);
                    CHECK(rq.bf.das == &c.scan.das && rq.bf.method == PBRT_SCAN_IQ && rq.bf.pw == 2e6f);
                    CHECK(rq.bf.probe == (probe != 0) && rq.bf.tab == (tables != 0) && rq.bf.window == PBRT_APOD_BOXCAR);
                    CHECK(rq.kind == PBRT_COH_CF && rq.half_kernel == 0u && rq.gamma == g && rq.width == 2u);
                    CHECK(rq.lds_bytes == 4u * 64u * 8u);
                }
            }
    for (uint32_t kind : {(uint32_t)PBRT_COH_SLSC, (uint32_t)PBRT_COH_CF}) {
        for (uint32_t e : {1u, 3u, 255u, 256u}) rule(kind, true, [e](pbrt_coherence_params &c) { c.scan.das.n_elements = e; });
        rule(kind, true, [](pbrt_coherence_params &c) { c.scan.das.f_number = 0.0f; });
        rule(kind, true, [](pbrt_coherence_params &c) { c.scan.p = NaN; });  // (p is read by p-DAS only)
        rule(kind, true, [](pbrt_coherence_params &) {});
    }
    {   // the worst case of the dynamic LDS: 72 KB per workgroup
        pbrt_coherence_params c = valid(PBRT_COH_SLSC);
        c.scan.das.n_elements = COH_MAX_E, c.half_kernel = COH_MAX_H;
        CoherenceRequest rq;
        CHECK(coherence_request(&rq, &c) == nullptr && rq.lds_bytes == 72u * 1024u);
    }

    // ---- the rules of the block, one violation at a time ----
    CHECK(refused(coherence_request(nullptr, nullptr)));
    {   // a zeroed block
        pbrt_coherence_params c;
        std::memset(&c, 0, sizeof c);
        CoherenceRequest rq;
        CHECK(refused(coherence_request(&rq, &c)));
        c = valid(PBRT_COH_SLSC);
        c.kind = 0u;
        CHECK(mentions(coherence_request(&rq, &c), "kind"));
    }
    for (uint32_t kind : {(uint32_t)PBRT_COH_SLSC, (uint32_t)PBRT_COH_CF}) {
        for (uint32_t m : {(uint32_t)PBRT_SCAN_DAS, (uint32_t)PBRT_BF_PDAS, (uint32_t)PBRT_BF_FDMAS, 4u, 0xffffffffu})
            rule(kind, false, [m](pbrt_coherence_params &c) { c.scan.method = m; }, "method");
        for (uint32_t t : {2u, 3u, 0xffffffffu}) rule(kind, false, [t](pbrt_coherence_params &c) { c.tables = t; }, "tables");
        for (uint32_t k : {0u, 3u, 4u, 0xffffffffu}) rule(kind, false, [k](pbrt_coherence_params &c) { c.kind = k; }, "kind");
        for (uint32_t e : {257u, 512u, 0xffffffffu})
            rule(kind, false, [e](pbrt_coherence_params &c) { c.scan.das.n_elements = e; }, "n_elements");
    }
    // SLSC
    for (float lp : {0.0f, -0.0f, -0.3f, std::nextafter(1.0f, 2.0f), 2.0f, NaN, Inf, -Inf})
        rule(PBRT_COH_SLSC, false, [lp](pbrt_coherence_params &c) { c.lag_prop = lp; }, "lag_prop");
    rule(PBRT_COH_SLSC, true, [](pbrt_coherence_params &c) { c.lag_prop = std::numeric_limits<float>::denorm_min(); });
    rule(PBRT_COH_SLSC, true, [](pbrt_coherence_params &c) { c.lag_prop = std::nextafter(1.0f, 0.0f); });
    for (uint32_t H : {5u, 6u, 0xffffffffu}) rule(PBRT_COH_SLSC, false, [H](pbrt_coherence_params &c) { c.half_kernel = H; }, "half_kernel");
    for (float g : {-1.0f, 5.0f, NaN, Inf}) rule(PBRT_COH_SLSC, true, [g](pbrt_coherence_params &c) { c.gamma = g; });
    // CF
    for (float g : {-1e-6f, -1.0f, std::nextafter(4.0f, 5.0f), 5.0f, NaN, Inf, -Inf})
        rule(PBRT_COH_CF, false, [g](pbrt_coherence_params &c) { c.gamma = g; }, "gamma");
    rule(PBRT_COH_CF, true, [](pbrt_coherence_params &c) { c.gamma = std::nextafter(4.0f, 0.0f); });
    for (uint32_t H : {1u, 4u, 5u, 0xffffffffu}) rule(PBRT_COH_CF, false, [H](pbrt_coherence_params &c) { c.half_kernel = H; }, "half_kernel");
    for (float lp : {0.0f, -1.0f, 2.0f, NaN, Inf}) rule(PBRT_COH_CF, true, [lp](pbrt_coherence_params &c) { c.lag_prop = lp; });

    // ---- everything a pbrt_scan_params refuses: the same edit through both makers gives the same answer ----
    for (uint32_t kind : {(uint32_t)PBRT_COH_SLSC, (uint32_t)PBRT_COH_CF}) {
        const auto both = [&](auto edit) {
            pbrt_coherence_params c = valid(kind);
            edit(c.scan);
            CoherenceRequest r1;
            BfRequest r2;
            const char *w1 = coherence_request(&r1, &c), *w2 = bf_request(&r2, &c.scan);
            CHECK(refused(w2));
            CHECK(refused(w1) && std::strcmp(w1, w2) == 0);
        };
        both([](pbrt_scan_params &s) { s.probe = 2u; });
        for (float f : {-1.0f, NaN, Inf}) both([f](pbrt_scan_params &s) { s.demod_freq = f; });
        both([](pbrt_scan_params &s) { s.das.n_angles = 0; });
        both([](pbrt_scan_params &s) { s.das.n_elements = 0; });
        both([](pbrt_scan_params &s) { s.das.time_samples = 1; });
        both([](pbrt_scan_params &s) { s.das.fs = 0.0f; });
        both([](pbrt_scan_params &s) { s.das.fs = NaN; });
        both([](pbrt_scan_params &s) { s.das.sound_speed = 0.0f; });
        both([](pbrt_scan_params &s) { s.das.interpolation = 2u; });
        both([](pbrt_scan_params &s) { s.das.f_number = -1.0f; });
        both([](pbrt_scan_params &s) { s.das.f_number = NaN; });
        both([](pbrt_scan_params &s) { s.das.nx = 0; });
        both([](pbrt_scan_params &s) { s.das.nz = 0; });
        both([](pbrt_scan_params &s) { s.das.nx = 0x10000u, s.das.nz = 0x10000u; });
    }

    // ---- the lag rule: M = min(max(1, floor(lag_prop N)), N - 1, 64), 0 for N < 2 ----
    struct Row {
        uint32_t N, M30, M100, M10;
    };
    for (const Row r : {Row{0, 0, 0, 0}, Row{1, 0, 0, 0}, Row{2, 1, 1, 1}, Row{3, 1, 2, 1}, Row{10, 3, 9, 1}, Row{64, 19, 63, 6},
                        Row{65, 19, 64, 6}, Row{130, 39, 64, 13}, Row{256, 64, 64, 25}}) {
        CHECK(coherence_lags(r.N, 0.3f) == r.M30);
        CHECK(coherence_lags(r.N, 1.0f) == r.M100);
        CHECK(coherence_lags(r.N, 0.1f) == r.M10);
    }
    for (uint32_t N = 0; N <= COH_MAX_E; ++N)
        for (float lp : {std::numeric_limits<float>::denorm_min(), 1e-6f, 0.1f, 0.3f, 0.5f, 0.9999f, 1.0f}) {
            const uint32_t M = coherence_lags(N, lp);
            CHECK(M == lags_by_hand(N, lp));
            CHECK(N < 2u ? M == 0u : (M >= 1u && M <= N - 1u && M <= COH_MAX_LAG));
        }

    std::printf("{\"checks\": %d, \"failures\": %d}\n", checks, failures);
    return failures ? 1 : 0;
}
