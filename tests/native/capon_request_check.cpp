// Host check of the Capon request in csrc/capon_request.h (tests/test_capon_request_host.py builds and runs it under the sanitizers):
// the maker of a pbrt_capon_params takes every valid block and fills the request (the I/Q request of bf_request, l_prop, delta_l),
// refuses every single violation of the method's own rules (a method other than PBRT_SCAN_IQ, tables > 1, l_prop not finite or outside
// [0, 0.5], delta_l not finite, <= 0 or > 1e3, more than CAPON_MAX_E elements) and everything a pbrt_scan_params refuses; and the
// subarray rule capon_lm, which the host and the kernel share, on its table.  Prints one JSON line: {"checks": N, "failures": M}.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "capon_request.h"

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

static pbrt_capon_params valid_capon() {
    pbrt_capon_params c;
    std::memset(&c, 0, sizeof c);
    pbrt_das_params &d = c.scan.das;
    d.n_angles = 2, d.n_elements = 64, d.time_samples = 16;
    d.fs = 5e6f, d.sound_speed = 1540.0f, d.t0 = 0.0f, d.f_number = 1.0f;
    d.interpolation = PBRT_DAS_LINEAR, d.compound_mean = 0, d.nx = 5, d.nz = 7;
    c.scan.method = PBRT_SCAN_IQ, c.scan.p = 2.0f, c.scan.demod_freq = 2e6f, c.scan.probe = 0u;
    c.tables = 0u, c.l_prop = 0.5f, c.delta_l = 0.01f;
    return c;
}
static bool refused(const char *why) { return why != nullptr && why[0] != '\0'; }
static bool mentions(const char *why, const char *word) { return why != nullptr && std::strstr(why, word) != nullptr; }

// one edit of a valid request: taken, or refused (with a rule text that names `word`)
template <class Edit>
static void rule(bool taken, Edit edit, const char *word = nullptr) {
    pbrt_capon_params c = valid_capon();
    edit(c);
    CaponRequest rq;
    const char *why = capon_request(&rq, &c);
    CHECK(refused(why) == !taken);
    if (!taken && word) CHECK(mentions(why, word));
}

int main() {
    CHECK(CAPON_MAX_L == 32u && CAPON_MAX_E == 256u);
    CHECK(sizeof(pbrt_capon_params) == sizeof(pbrt_scan_params) + 12u && sizeof(pbrt_capon_params) == sizeof(pbrt_apod_params));

    // ---- every valid block: both probes x both scan kinds x both interpolations x settings -> the request as filled ----
    for (uint32_t probe = 0; probe <= 1u; ++probe)
        for (uint32_t tables = 0; tables <= 1u; ++tables)
            for (uint32_t interp = 0; interp <= 1u; ++interp)
                for (float lp : {0.0f, -0.0f, 0.25f, 0.5f, 1e-6f})
                    for (float dl : {0.01f, 1e-6f, 1.0f, 1e3f}) {
                        pbrt_capon_params c = valid_capon();
                        c.scan.probe = probe, c.tables = tables, c.scan.das.interpolation = interp, c.l_prop = lp, c.delta_l = dl;
                        CaponRequest rq;
                        std::memset(&rq, 0xff, sizeof rq);
                        const char *why = capon_request(&rq, &c);
                        CHECK(why == nullptr);
                        CHECK(rq.bf.das == &c.scan.das && rq.bf.method == PBRT_SCAN_IQ && rq.bf.pw == 2e6f);
                        CHECK(rq.bf.probe == (probe != 0) && rq.bf.tab == (tables != 0) && rq.bf.window == PBRT_APOD_BOXCAR);
                        CHECK(rq.l_prop == lp && rq.delta_l == dl);
                    }
    for (uint32_t e : {1u, 3u, 255u, 256u}) rule(true, [e](pbrt_capon_params &c) { c.scan.das.n_elements = e; });
    rule(true, [](pbrt_capon_params &c) { c.scan.das.f_number = 0.0f; });
    rule(true, [](pbrt_capon_params &c) { c.scan.p = NaN; });  // (p is read by p-DAS only)

    // ---- the method's own rules, one violation at a time ----
    CHECK(refused(capon_request(nullptr, nullptr)));
    rule(true, [](pbrt_capon_params &) {});
    for (uint32_t m : {(uint32_t)PBRT_SCAN_DAS, (uint32_t)PBRT_BF_PDAS, (uint32_t)PBRT_BF_FDMAS, 4u, 0xffffffffu})
        rule(false, [m](pbrt_capon_params &c) { c.scan.method = m; }, "method");
    for (uint32_t t : {2u, 3u, 0xffffffffu}) rule(false, [t](pbrt_capon_params &c) { c.tables = t; }, "tables");
    for (float lp : {-1e-6f, -0.5f, std::nextafter(0.5f, 1.0f), 0.75f, 1.0f, NaN, Inf, -Inf})
        rule(false, [lp](pbrt_capon_params &c) { c.l_prop = lp; }, "l_prop");
    rule(true, [](pbrt_capon_params &c) { c.l_prop = std::nextafter(0.5f, 0.0f); });
    for (float dl : {0.0f, -0.0f, -0.01f, std::nextafter(1e3f, 2e3f), 1e4f, NaN, Inf, -Inf})
        rule(false, [dl](pbrt_capon_params &c) { c.delta_l = dl; }, "delta_l");
    rule(true, [](pbrt_capon_params &c) { c.delta_l = std::numeric_limits<float>::denorm_min(); });
    for (uint32_t e : {257u, 512u, 0xffffffffu}) rule(false, [e](pbrt_capon_params &c) { c.scan.das.n_elements = e; }, "n_elements");

    // ---- everything a pbrt_scan_params refuses: the same edit through both makers gives the same answer ----
    const auto both = [&](auto edit) {
        pbrt_capon_params c = valid_capon();
        edit(c.scan);
        CaponRequest r1;
        BfRequest r2;
        const char *w1 = capon_request(&r1, &c), *w2 = bf_request(&r2, &c.scan);
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

    // ---- the subarray rule: L = min(max(1, floor(l_prop N)), 32), M = N - L + 1 ----
    struct Row {
        uint32_t N, L50, L25;
    };
    for (const Row r : {Row{0, 1, 1}, Row{1, 1, 1}, Row{2, 1, 1}, Row{3, 1, 1}, Row{63, 31, 15}, Row{64, 32, 16}, Row{65, 32, 16},
                        Row{130, 32, 32}, Row{256, 32, 32}}) {
        const CaponLM a = capon_lm(r.N, 0.5f), b = capon_lm(r.N, 0.25f), z = capon_lm(r.N, 0.0f), nz = capon_lm(r.N, -0.0f);
        CHECK(a.L == r.L50 && a.M == (r.N ? r.N - r.L50 + 1u : 0u));
        CHECK(b.L == r.L25 && b.M == (r.N ? r.N - r.L25 + 1u : 0u));
        CHECK(z.L == 1u && z.M == r.N && nz.L == 1u && nz.M == r.N);
    }
    for (uint32_t N = 0; N <= CAPON_MAX_E; ++N)
        for (float lp : {0.0f, 0.1f, 0.25f, 0.4999f, 0.5f}) {
            const CaponLM v = capon_lm(N, lp);
            CHECK(v.L >= 1u && v.L <= CAPON_MAX_L && (N == 0u ? v.M == 0u : (v.L <= N && v.M + v.L == N + 1u)));
        }

    std::printf("{\"checks\": %d, \"failures\": %d}\n", checks, failures);
    return failures ? 1 : 0;
}
