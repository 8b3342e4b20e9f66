// Host check of the receive-window request in csrc/bf_request.h (tests/test_apod_restatement.py builds and runs it under the
// sanitizers): the maker of a pbrt_apod_params takes every window x every method and fills the request (method, pw, probe, tab, window,
// a0, alpha), refuses every single violation of the window's own rules (window >= 4, a Tukey alpha outside (0, 1] or not finite, a
// window without an f-number, tables > 1) and everything a pbrt_scan_params refuses; the four older makers yield a boxcar request.
// Prints one JSON line: {"checks": N, "failures": M}.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "bf_request.h"

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

static pbrt_das_params valid_das() {
    pbrt_das_params d;
    std::memset(&d, 0, sizeof d);
    d.n_angles = 2, d.n_elements = 3, d.time_samples = 16;
    d.fs = 5e6f, d.sound_speed = 1540.0f, d.t0 = 0.0f, d.f_number = 1.0f;
    d.interpolation = PBRT_DAS_LINEAR, d.compound_mean = 0, d.nx = 5, d.nz = 7;
    return d;
}
static pbrt_apod_params valid_apod(uint32_t window, uint32_t method) {
    pbrt_apod_params a;
    std::memset(&a, 0, sizeof a);
    a.scan = pbrt_scan_params{valid_das(), method, 3.0f, 2e6f, 0u};
    a.tables = 0u, a.window = window, a.alpha = 0.25f;
    return a;
}
static bool refused(const char *why) { return why != nullptr && why[0] != '\0'; }
static bool mentions(const char *why, const char *word) { return why != nullptr && std::strstr(why, word) != nullptr; }
static bool boxcar(const char *why, const BfRequest &rq) { return why == nullptr && rq.window == PBRT_APOD_BOXCAR; }

// one edit of a valid Hann request: taken, or refused
template <class Edit>
static void rule(bool taken, Edit edit, const char *word = nullptr) {
    pbrt_apod_params a = valid_apod(PBRT_APOD_HANN, PBRT_SCAN_DAS);
    edit(a);
    BfRequest rq;
    const char *why = bf_request(&rq, &a);
    CHECK(refused(why) == !taken);
    if (!taken && word) CHECK(mentions(why, word));
}

int main() {
    BfRequest rq;
    CHECK(PBRT_APOD_BOXCAR == 0u && PBRT_APOD_TUKEY == 1u && PBRT_APOD_HANN == 2u && PBRT_APOD_HAMMING == 3u);
    CHECK(sizeof(pbrt_apod_params) == sizeof(pbrt_scan_params) + 12u && sizeof(pbrt_scan_params) == 60u);

    // ---- every window x every method x both probes x both scan kinds -> the request as filled ----
    for (uint32_t window = 0; window <= 3u; ++window)
        for (uint32_t method = 0; method <= 3u; ++method)
            for (uint32_t probe = 0; probe <= 1u; ++probe)
                for (uint32_t tables = 0; tables <= 1u; ++tables) {
                    pbrt_apod_params a = valid_apod(window, method);
                    a.scan.probe = probe, a.tables = tables;
                    const char *why = bf_request(&rq, &a);
                    const float pw = method == PBRT_SCAN_IQ ? 2e6f : method == PBRT_SCAN_DAS ? 0.0f : 3.0f;
                    CHECK(why == nullptr);
                    CHECK(rq.das == &a.scan.das && rq.method == method && rq.pw == pw && rq.probe == (probe != 0) && rq.tab == (tables != 0));
                    CHECK(rq.window == window);
                    CHECK(rq.a0 == (window == PBRT_APOD_BOXCAR ? 1.0f : window == PBRT_APOD_HAMMING ? 0.54f : 0.5f));
                    CHECK(rq.alpha == (window == PBRT_APOD_TUKEY ? 0.25f : 1.0f));   // Hann is Tukey(1): the same launch arguments
                }
    {   // Tukey(1) and Hann differ in the window's number alone
        pbrt_apod_params t = valid_apod(PBRT_APOD_TUKEY, PBRT_SCAN_DAS), h = valid_apod(PBRT_APOD_HANN, PBRT_SCAN_DAS);
        t.alpha = 1.0f;
        BfRequest rt, rh;
        CHECK(bf_request(&rt, &t) == nullptr && bf_request(&rh, &h) == nullptr && rt.a0 == rh.a0 && rt.alpha == rh.alpha);
    }

    // ---- the window's own rules, one violation at a time ----
    CHECK(refused(bf_request(&rq, (const pbrt_apod_params *)nullptr)));
    rule(true, [](pbrt_apod_params &) {});
    for (uint32_t w : {4u, 5u, 0x80000000u, 0xffffffffu}) rule(false, [w](pbrt_apod_params &a) { a.window = w; }, "window");
    for (float al : {0.0f, -0.0f, -0.5f, 1.5f, NaN, Inf, -Inf})
        rule(false, [al](pbrt_apod_params &a) { a.window = PBRT_APOD_TUKEY, a.alpha = al; }, "alpha");
    for (float al : {1.0f, 0.5f, 1e-6f, std::nextafter(1.0f, 0.0f)})
        rule(true, [al](pbrt_apod_params &a) { a.window = PBRT_APOD_TUKEY, a.alpha = al; });
    rule(false, [](pbrt_apod_params &a) { a.window = PBRT_APOD_TUKEY, a.alpha = std::nextafter(1.0f, 2.0f); }, "alpha");
    // alpha is read by Tukey only
    for (uint32_t w : {PBRT_APOD_BOXCAR, PBRT_APOD_HANN, PBRT_APOD_HAMMING})
        for (float al : {0.0f, -0.5f, 1.5f, NaN, Inf}) rule(true, [w, al](pbrt_apod_params &a) { a.window = w, a.alpha = al; });
    // a window needs an aperture; boxcar does not
    for (uint32_t w : {PBRT_APOD_TUKEY, PBRT_APOD_HANN, PBRT_APOD_HAMMING})
        rule(false, [w](pbrt_apod_params &a) { a.window = w, a.scan.das.f_number = 0.0f; }, "f_number");
    rule(true, [](pbrt_apod_params &a) { a.window = PBRT_APOD_BOXCAR, a.scan.das.f_number = 0.0f; });
    rule(false, [](pbrt_apod_params &a) { a.scan.das.f_number = -1.0f; });
    rule(false, [](pbrt_apod_params &a) { a.scan.das.f_number = NaN; });
    for (uint32_t t : {2u, 3u, 0xffffffffu}) rule(false, [t](pbrt_apod_params &a) { a.tables = t; }, "tables");

    // ---- everything a pbrt_scan_params refuses: the same edit through both makers gives the same answer ----
    const auto both = [&](auto edit) {
        pbrt_apod_params a = valid_apod(PBRT_APOD_HAMMING, PBRT_SCAN_DAS);
        edit(a.scan);
        BfRequest r1, r2;
        const char *w1 = bf_request(&r1, &a), *w2 = bf_request(&r2, &a.scan);
        CHECK(refused(w2));
        CHECK(refused(w1) && std::strcmp(w1, w2) == 0);
    };
    both([](pbrt_scan_params &s) { s.method = 4u; });
    both([](pbrt_scan_params &s) { s.method = 0xffffffffu; });
    both([](pbrt_scan_params &s) { s.probe = 2u; });
    for (float p : {0.5f, 8.5f, NaN, Inf}) both([p](pbrt_scan_params &s) { s.method = PBRT_BF_PDAS, s.p = p; });
    for (float f : {-1.0f, NaN, Inf}) both([f](pbrt_scan_params &s) { s.method = PBRT_SCAN_IQ, s.demod_freq = f; });
    both([](pbrt_scan_params &s) { s.das.n_angles = 0; });
    both([](pbrt_scan_params &s) { s.das.n_elements = 0; });
    both([](pbrt_scan_params &s) { s.das.time_samples = 1; });
    both([](pbrt_scan_params &s) { s.das.fs = 0.0f; });
    both([](pbrt_scan_params &s) { s.das.fs = NaN; });
    both([](pbrt_scan_params &s) { s.das.sound_speed = 0.0f; });
    both([](pbrt_scan_params &s) { s.das.interpolation = 2u; });
    both([](pbrt_scan_params &s) { s.das.nx = 0; });
    both([](pbrt_scan_params &s) { s.das.nz = 0; });
    both([](pbrt_scan_params &s) { s.das.nx = 0x10000u, s.das.nz = 0x10000u; });
    // (p is read by p-DAS only, demod_freq by I/Q only: a window changes neither)
    rule(true, [](pbrt_apod_params &a) { a.scan.p = NaN, a.scan.demod_freq = NaN; });

    // ---- the four older makers yield a boxcar request ----
    const pbrt_das_params d = valid_das();
    pbrt_bf_params b{d, PBRT_BF_FDMAS, 2.0f, 0u};
    pbrt_iq_params q{d, 2e6f, 1u};
    pbrt_scan_params s{d, PBRT_BF_PDAS, 2.0f, 0.0f, 0u};
    std::memset(&rq, 0xff, sizeof rq);
    CHECK(boxcar(bf_request(&rq, &d, false), rq));
    std::memset(&rq, 0xff, sizeof rq);
    CHECK(boxcar(bf_request(&rq, &d, true), rq));
    std::memset(&rq, 0xff, sizeof rq);
    CHECK(boxcar(bf_request(&rq, &b), rq));
    std::memset(&rq, 0xff, sizeof rq);
    CHECK(boxcar(bf_request(&rq, &q), rq));
    std::memset(&rq, 0xff, sizeof rq);
    CHECK(boxcar(bf_request(&rq, &s), rq));

    std::printf("{\"checks\": %d, \"failures\": %d}\n", checks, failures);
    return failures ? 1 : 0;
}
