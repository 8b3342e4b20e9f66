// Host check of csrc/bf_request.h (tests/test_bf_request_host.py builds and runs it under the sanitizers): the four makers turn a
// valid parameter block into the request (method, pw, probe, tab) the launch reads, and refuse every single violation of the rules
// the entry points kept before the header existed -- those of a pbrt_das_params (counts, rates, interpolation, f-number, the pixel
// count and the launch grid), the methods each block admits, probe <= 1, 1 <= p <= 8 for p-DAS only, demod_freq finite and >= 0 for I/Q only.
// And the launch grid the host and the kernels share: over 12 x 12 scan sizes, axes and tables, the slots 0 .. blocks - 1 of das_grid give,
// through das_tile_of, every tile of the scan exactly once and nothing else.
// Prints one JSON line: {"checks": N, "failures": M}.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <vector>

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

// the request a maker gave: refused (with a text), or these four
static bool is(const char *why, const BfRequest &rq, const pbrt_das_params *das, uint32_t method, float pw, bool probe, bool tab) {
    return why == nullptr && rq.das == das && rq.method == method && rq.pw == pw && rq.probe == probe && rq.tab == tab;
}
static bool refused(const char *why) { return why != nullptr && why[0] != '\0'; }

// every maker on one das block: all take it, or all refuse it
template <class Edit>
static void das_rule(bool taken, Edit edit) {
    pbrt_das_params d = valid_das();
    edit(d);
    pbrt_bf_params b{d, PBRT_BF_FDMAS, 2.0f, 0u};
    pbrt_iq_params q{d, 2e6f, 0u};
    pbrt_scan_params s{d, PBRT_SCAN_DAS, 2.0f, 0.0f, 0u};
    BfRequest rq;
    CHECK(refused(bf_request(&rq, &d, false)) == !taken);
    CHECK(refused(bf_request(&rq, &d, true)) == !taken);
    CHECK(refused(bf_request(&rq, &b)) == !taken);
    CHECK(refused(bf_request(&rq, &q)) == !taken);
    CHECK(refused(bf_request(&rq, &s)) == !taken);
}

int main() {
    const pbrt_das_params d = valid_das();
    BfRequest rq;
    // ---- one numbering: the internal methods are the public constants ----
    CHECK(PBRT_SCAN_DAS == 0u && PBRT_BF_PDAS == 1u && PBRT_BF_FDMAS == 2u && PBRT_SCAN_IQ == 3u);
    CHECK(DAS_TILE == 8u && DAS_XCDS == 8u && DAS_BANDS == 16u);
    CHECK(das_tiles(1) == 1 && das_tiles(8) == 1 && das_tiles(9) == 2 && das_tiles(0xffffffffu) == 0x20000000u);

    // ---- valid blocks -> (method, pw, probe, tab) ----
    CHECK(is(bf_request(&rq, &d, false), rq, &d, PBRT_SCAN_DAS, 0.0f, false, false));
    CHECK(is(bf_request(&rq, &d, true), rq, &d, PBRT_SCAN_DAS, 0.0f, true, false));
    for (uint32_t probe = 0; probe <= 1; ++probe) {
        pbrt_bf_params b{d, PBRT_BF_PDAS, 3.0f, probe};
        CHECK(is(bf_request(&rq, &b), rq, &b.das, PBRT_BF_PDAS, 3.0f, probe != 0, false));
        b.method = PBRT_BF_FDMAS, b.p = 2.5f;   // (F-DMAS does not read p: it is handed on as it came)
        CHECK(is(bf_request(&rq, &b), rq, &b.das, PBRT_BF_FDMAS, 2.5f, probe != 0, false));
        pbrt_iq_params q{d, 2e6f, probe};
        CHECK(is(bf_request(&rq, &q), rq, &q.das, PBRT_SCAN_IQ, 2e6f, probe != 0, false));
        pbrt_scan_params s{d, PBRT_SCAN_DAS, 3.0f, 2e6f, probe};
        CHECK(is(bf_request(&rq, &s), rq, &s.das, PBRT_SCAN_DAS, 0.0f, probe != 0, true));
        s.method = PBRT_BF_PDAS;
        CHECK(is(bf_request(&rq, &s), rq, &s.das, PBRT_BF_PDAS, 3.0f, probe != 0, true));
        s.method = PBRT_BF_FDMAS;
        CHECK(is(bf_request(&rq, &s), rq, &s.das, PBRT_BF_FDMAS, 3.0f, probe != 0, true));
        s.method = PBRT_SCAN_IQ;
        CHECK(is(bf_request(&rq, &s), rq, &s.das, PBRT_SCAN_IQ, 2e6f, probe != 0, true));
    }

    // ---- no block at all ----
    CHECK(refused(bf_request(&rq, (const pbrt_das_params *)nullptr, false)));
    CHECK(refused(bf_request(&rq, (const pbrt_bf_params *)nullptr)));
    CHECK(refused(bf_request(&rq, (const pbrt_iq_params *)nullptr)));
    CHECK(refused(bf_request(&rq, (const pbrt_scan_params *)nullptr)));

    // ---- the rules of a pbrt_das_params, one violation at a time, through every maker ----
    das_rule(true, [](pbrt_das_params &) {});
    das_rule(false, [](pbrt_das_params &p) { p.n_angles = 0; });
    das_rule(false, [](pbrt_das_params &p) { p.n_elements = 0; });
    das_rule(false, [](pbrt_das_params &p) { p.time_samples = 1; });
    das_rule(true, [](pbrt_das_params &p) { p.time_samples = 2; });
    das_rule(false, [](pbrt_das_params &p) { p.fs = 0.0f; });
    das_rule(false, [](pbrt_das_params &p) { p.fs = NaN; });
    das_rule(false, [](pbrt_das_params &p) { p.sound_speed = 0.0f; });
    das_rule(false, [](pbrt_das_params &p) { p.sound_speed = -1540.0f; });
    das_rule(false, [](pbrt_das_params &p) { p.interpolation = 2; });
    das_rule(true, [](pbrt_das_params &p) { p.interpolation = PBRT_DAS_NEAREST; });
    das_rule(false, [](pbrt_das_params &p) { p.f_number = -1.0f; });
    das_rule(false, [](pbrt_das_params &p) { p.f_number = NaN; });
    das_rule(true, [](pbrt_das_params &p) { p.f_number = 0.0f; });
    das_rule(true, [](pbrt_das_params &p) { p.t0 = -1e-6f, p.compound_mean = 1; });
    das_rule(false, [](pbrt_das_params &p) { p.nx = 0; });
    das_rule(false, [](pbrt_das_params &p) { p.nz = 0; });
    // the pixel count: nx * nz < 2^32 - 1
    das_rule(false, [](pbrt_das_params &p) { p.nx = 65536, p.nz = 65536; });
    das_rule(false, [](pbrt_das_params &p) { p.nx = 65537, p.nz = 65535; });   // 2^32 - 1 itself
    das_rule(true, [](pbrt_das_params &p) { p.nx = 65535, p.nz = 65536; });
    // the launch grid: tiles(nx) * (tiles(nz) + 16) * 8 < 2^31 - 1
    das_rule(false, [](pbrt_das_params &p) { p.nx = 0x7fffffffu, p.nz = 1; });             // 2^28 * 17 * 8
    das_rule(false, [](pbrt_das_params &p) { p.nx = 8u * 15790321u, p.nz = 1; });          // 15790321 * 136 = 2^31 + 8
    das_rule(true, [](pbrt_das_params &p) { p.nx = 8u * 15790320u, p.nz = 1; });           // 15790320 * 136 = 2^31 - 128
    das_rule(false, [](pbrt_das_params &p) { p.nx = 1, p.nz = 8u * 268435440u; });         // (268435440 + 16) * 8 = 2^31
    das_rule(true, [](pbrt_das_params &p) { p.nx = 1, p.nz = 8u * 268435439u; });          // (268435439 + 16) * 8 = 2^31 - 8

    // ---- the methods each block admits ----
    for (uint32_t m = 0; m <= 5; ++m) {
        pbrt_bf_params b{d, m, 2.0f, 0u};
        CHECK(refused(bf_request(&rq, &b)) == !(m == PBRT_BF_PDAS || m == PBRT_BF_FDMAS));   // (0 and 3: plain and I/Q have their own calls)
        pbrt_scan_params s{d, m, 2.0f, 0.0f, 0u};
        CHECK(refused(bf_request(&rq, &s)) == (m >= 4));
    }
    {
        pbrt_scan_params s{d, 0xffffffffu, 2.0f, 0.0f, 0u};
        CHECK(refused(bf_request(&rq, &s)));
    }

    // ---- probe <= 1 ----
    for (uint32_t probe : {2u, 0x100u, 0xffffffffu}) {
        pbrt_bf_params b{d, PBRT_BF_FDMAS, 2.0f, probe};
        pbrt_iq_params q{d, 2e6f, probe};
        pbrt_scan_params s{d, PBRT_SCAN_DAS, 2.0f, 0.0f, probe};
        CHECK(refused(bf_request(&rq, &b)) && refused(bf_request(&rq, &q)) && refused(bf_request(&rq, &s)));
    }

    // ---- p: checked for p-DAS only ----
    for (float p : {NaN, Inf, 0.5f, 8.5f, -2.0f, 0.0f}) {
        pbrt_bf_params b{d, PBRT_BF_PDAS, p, 0u};
        CHECK(refused(bf_request(&rq, &b)));
        b.method = PBRT_BF_FDMAS;
        CHECK(!refused(bf_request(&rq, &b)) && rq.method == PBRT_BF_FDMAS);
        pbrt_scan_params s{d, PBRT_BF_PDAS, p, 0.0f, 0u};
        CHECK(refused(bf_request(&rq, &s)));
        for (uint32_t m : {PBRT_SCAN_DAS, PBRT_BF_FDMAS, PBRT_SCAN_IQ}) {
            s.method = m;
            CHECK(!refused(bf_request(&rq, &s)) && rq.method == m);
        }
    }
    for (float p : {1.0f, 1.5f, 8.0f}) {
        pbrt_bf_params b{d, PBRT_BF_PDAS, p, 0u};
        CHECK(is(bf_request(&rq, &b), rq, &b.das, PBRT_BF_PDAS, p, false, false));
    }

    // ---- demod_freq: checked for I/Q only; -0.0 is taken ----
    for (float f : {NaN, Inf, -Inf, -1.0f}) {
        pbrt_iq_params q{d, f, 0u};
        CHECK(refused(bf_request(&rq, &q)));
        pbrt_scan_params s{d, PBRT_SCAN_IQ, 2.0f, f, 0u};
        CHECK(refused(bf_request(&rq, &s)));
        for (uint32_t m : {PBRT_SCAN_DAS, PBRT_BF_PDAS, PBRT_BF_FDMAS}) {
            s.method = m;
            CHECK(!refused(bf_request(&rq, &s)) && rq.method == m && rq.pw == (m == PBRT_SCAN_DAS ? 0.0f : 2.0f));
        }
    }
    for (float f : {-0.0f, 0.0f, 2e6f}) {
        pbrt_iq_params q{d, f, 1u};
        CHECK(is(bf_request(&rq, &q), rq, &q.das, PBRT_SCAN_IQ, f, true, false));
        pbrt_scan_params s{d, PBRT_SCAN_IQ, NaN, f, 0u};   // (p is not read)
        CHECK(is(bf_request(&rq, &s), rq, &s.das, PBRT_SCAN_IQ, f, false, true));
    }

    // ---- the launch grid: das_grid's slots, walked through das_tile_of as the kernels walk them, hand every tile out exactly once ----
    const uint32_t sizes[] = {1, 7, 8, 9, 64, 121, 127, 128, 129, 135, 1040, 2547};  // 1, 2, 8, 9, 16, 17 tiles ... and the bench shape
    for (uint32_t nx : sizes)
        for (uint32_t nz : sizes)
            for (uint32_t tab = 0; tab <= 1; ++tab) {
                DasGrid g;
                const uint32_t blocks = das_grid(&g, nx, nz, tab != 0);
                CHECK(g.ntx == das_tiles(nx) && g.ntz == das_tiles(nz) && g.tab == tab && g.m >= 1 && g.m <= g.ntz);
                CHECK(blocks == DAS_XCDS * g.ntx * g.m);
                std::vector<uint8_t> given((size_t)g.ntx * g.ntz, 0);
                uint32_t taken = 0, outside = 0, twice = 0;
                for (uint32_t b = 0; b < blocks; ++b) {
                    uint32_t tx = 0, tz = 0;
                    if (!das_tile_of(g, b, &tx, &tz)) continue;
                    ++taken;
                    if (tx >= g.ntx || tz >= g.ntz) {
                        ++outside;
                    } else if (given[(size_t)tx * g.ntz + tz]++) {
                        ++twice;
                    }
                }
                // (every slot that is taken names a tile of the scan, no tile twice, and as many as there are tiles: each exactly once,
                // and every other slot is refused)
                CHECK(outside == 0 && twice == 0 && taken == g.ntx * g.ntz);
            }

    std::printf("{\"checks\": %d, \"failures\": %d}\n", checks, failures);
    return failures ? 1 : 0;
}
