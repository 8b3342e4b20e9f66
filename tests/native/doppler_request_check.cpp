// Host check of the Doppler requests in csrc/doppler_request.h (tests/test_doppler_request_host.py builds and runs it under the
// sanitizers): the two makers take every valid block and fill the request; every rule refuses its case and accepts the neighbouring
// boundary (null pointers, n_frames outside [2, 64], wall_degree > 3 or + 1 >= n_frames, a missing basis, kx / kz even or outside
// [1, 15], an unknown window, nyquist_velocity not finite or <= 0, sizes outside 32 bits, input and output overlapping); `empty` is
// "no pixel"; the launch shapes equal literals worked out by hand; a sweep over the admitted ranges keeps grid, block and LDS within
// what a launch may ask for; and the smoothing weights are normalised, symmetric and positive.  Prints one JSON line:
// {"checks": N, "failures": M}.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "doppler_request.h"

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
static bool refused(const char *why) { return why != nullptr && why[0] != '\0'; }
static bool mentions(const char *why, const char *word) { return why != nullptr && std::strstr(why, word) != nullptr; }

// pointers that are never read: far apart, so that nothing of a valid request overlaps
static char *const FRAMES = reinterpret_cast<char *>(uintptr_t(1) << 40), *const Q = reinterpret_cast<char *>(uintptr_t(2) << 40),
                  *const ACF = reinterpret_cast<char *>(uintptr_t(3) << 40), *const VEL = reinterpret_cast<char *>(uintptr_t(4) << 40),
                  *const AMP = reinterpret_cast<char *>(uintptr_t(5) << 40);

static pbrt_doppler_params valid() {
    pbrt_doppler_params p;
    std::memset(&p, 0, sizeof p);
    p.n_frames = 8, p.nx = 13, p.nz = 37, p.wall_degree = 1, p.kx = 3, p.kz = 5, p.window = PBRT_DOPPLER_HAMMING, p.nyquist_velocity = 0.3f;
    return p;
}
template <class Edit>
static void acf_rule(bool taken, Edit edit, const char *word = nullptr) {
    pbrt_doppler_params p = valid();
    const void *frames = FRAMES, *q = Q, *acf = ACF;
    edit(p, frames, q, acf);
    DopplerAcfRequest rq;
    const char *why = doppler_acf_request(&rq, &p, frames, q, acf);
    CHECK(refused(why) == !taken);
    if (!taken && word) CHECK(mentions(why, word));
}
template <class Edit>
static void maps_rule(bool taken, Edit edit, const char *word = nullptr) {
    pbrt_doppler_params p = valid();
    const void *acf = ACF, *vel = VEL, *amp = AMP;
    edit(p, acf, vel, amp);
    DopplerMapsRequest rq;
    const char *why = doppler_maps_request(&rq, &p, acf, vel, amp);
    CHECK(refused(why) == !taken);
    if (!taken && word) CHECK(mentions(why, word));
}
#define ACF_EDIT [=](pbrt_doppler_params &p, const void *&frames, const void *&q, const void *&acf)
#define MAPS_EDIT [=](pbrt_doppler_params &p, const void *&acf, const void *&vel, const void *&amp)
#define UNUSED3(a, b, c) (void)a, (void)b, (void)c

int main() {
    CHECK(sizeof(pbrt_doppler_params) == 32u);
    CHECK(DOPPLER_MAX_FRAMES == 64u && DOPPLER_MAX_DEGREE == 3u && DOPPLER_MAX_K == 15u && DOPPLER_TILE_X * DOPPLER_TILE_Z == 256u);

    // ---- the autocorrelation: every rule, its case and the neighbouring boundary ----
    acf_rule(true, ACF_EDIT { UNUSED3(frames, q, acf); (void)p; });
    {
        DopplerAcfRequest rq;
        CHECK(refused(doppler_acf_request(&rq, nullptr, FRAMES, Q, ACF)));
    }
    acf_rule(false, ACF_EDIT { UNUSED3(p, q, acf); frames = nullptr; }, "frames");
    acf_rule(false, ACF_EDIT { UNUSED3(p, q, frames); acf = nullptr; }, "acf");
    for (uint32_t n : {0u, 1u, 65u, 0xffffffffu}) acf_rule(false, ACF_EDIT { UNUSED3(frames, q, acf); p.n_frames = n; p.wall_degree = PBRT_DOPPLER_WALL_NONE; }, "n_frames");
    for (uint32_t n : {2u, 3u, 63u, 64u}) acf_rule(true, ACF_EDIT { UNUSED3(frames, q, acf); p.n_frames = n; p.wall_degree = PBRT_DOPPLER_WALL_NONE; });
    for (uint32_t d : {4u, 5u, 0xfffffffeu}) acf_rule(false, ACF_EDIT { UNUSED3(frames, q, acf); p.n_frames = 64; p.wall_degree = d; }, "wall_degree");
    for (uint32_t d : {0u, 1u, 2u, 3u, PBRT_DOPPLER_WALL_NONE}) acf_rule(true, ACF_EDIT { UNUSED3(frames, q, acf); p.n_frames = 64; p.wall_degree = d; });
    // wall_degree + 1 < n_frames: (N, d) taken iff d <= N - 2
    for (uint32_t N = 2; N <= 6; ++N)
        for (uint32_t d = 0; d <= 3; ++d) acf_rule(d + 2 <= N, ACF_EDIT { UNUSED3(frames, q, acf); p.n_frames = N; p.wall_degree = d; }, "n_frames");
    acf_rule(false, ACF_EDIT { UNUSED3(p, frames, acf); q = nullptr; }, "q");
    acf_rule(true, ACF_EDIT { UNUSED3(frames, acf, q); q = nullptr; p.wall_degree = PBRT_DOPPLER_WALL_NONE; });
    // sizes: nx nz and n_frames nx nz below 2^32 - 1
    acf_rule(false, ACF_EDIT { UNUSED3(frames, q, acf); p.nx = 0x10000u, p.nz = 0x10000u; p.n_frames = 2; p.wall_degree = 0; }, "0xffffffff");
    acf_rule(false, ACF_EDIT { UNUSED3(frames, q, acf); p.nx = 0xffffffffu, p.nz = 1u; p.n_frames = 2; p.wall_degree = 0; }, "0xffffffff");
    acf_rule(false, ACF_EDIT { UNUSED3(frames, q, acf); p.nx = 0x4000000u, p.nz = 1u; p.n_frames = 64; }, "0xffffffff");        // 2^26 * 64 = 2^32
    acf_rule(true, ACF_EDIT { UNUSED3(frames, q, acf); p.nx = 0x4000000u - 1u, p.nz = 1u; p.n_frames = 64; });                   // 2^32 - 64
    acf_rule(true, ACF_EDIT { UNUSED3(frames, q, acf); p.nx = 0x7fffffffu, p.nz = 1u; p.n_frames = 2; p.wall_degree = 0; });     // 2^32 - 2
    acf_rule(false, ACF_EDIT { UNUSED3(frames, q, acf); p.nx = 0x80000000u, p.nz = 1u; p.n_frames = 2; p.wall_degree = 0; }, "0xffffffff");
    // overlap: frames [N P 8 bytes) and q [(d + 1) N 4 bytes) against acf [P 12 bytes)
    {
        const size_t P = 13 * 37, nf = 8 * P * 8, na = P * 12, nq = 2 * 8 * 4;
        acf_rule(false, ACF_EDIT { UNUSED3(p, frames, q); acf = FRAMES; }, "overlap");
        acf_rule(false, ACF_EDIT { UNUSED3(p, frames, q); acf = FRAMES + nf - 1; }, "overlap");
        acf_rule(true, ACF_EDIT { UNUSED3(p, frames, q); acf = FRAMES + nf; });
        acf_rule(false, ACF_EDIT { UNUSED3(p, frames, q); acf = FRAMES - na + 1; }, "overlap");
        acf_rule(true, ACF_EDIT { UNUSED3(p, frames, q); acf = FRAMES - na; });
        acf_rule(false, ACF_EDIT { UNUSED3(p, frames, q); acf = Q + nq - 1; }, "overlap");
        acf_rule(true, ACF_EDIT { UNUSED3(p, frames, q); acf = Q + nq; });
        acf_rule(false, ACF_EDIT { UNUSED3(p, frames, q); acf = Q - na + 1; }, "overlap");
        acf_rule(true, ACF_EDIT { UNUSED3(p, frames, q); acf = Q - na; });
        acf_rule(true, ACF_EDIT { UNUSED3(frames, q, acf); q = ACF; p.wall_degree = PBRT_DOPPLER_WALL_NONE; });   // (q is not read)
    }
    // the fields of the other step are not read
    acf_rule(true, ACF_EDIT { UNUSED3(frames, q, acf); p.kx = 2, p.kz = 0, p.window = 9, p.nyquist_velocity = NaN; });

    // the request as filled, `empty`, and launch shapes worked out by hand
    {
        pbrt_doppler_params p = valid();
        DopplerAcfRequest rq;
        std::memset(&rq, 0xff, sizeof rq);
        CHECK(doppler_acf_request(&rq, &p, FRAMES, Q, ACF) == nullptr);
        CHECK(!rq.empty && rq.N == 8u && rq.P == 481u && rq.n_coef == 2u);
        CHECK(rq.launch.gx == 2u && rq.launch.gy == 1u && rq.launch.block == 256u && rq.launch.lds == 0u);   // 481 pixels: two workgroups
        p.wall_degree = PBRT_DOPPLER_WALL_NONE;
        CHECK(doppler_acf_request(&rq, &p, FRAMES, nullptr, ACF) == nullptr && rq.n_coef == 0u);
        p.nx = 1, p.nz = 256;
        CHECK(doppler_acf_request(&rq, &p, FRAMES, nullptr, ACF) == nullptr && rq.launch.gx == 1u && rq.P == 256u);
        p.nz = 257;
        CHECK(doppler_acf_request(&rq, &p, FRAMES, nullptr, ACF) == nullptr && rq.launch.gx == 2u);
        p.nx = 1040, p.nz = 638;
        CHECK(doppler_acf_request(&rq, &p, FRAMES, nullptr, ACF) == nullptr && rq.P == 663520u && rq.launch.gx == 2592u);   // 663520 / 256 = 2591.9
        p.nx = 0, p.nz = 638;
        CHECK(doppler_acf_request(&rq, &p, FRAMES, nullptr, ACF) == nullptr && rq.empty);
        p.nx = 5, p.nz = 0;
        CHECK(doppler_acf_request(&rq, &p, FRAMES, nullptr, ACF) == nullptr && rq.empty);
    }

    // ---- the maps ----
    maps_rule(true, MAPS_EDIT { UNUSED3(acf, vel, amp); (void)p; });
    {
        DopplerMapsRequest rq;
        CHECK(refused(doppler_maps_request(&rq, nullptr, ACF, VEL, AMP)));
    }
    maps_rule(false, MAPS_EDIT { UNUSED3(p, vel, amp); acf = nullptr; }, "acf");
    maps_rule(false, MAPS_EDIT { UNUSED3(p, acf, amp); vel = nullptr; }, "velocity");
    maps_rule(false, MAPS_EDIT { UNUSED3(p, acf, vel); amp = nullptr; }, "amplitude");
    for (uint32_t k : {0u, 2u, 4u, 14u, 16u, 17u, 0xffffffffu}) {
        maps_rule(false, MAPS_EDIT { UNUSED3(acf, vel, amp); p.kx = k; }, "kx");
        maps_rule(false, MAPS_EDIT { UNUSED3(acf, vel, amp); p.kz = k; }, "kz");
    }
    for (uint32_t k : {1u, 3u, 13u, 15u}) {
        maps_rule(true, MAPS_EDIT { UNUSED3(acf, vel, amp); p.kx = k; });
        maps_rule(true, MAPS_EDIT { UNUSED3(acf, vel, amp); p.kz = k; });
    }
    for (uint32_t w : {2u, 3u, 0xffffffffu}) maps_rule(false, MAPS_EDIT { UNUSED3(acf, vel, amp); p.window = w; }, "window");
    for (uint32_t w : {(uint32_t)PBRT_DOPPLER_BOXCAR, (uint32_t)PBRT_DOPPLER_HAMMING}) maps_rule(true, MAPS_EDIT { UNUSED3(acf, vel, amp); p.window = w; });
    for (float v : {0.0f, -0.0f, -1.0f, NaN, Inf, -Inf}) maps_rule(false, MAPS_EDIT { UNUSED3(acf, vel, amp); p.nyquist_velocity = v; }, "nyquist_velocity");
    for (float v : {std::numeric_limits<float>::denorm_min(), 1e-3f, std::numeric_limits<float>::max()})
        maps_rule(true, MAPS_EDIT { UNUSED3(acf, vel, amp); p.nyquist_velocity = v; });
    maps_rule(false, MAPS_EDIT { UNUSED3(acf, vel, amp); p.nx = 0x10000u, p.nz = 0x10000u; }, "0xffffffff");
    maps_rule(false, MAPS_EDIT { UNUSED3(acf, vel, amp); p.nx = 0xffffffffu, p.nz = 1u; }, "0xffffffff");
    maps_rule(true, MAPS_EDIT { UNUSED3(acf, vel, amp); p.nx = 0xfffffffeu, p.nz = 1u; });
    maps_rule(true, MAPS_EDIT { UNUSED3(acf, vel, amp); p.nx = 1u, p.nz = 0xfffffffeu; });
    {
        const size_t P = 13 * 37;
        maps_rule(false, MAPS_EDIT { UNUSED3(p, acf, amp); vel = ACF + 12 * P - 1; }, "overlap");
        maps_rule(true, MAPS_EDIT { UNUSED3(p, acf, amp); vel = ACF + 12 * P; });
        maps_rule(false, MAPS_EDIT { UNUSED3(p, acf, amp); vel = ACF - 4 * P + 1; }, "overlap");
        maps_rule(true, MAPS_EDIT { UNUSED3(p, acf, amp); vel = ACF - 4 * P; });
        maps_rule(false, MAPS_EDIT { UNUSED3(p, acf, vel); amp = ACF + 4 * P; }, "overlap");     // the second plane
        maps_rule(true, MAPS_EDIT { UNUSED3(p, acf, vel); amp = ACF + 12 * P; });
        maps_rule(false, MAPS_EDIT { UNUSED3(p, acf, vel); amp = VEL; }, "overlap");
        maps_rule(false, MAPS_EDIT { UNUSED3(p, acf, vel); amp = VEL + 4 * P - 1; }, "overlap");
        maps_rule(true, MAPS_EDIT { UNUSED3(p, acf, vel); amp = VEL + 4 * P; });
    }
    maps_rule(true, MAPS_EDIT { UNUSED3(acf, vel, amp); p.n_frames = 0, p.wall_degree = 77; });   // (the other step's fields are not read)
    {
        pbrt_doppler_params p = valid();
        DopplerMapsRequest rq;
        std::memset(&rq, 0xff, sizeof rq);
        CHECK(doppler_maps_request(&rq, &p, ACF, VEL, AMP) == nullptr);
        CHECK(!rq.empty && rq.nx == 13u && rq.nz == 37u && rq.kx == 3u && rq.kz == 5u && rq.tiles_z == 2u);
        CHECK(rq.launch.gx == 4u && rq.launch.gy == 1u && rq.launch.block == 256u);             // 2 tiles of 8 rows x 2 tiles of 32 columns
        CHECK(rq.launch.lds == (3u * 10u * 36u + 3u * 10u * 32u + 32u) * 4u);                 // 10 x 36 staged, 10 x 32 smoothed, 32 weights: 8288
        CHECK(rq.launch.lds == 8288u);
        CHECK(std::fabs(rq.scale - 0.3f / 3.14159265f) <= 1e-8f);
        p.kx = p.kz = 15;
        CHECK(doppler_maps_request(&rq, &p, ACF, VEL, AMP) == nullptr && rq.launch.lds == 20720u);   // (3 * 22 * 46 + 3 * 22 * 32 + 32) * 4
        p.kx = p.kz = 1;
        CHECK(doppler_maps_request(&rq, &p, ACF, VEL, AMP) == nullptr && rq.launch.lds == 6272u);    // (3 * 8 * 32 * 2 + 32) * 4
        CHECK(rq.w.wx[0] == 1.0f && rq.w.wz[0] == 1.0f && rq.w.wx[1] == 0.0f && rq.w.wz[14] == 0.0f);
        p.nx = 1040, p.nz = 638;
        CHECK(doppler_maps_request(&rq, &p, ACF, VEL, AMP) == nullptr && rq.tiles_z == 20u && rq.launch.gx == 130u * 20u);
        p.nx = 8, p.nz = 32;
        CHECK(doppler_maps_request(&rq, &p, ACF, VEL, AMP) == nullptr && rq.launch.gx == 1u);
        p.nx = 9, p.nz = 33;
        CHECK(doppler_maps_request(&rq, &p, ACF, VEL, AMP) == nullptr && rq.launch.gx == 4u);
        p.nx = 0;
        CHECK(doppler_maps_request(&rq, &p, ACF, VEL, AMP) == nullptr && rq.empty);
        p.nx = 3, p.nz = 0;
        CHECK(doppler_maps_request(&rq, &p, ACF, VEL, AMP) == nullptr && rq.empty);
    }

    // ---- the weights: normalised, symmetric, positive; the boxcar 1 / k, the Hamming ends 0.08 of its middle ----
    for (uint32_t window : {(uint32_t)PBRT_DOPPLER_BOXCAR, (uint32_t)PBRT_DOPPLER_HAMMING})
        for (uint32_t k = 1; k <= DOPPLER_MAX_K; k += 2) {
            float w[DOPPLER_MAX_K];
            doppler_window(window, k, w);
            double sum = 0.0;
            for (uint32_t i = 0; i < DOPPLER_MAX_K; ++i) {
                sum += w[i];
                CHECK(i < k ? (w[i] > 0.0f && w[i] == w[k - 1 - i]) : w[i] == 0.0f);
                if (window == PBRT_DOPPLER_BOXCAR && i < k) CHECK(w[i] == (float)(1.0 / k));
            }
            CHECK(std::fabs(sum - 1.0) <= 4.0 * 5.96e-8);
            if (window == PBRT_DOPPLER_HAMMING && k > 1) CHECK(std::fabs(w[0] / w[k / 2] - 0.08) <= 1e-6);
        }

    // ---- a sweep over the admitted ranges: grid, block and LDS stay within what a launch may ask for ----
    for (uint32_t nx : {1u, 7u, 8u, 9u, 1040u, 65536u, 0x7fffffu})
        for (uint32_t nz : {1u, 31u, 32u, 33u, 638u, 4096u, 511u}) {
            if ((uint64_t)nx * nz * 2u >= 0xffffffffull) continue;
            for (uint32_t N : {2u, 8u, 64u}) {
                if ((uint64_t)nx * nz * N >= 0xffffffffull) continue;
                for (uint32_t d : {0u, 3u, PBRT_DOPPLER_WALL_NONE}) {
                    if (d != PBRT_DOPPLER_WALL_NONE && d + 1 >= N) continue;
                    pbrt_doppler_params p = valid();
                    p.nx = nx, p.nz = nz, p.n_frames = N, p.wall_degree = d;
                    DopplerAcfRequest rq;
                    CHECK(doppler_acf_request(&rq, &p, FRAMES, Q, ACF) == nullptr);
                    CHECK(rq.launch.gx >= 1u && rq.launch.gx <= 0x7fffffffu && rq.launch.gy == 1u && rq.launch.block == 256u && rq.launch.lds == 0u);
                    CHECK((uint64_t)rq.launch.gx * 256u >= rq.P && (uint64_t)(rq.launch.gx - 1u) * 256u < rq.P && rq.n_coef <= 4u);
                }
            }
            for (uint32_t kx = 1; kx <= 15; kx += 2)
                for (uint32_t kz = 1; kz <= 15; kz += 2) {
                    pbrt_doppler_params p = valid();
                    p.nx = nx, p.nz = nz, p.kx = kx, p.kz = kz;
                    DopplerMapsRequest rq;
                    CHECK(doppler_maps_request(&rq, &p, ACF, VEL, AMP) == nullptr);
                    CHECK(rq.launch.gx >= 1u && rq.launch.gx <= 0x7fffffffu && rq.launch.gy == 1u && rq.launch.block == 256u);
                    CHECK(rq.launch.lds <= 65536u && rq.launch.lds % 4u == 0u);
                    CHECK((uint64_t)rq.tiles_z * DOPPLER_TILE_Z >= nz && rq.launch.gx % rq.tiles_z == 0u &&
                          (uint64_t)(rq.launch.gx / rq.tiles_z) * DOPPLER_TILE_X >= nx);
                    // the last word the kernel touches in LDS: the weights, the staged planes, the smoothed rows
                    const size_t rows = 8u + kx - 1u, cols = 32u + kz - 1u;
                    CHECK((32u + 3u * rows * cols + 3u * rows * 32u) * 4u == rq.launch.lds);
                }
        }

    std::printf("{\"checks\": %d, \"failures\": %d}\n", checks, failures);
    return failures ? 1 : 0;
}
