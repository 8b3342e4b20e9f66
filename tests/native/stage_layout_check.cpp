// Host check of the staging layout (csrc/stage_layout.h; tests/test_stage_layout_host.py builds and runs it under the sanitizers):
// over lists of 1 to 12 arrays of element sizes 1, 4 and 8, lengths 0, 1, 3, 5, 15, 16, 17, 67 and 2^20 + 1, some inputs null --
// every offset is a multiple of 16, slots do not overlap, the last slot ends at or before the total, the total is the sum of the
// rounded sizes, and the layout is a function of the list alone (null pointers and a second evaluation change nothing).  Then the
// lists the nine leaf operators and the host form of the beamformers hand to it, restated here from pbrt_api.hip, at 1 and 67 items:
// the total is at most what the driver used to count by hand, plus its 1024 bytes of slack.
// Prints one JSON line: {"checks": N, "failures": M}.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "stage_layout.h"

static int checks = 0, failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        ++checks;                                                     \
        if (!(cond)) {                                                \
            ++failures;                                               \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);   \
        }                                                             \
    } while (0)

static const size_t LENGTHS[] = {0, 1, 3, 5, 15, 16, 17, 67, (1u << 20) + 1u};
static uint32_t lcg = 12345u;
static uint32_t rnd(uint32_t n) {
    lcg = lcg * 1664525u + 1013904223u;
    return (lcg >> 8) % n;
}

// the properties of one layout, against the byte lengths it was made from
template <size_t N>
static void check_layout(const StageLayout<N> &L, const std::array<size_t, N> &bytes) {
    size_t sum = 0;
    for (size_t i = 0; i < N; ++i) {
        CHECK(L.offset[i] % 16 == 0);
        CHECK(L.offset[i] == sum);                      // slot i begins where slot i - 1 ends: no overlap, no gap
        CHECK(L.offset[i] + bytes[i] <= L.total);       // the array itself lies inside
        for (size_t j = 0; j < i; ++j) CHECK(L.offset[j] + bytes[j] <= L.offset[i]);
        const size_t slot = (bytes[i] + 15) / 16 * 16;  // (the rounding, restated)
        CHECK(slot >= bytes[i] && slot < bytes[i] + 16 && stage_slot(bytes[i]) == slot);
        sum += slot;
    }
    CHECK(L.total == sum);
}

// a list of N arrays drawn from the element sizes and lengths above, through the typed descriptions (u8 / float / double, in, out, inout)
template <size_t N>
static void random_lists(int rounds) {
    static const float f = 0;
    static const double d = 0;
    static const uint8_t b = 0;
    for (int r = 0; r < rounds; ++r) {
        std::array<size_t, N> bytes{}, again{};
        for (size_t i = 0; i < N; ++i) {
            const size_t n = LENGTHS[rnd(9)], kind = rnd(3), null = rnd(4) == 0;
            // the same array as a null input, as an input, as an output: its slot is the same
            const size_t b1 = kind == 0 ? stage_in(null ? nullptr : &b, n).bytes() : kind == 1 ? stage_in(null ? nullptr : &f, n).bytes()
                                                                                               : stage_in(null ? nullptr : &d, n).bytes();
            const size_t b2 = kind == 0 ? stage_out((uint8_t *)nullptr, n).bytes() : kind == 1 ? stage_out((float *)nullptr, n).bytes()
                                                                                               : stage_out((double *)nullptr, n).bytes();
            CHECK(b1 == b2 && b1 == n * (kind == 0 ? 1u : kind == 1 ? 4u : 8u));
            bytes[i] = again[i] = b1;
        }
        const StageLayout<N> L = stage_layout<N>(bytes), M = stage_layout<N>(again);
        check_layout(L, bytes);
        CHECK(L.total == M.total && L.offset == M.offset);
    }
}

// a call's list as the driver writes it, and the byte count the driver used to write by hand for it
template <class... T>
static void driver_list(size_t hand_count, const StageArray<T> &...a) {
    const auto L = stage_layout(a...);
    const std::array<size_t, sizeof...(T)> bytes{{a.bytes()...}};
    check_layout(L, bytes);
    CHECK(L.total <= hand_count + 1024);
}

static void driver_lists(uint32_t n) {
    const float *F = nullptr;  // (a layout reads no pointer)
    float *O = nullptr;
    uint32_t *U = nullptr;
    uint8_t *B = nullptr;
    const size_t n3 = 3 * (size_t)n;
    // pbrt_ray_intersect, pbrt_ray_test
    driver_list((size_t)n * 4 * 12, stage_in(F, n3), stage_in(F, n3), stage_in(F, n), stage_out(O, n), stage_out(U, n), stage_out(O, n), stage_out(O, n));
    driver_list((size_t)n * 4 * 9, stage_in(F, n3), stage_in(F, n3), stage_in(F, n), stage_out(B, n));
    // pbrt_bsdf_sample (n_geo, n_sh, sh_s may be null: the slots stay), pbrt_bsdf_eval_pdf
    driver_list((size_t)n * 4 * 25, stage_in(F, n3), stage_in(F, n3), stage_in(F, n3), stage_in(F, n3), stage_in(F, n), stage_in(F, 2 * (size_t)n),
                stage_out(O, n3), stage_out(O, n), stage_out(O, n3), stage_out(U, n));
    driver_list((size_t)n * 4 * 12, stage_in(F, n3), stage_in(F, n3), stage_out(O, n3), stage_out(O, n));
    // pbrt_emitter_sample_direction, pbrt_sensor_sample_ray
    driver_list((size_t)n * 4 * 22, stage_in(F, n3), stage_in(F, 4 * (size_t)n), stage_out(O, n3), stage_out(O, n), stage_out(O, n), stage_out(O, n3),
                stage_out(O, n3), stage_out(U, n));
    driver_list((size_t)n * 4 * 10, stage_in(F, 2 * (size_t)n), stage_out(O, n3), stage_out(O, n3), stage_out(O, n));
    // pbrt_us_sensor_sample_ray, pbrt_us_emitter_sample_ray
    driver_list((size_t)n * 4 * 14, stage_in(F, n), stage_in(F, n), stage_in(F, 2 * (size_t)n), stage_in(F, 2 * (size_t)n), stage_out(O, n3),
                stage_out(O, n3), stage_out(O, n));
    driver_list((size_t)n * 4 * 16, stage_in(F, n), stage_in(F, n), stage_in(F, 2 * (size_t)n), stage_in(F, n), stage_out(O, n3), stage_out(O, n3),
                stage_out(O, n), stage_out(O, n), stage_out(O, n));
    // pbrt_us_put_data on a receiver of 5 elements x 67 samples
    const size_t nb = 5 * 67;
    driver_list((size_t)n * 4 * 7 + nb * 4, stage_in(F, n), stage_in(F, n), stage_in(F, n3), stage_in(F, n), stage_inout(O, nb));
    // beamform_host: 3 angles x 5 elements x 67 samples on n = nx * nz pixels (nx = n, nz = 1); axes or pixel tables, positions or the
    // element table, real or I/Q samples
    for (int tab = 0; tab < 2; ++tab)
        for (int probe = 0; probe < 2; ++probe)
            for (size_t width = 1; width <= 2; ++width) {
                const size_t nd = 3 * 5 * 67 * width, ne = 3 * 5, nel = 5 * (probe ? 4u : 1u), ngx = n, ngz = tab ? n : 1;
                driver_list((nd + ne + nel + ngx + ngz + (size_t)n * width) * 4 + 256, stage_in(F, nd), stage_in(F, ne), stage_in(F, nel),
                            stage_in(F, ngx), stage_in(F, ngz), stage_out(O, n * width));
            }
}

int main() {
    random_lists<1>(40);
    random_lists<2>(60);
    random_lists<3>(60);
    random_lists<4>(60);
    random_lists<5>(60);
    random_lists<6>(60);
    random_lists<7>(60);
    random_lists<8>(60);
    random_lists<9>(60);
    random_lists<10>(60);
    random_lists<11>(60);
    random_lists<12>(60);
    // every length once in every position of a list of three, between a one-byte and an eight-byte neighbour
    for (size_t a : LENGTHS)
        for (size_t sz : {size_t(1), size_t(4), size_t(8)}) {
            const std::array<size_t, 3> bytes{{17, a * sz, 8 * 3}};
            check_layout(stage_layout<3>(bytes), bytes);
            CHECK(stage_layout<3>(bytes).offset[1] == 32 && stage_layout<3>(bytes).total == 32 + (a * sz + 15) / 16 * 16 + 32);
        }
    driver_lists(1);
    driver_lists(67);
    // pbrt_bsdf_sample at 1000 items: 92000 bytes, where the hand count asked for 100000 + 1024
    {
        const float *F = nullptr;
        float *O = nullptr;
        uint32_t *U = nullptr;
        CHECK(stage_layout(stage_in(F, 3000), stage_in(F, 3000), stage_in(F, 3000), stage_in(F, 3000), stage_in(F, 1000), stage_in(F, 2000),
                           stage_out(O, 3000), stage_out(O, 1000), stage_out(O, 3000), stage_out(U, 1000)).total == 92000);
    }
    std::printf("{\"checks\": %d, \"failures\": %d}\n", checks, failures);
    return failures ? 1 : 0;
}
