// Host check of csrc/us_request.h (tests/test_us_request_host.py builds and runs it under the sanitizers, with the library's
// -ffp-contract=off): the maker turns a valid pbrt_us_params into the facts the stages of the acquisition driver read, refuses every
// single violation of the argument rules with a text that names the field and with the right code, reports the first of two
// violations in the order the driver always kept, computes the host's constants of UsArgs as the float64 statements of
// CustomIntegrator.py say, and the permutation stride of the emitter regions is the loop the driver used to carry.
// Prints one JSON line: {"checks": N, "failures": M}.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <numeric>

#include "us_request.h"

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
static const char *UNSUPPORTED = "emitter.radius != 0 transmits from an arc: set PBRT_US_ARRAY_CONVEX in pbrt_us_params.primary";

static const float IDENT[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
static const uint32_t NA = 3, NE = 8, T = 256;

static pbrt_us_params linear() {
    pbrt_us_params p;
    std::memset(&p, 0, sizeof p);
    p.max_depth = 4, p.frequency = 5e6f, p.sound_speed = 1540.0f, p.attenuation = 0.2f;
    p.main_beam_angle = 24.0f, p.cutoff_angle = 30.0f, p.fs = 50e6f;
    p.n_elements = NE, p.pitch = 1.2e-4f, p.n_angles = NA, p.time_samples = T;
    p.angles_deg[0] = -7.5f, p.angles_deg[1] = 0.0f, p.angles_deg[2] = 7.5f;
    std::memcpy(p.sensor_to_world, IDENT, sizeof IDENT);
    p.quirks = PBRT_USQ_REFERENCE, p.primary = PBRT_US_PRIMARY_ELEMENT;
    return p;
}
static pbrt_us_params emitter() {  // CustomEmitter on the acquisition's elements as the source of the primary rays
    pbrt_us_params p = linear();
    p.primary = PBRT_US_PRIMARY_EMITTER;
    pbrt_us_emitter &E = p.emitter;
    E.number_of_elements = NE, E.pitch = 1.2e-4f, E.element_width = 1e-4f, E.element_height = 4e-4f;
    E.number_of_rays_per_element = 1, E.speed_of_sound = 1540.0f, E.steering_angle_min = -12.0f, E.steering_angle_max = 12.0f;
    return p;
}
static pbrt_us_params with_array(pbrt_us_params p) {  // the curved array on top of either
    p.primary |= PBRT_US_ARRAY_CONVEX;
    p.emitter.number_of_elements = NE, p.emitter.radius = 0.03f, p.emitter.opening_angle = 40.0f;
    return p;
}
static pbrt_us_params convex() { return with_array(linear()); }

// accepted, with the facts of the request
static bool taken(const pbrt_us_params &p, uint32_t ppr, bool cvx, bool emit, bool tables, bool fuse) {
    UsRequest rq;
    if (us_request(&rq, &p, ppr, true) != nullptr || rq.code != PBRT_OK) return false;
    return rq.p == &p && rq.convex == cvx && rq.emit == emit && rq.primary == (emit ? PBRT_US_PRIMARY_EMITTER : PBRT_US_PRIMARY_ELEMENT) &&
           rq.NA == p.n_angles && rq.NE == p.n_elements && rq.T == p.time_samples && rq.n_rays == p.n_angles * p.n_elements &&
           rq.n_ex == (cvx ? 4u : 1u) * p.n_elements && rq.nchan == (uint64_t)p.n_angles * p.n_elements * p.time_samples &&
           rq.tables == tables && rq.fuse == fuse;
}
// refused with this code and a text that holds `field` (INVALID), or is `field` (UNSUPPORTED)
static bool refused(const pbrt_us_params *p, uint32_t ppr, bool has_channel, int code, const char *field) {
    UsRequest rq;
    const char *why = us_request(&rq, p, ppr, has_channel);
    if (!why || rq.code != code) return false;
    return code == PBRT_E_UNSUPPORTED ? std::strcmp(why, field) == 0 : std::strstr(why, field) != nullptr;
}
static const char *text_of(const pbrt_us_params &p, uint32_t ppr = 4) {
    UsRequest rq;
    const char *why = us_request(&rq, &p, ppr, true);
    return why ? why : "";
}
// one violation on a valid block
template <class Edit>
static void violation(pbrt_us_params p, const char *field, Edit edit, int code = PBRT_E_INVALID) {
    CHECK(text_of(p)[0] == '\0');
    edit(p);
    CHECK(refused(&p, 4, true, code, field));
}
static bool same(const char *a, const char *b) { return std::strcmp(a, b) == 0; }

// ---- the float64 restatement of CustomIntegrator.py:265-273: a_rad = deg2rad(angle); direction = (sin a, 0, cos a);
// normalize(sensor_T @ direction); and of the transducer normal, normalize(sensor_T @ (0, 0, 1)) ----
static void ref_dir(const float *M, double x, double y, double z, double *o) {
    for (int r = 0; r < 3; ++r) o[r] = (double)M[4 * r] * x + (double)M[4 * r + 1] * y + (double)M[4 * r + 2] * z;
    const double len = std::sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]);
    for (int r = 0; r < 3; ++r) o[r] /= len;
}
// The bound on |float32 - float64| per component, u = 2^-24, for a rotation (rows of unit length) and angles up to 45 degrees:
//  - sin, cos: the argument is rounded once (<= u |a| < 0.8 u), sinf / cosf are within 1 ulp (<= 2 u for values up to 1): 3 u each;
//  - three multiply-adds per component: the inputs' 3 u times |M_r0| + |M_r2| <= sqrt 2 (4.3 u), and the two roundings that are not
//    exact (M_r2 z, the outer fma; the inner adds M_r1 * 0) on values up to 1: 2 u.  6.3 u per component, sqrt 3 * 6.3 u = 11 u of the length;
//  - the normalisation: 1 / sqrt(v . v) carries those 11 u, 1.5 u of the three roundings under the root, u of the root, u of the
//    division; the product with the component one more u: 15.5 u times a component of at most 1.
// 6.3 u + 15.5 u < 22 u.
static const double DIR_TOL = 22.0 * 5.9604644775390625e-08;

static void constants_of(const pbrt_us_params &p, bool exact_axis) {
    UsRequest rq;
    CHECK(us_request(&rq, &p, 4, true) == nullptr);
    double want[3];
    ref_dir(p.sensor_to_world, 0.0, 0.0, 1.0, want);
    for (int k = 0; k < 3; ++k) CHECK(std::fabs((double)rq.tn[k] - want[k]) <= DIR_TOL);
    for (uint32_t a = 0; a < p.n_angles; ++a) {
        const double ar = (double)p.angles_deg[a] * (M_PI / 180.0);
        ref_dir(p.sensor_to_world, std::sin(ar), 0.0, std::cos(ar), want);
        for (int k = 0; k < 3; ++k) CHECK(std::fabs((double)rq.dir0[3 * a + k] - want[k]) <= DIR_TOL);
        if (exact_axis && p.angles_deg[a] == 0.0f) CHECK(rq.dir0[3 * a] == 0.0f && rq.dir0[3 * a + 1] == 0.0f && rq.dir0[3 * a + 2] == 1.0f);
    }
    if (exact_axis) CHECK(rq.tn[0] == 0.0f && rq.tn[1] == 0.0f && rq.tn[2] == 1.0f);
    // the float statements, each operation in float64 and rounded once (exact for +, *, / of float32 operands: 53 >= 2 * 24 + 2)
    const float k = (float)((double)3.14159265358979323846f / 180.0);
    CHECK(rq.am == (float)((double)p.main_beam_angle * (double)k));
    CHECK(rq.ac == (float)((double)p.cutoff_angle * (double)k));
    CHECK(rq.inv_c == (float)(1.0 / (double)p.sound_speed));
    // cosf is within 1 ulp of the rounded float64 cosine, not bound to be it
    const float c64 = (float)std::cos((double)rq.ac);
    CHECK(rq.cos_min >= std::nextafterf(c64, -2.0f) && rq.cos_min <= std::nextafterf(c64, 2.0f));
    CHECK(rq.katt == (float)(-(double)p.attenuation * (double)p.frequency * 1e-6));      // CustomIntegrator.py:328
    CHECK(rq.two_pi_f == (float)(2.0 * M_PI * (double)p.frequency));                     // :330
}

// the loop the driver carried (pbrt_api.hip us_impl before the stages), for regions > 2 NA and a switch that is not 0
static uint32_t parent_blk_mul(uint32_t nseg_pass, uint32_t na, int permute) {
    uint32_t m = (nseg_pass / na) | 1u;
    if (permute > 1) m = (uint32_t)permute | 1u;
    while (std::gcd(m, nseg_pass) != 1u) m += 2u;
    return m % nseg_pass;
}

int main() {
    // ---- valid blocks -> the facts every stage reads ----
    {
        pbrt_us_params p = linear();
        CHECK(taken(p, 16, false, false, true, true));
        p = convex();
        CHECK(taken(p, 16, true, false, true, true));
        p = emitter();
        CHECK(taken(p, 16, false, true, false, true));                 // (emitter rays: every path has its own origin, no tables)
        p = with_array(emitter());
        CHECK(taken(p, 16, true, true, false, true));
        // first-bounce tables: once a ray has at least as many paths as receive elements
        p = linear();
        CHECK(taken(p, NE - 1, false, false, false, true));
        CHECK(taken(p, NE, false, false, true, true));
        CHECK(taken(p, NE + 1, false, false, true, true));
        p = convex();
        CHECK(taken(p, NE - 1, true, false, false, true) && taken(p, NE, true, false, true, true));
        p = linear();
        p.quirks |= PBRT_USQ_NO_FIRST_TABLES;
        CHECK(taken(p, 16, false, false, false, true));
        p.quirks = PBRT_USQ_REFERENCE | PBRT_USQ_NO_FUSED_BOUNCES;
        CHECK(taken(p, 16, false, false, true, false));
        p.quirks = 0;
        CHECK(taken(p, 1, false, false, false, true));
        // the limits themselves are taken
        p = linear();
        p.n_angles = PBRT_US_MAX_ANGLES;
        CHECK(taken(p, 16, false, false, true, true));
        p = linear();
        p.max_depth = 0x3fffffffu;
        CHECK(taken(p, 16, false, false, true, true));
        p = linear();
        p.n_angles = 3, p.n_elements = 21845, p.time_samples = 65536;   // 2^32 - 65536 bins
        CHECK(taken(p, 1, false, false, false, true));
        p = emitter();
        p.emitter.radius = 0.03f;                                       // read only with the array bit or emitter rays
        p.primary = PBRT_US_PRIMARY_ELEMENT;
        CHECK(taken(p, 16, false, false, true, true));
        p = linear();
        p.emitter.pitch = NaN;                                          // (not read without emitter rays)
        CHECK(taken(p, 16, false, false, true, true));
        CHECK(us_array_rules(&p) != nullptr);
        p = convex();
        CHECK(us_array_rules(&p) == nullptr && us_convex(&p));
        p = linear();
        CHECK(!us_convex(&p));
    }

    // ---- no block, no channel buffer ----
    {
        pbrt_us_params p = linear();
        CHECK(refused(nullptr, 4, true, PBRT_E_INVALID, "p"));
        CHECK(refused(&p, 4, false, PBRT_E_INVALID, "has_channel"));
    }

    // ---- single violations: the text names the field, the code is PBRT_E_INVALID ----
    violation(linear(), "n_angles", [](pbrt_us_params &p) { p.n_angles = 0; });
    violation(linear(), "n_elements", [](pbrt_us_params &p) { p.n_elements = 0; });
    violation(linear(), "time_samples", [](pbrt_us_params &p) { p.time_samples = 0; });
    violation(linear(), "max_depth", [](pbrt_us_params &p) { p.max_depth = 0; });
    {
        pbrt_us_params p = linear();
        CHECK(refused(&p, 0, true, PBRT_E_INVALID, "ppr"));
    }
    violation(linear(), "n_angles", [](pbrt_us_params &p) { p.n_angles = PBRT_US_MAX_ANGLES + 1; });
    violation(linear(), "n_angles", [](pbrt_us_params &p) { p.n_angles = 0xffffffffu; });
    // 3 x 21845 x 65537 = 2^32 - 1: the first count the 32-bit channel index does not address
    violation(linear(), "time_samples", [](pbrt_us_params &p) { p.n_angles = 3, p.n_elements = 21845, p.time_samples = 65537; });
    violation(linear(), "time_samples", [](pbrt_us_params &p) { p.n_angles = 64, p.n_elements = 0x10000u, p.time_samples = 0x10000u; });
    violation(linear(), "max_depth", [](pbrt_us_params &p) { p.max_depth = 0x40000000u; });
    violation(linear(), "max_depth", [](pbrt_us_params &p) { p.max_depth = 0xffffffffu; });
    for (float v : {0.0f, -1.0f, NaN}) {
        violation(linear(), "fs", [v](pbrt_us_params &p) { p.fs = v; });
        violation(linear(), "sound_speed", [v](pbrt_us_params &p) { p.sound_speed = v; });
    }
    for (uint32_t v : {2u, 3u, 0xffu, 0x200u, 0xffffffffu, 2u | PBRT_US_ARRAY_CONVEX})
        violation(linear(), "primary", [v](pbrt_us_params &p) { p.primary = v; });
    // the emitter's own fields
    for (float v : {NaN, Inf, -Inf}) {
        violation(emitter(), "pitch", [v](pbrt_us_params &p) { p.emitter.pitch = v; });
        violation(emitter(), "element_width", [v](pbrt_us_params &p) { p.emitter.element_width = v; });
        violation(emitter(), "element_height", [v](pbrt_us_params &p) { p.emitter.element_height = v; });
        violation(emitter(), "radius", [v](pbrt_us_params &p) { p.emitter.radius = v; });
        violation(emitter(), "steering_angle_min", [v](pbrt_us_params &p) { p.emitter.steering_angle_min = v; });
        violation(emitter(), "steering_angle_max", [v](pbrt_us_params &p) { p.emitter.steering_angle_max = v; });
        violation(emitter(), "opening_angle", [v](pbrt_us_params &p) { p.emitter.opening_angle = v; });
    }
    violation(emitter(), "number_of_elements", [](pbrt_us_params &p) { p.emitter.number_of_elements = NE + 1; });
    violation(emitter(), "number_of_elements", [](pbrt_us_params &p) { p.n_elements = NE - 1; });
    violation(emitter(), "number_of_rays_per_element", [](pbrt_us_params &p) { p.emitter.number_of_rays_per_element = 0; });
    for (float v : {0.0f, -1540.0f, NaN}) violation(emitter(), "speed_of_sound", [v](pbrt_us_params &p) { p.emitter.speed_of_sound = v; });
    // the curved array, under element rays and under emitter rays
    for (const pbrt_us_params &base : {convex(), with_array(emitter())}) {
        violation(base, "number_of_elements", [](pbrt_us_params &p) { p.emitter.number_of_elements = NE - 1; });
        for (float v : {0.0f, -0.03f, NaN}) violation(base, "radius", [v](pbrt_us_params &p) { p.emitter.radius = v; });
        for (float v : {0.0f, 180.0f, NaN, -40.0f, 200.0f}) violation(base, "opening_angle", [v](pbrt_us_params &p) { p.emitter.opening_angle = v; });
    }
    violation(convex(), "radius", [](pbrt_us_params &p) { p.emitter.radius = Inf; });
    violation(convex(), "number_of_elements", [](pbrt_us_params &p) { p.n_elements = NE + 1; });
    {   // the helpers' rule function alone gives the same answers
        pbrt_us_params p = convex();
        p.emitter.opening_angle = 180.0f;
        const char *why = us_array_rules(&p);
        CHECK(why && std::strstr(why, "opening_angle"));
        p.emitter.opening_angle = 179.0f;
        CHECK(us_array_rules(&p) == nullptr);
    }
    // an emitter on an arc without the array bit: its own code, its text verbatim
    violation(emitter(), UNSUPPORTED, [](pbrt_us_params &p) { p.emitter.radius = 0.03f; }, PBRT_E_UNSUPPORTED);
    violation(emitter(), UNSUPPORTED, [](pbrt_us_params &p) { p.emitter.radius = -1.0f; }, PBRT_E_UNSUPPORTED);

    // ---- the texts are the ones the driver has always reported (the parameter block's own field names) ----
    {
        pbrt_us_params p = linear();
        p.n_elements = 0;
        CHECK(same(text_of(p), "p->n_angles > 0 && p->n_angles <= PBRT_US_MAX_ANGLES && p->n_elements > 0 && p->time_samples > 0"));
        p = linear(), p.n_angles = 3, p.n_elements = 21845, p.time_samples = 65537;
        CHECK(same(text_of(p), "(uint64_t)p->n_angles * p->n_elements * p->time_samples < 0xffffffffull"));
        p = linear(), p.fs = 0.0f;
        CHECK(same(text_of(p), "p->max_depth > 0 && ppr > 0 && p->sound_speed > 0 && p->fs > 0"));
        p = linear(), p.max_depth = 0x40000000u;
        CHECK(same(text_of(p), "p->max_depth < 0x40000000u"));
        p = linear(), p.primary = 2;
        CHECK(same(text_of(p), "primary <= PBRT_US_PRIMARY_EMITTER"));
        p = emitter(), p.emitter.speed_of_sound = 0.0f;
        CHECK(same(text_of(p), "E.number_of_elements == p->n_elements && E.number_of_rays_per_element > 0 && E.speed_of_sound > 0.0f"));
        p = emitter(), p.emitter.element_height = NaN;
        CHECK(same(text_of(p), "std::isfinite(E.pitch) && std::isfinite(E.element_width) && std::isfinite(E.element_height) && std::isfinite(E.radius)"));
        p = emitter(), p.emitter.opening_angle = NaN;
        CHECK(same(text_of(p), "std::isfinite(E.steering_angle_min) && std::isfinite(E.steering_angle_max) && std::isfinite(E.opening_angle)"));
        p = convex(), p.emitter.radius = 0.0f;
        CHECK(same(text_of(p), "std::isfinite(E.radius) && E.radius > 0.0f"));
        p = convex(), p.emitter.opening_angle = 0.0f;
        CHECK(same(text_of(p), "std::isfinite(E.opening_angle) && E.opening_angle > 0.0f && E.opening_angle < 180.0f"));
        p = convex(), p.emitter.number_of_elements = 1;
        CHECK(same(text_of(p), "E.number_of_elements == p->n_elements"));
    }

    // ---- two violations: the one the driver's order meets first ----
    {
        pbrt_us_params p = linear();
        p.n_angles = 0, p.fs = 0.0f;                                               // counts before rates
        CHECK(refused(&p, 4, true, PBRT_E_INVALID, "n_angles") && !std::strstr(text_of(p), "fs"));
        p = linear(), p.max_depth = 0x40000000u, p.primary = 2;                    // the depth limit before the primary
        CHECK(same(text_of(p), "p->max_depth < 0x40000000u"));
        p = emitter(), p.emitter.number_of_elements = NE + 1, p.emitter.pitch = NaN;   // the emitter's counts before its finite fields
        CHECK(refused(&p, 4, true, PBRT_E_INVALID, "number_of_rays_per_element"));
        p = emitter(), p.emitter.pitch = NaN, p.emitter.radius = 0.03f;            // a non-finite field before the arc without the bit
        CHECK(refused(&p, 4, true, PBRT_E_INVALID, "std::isfinite(E.pitch)"));
        p = emitter(), p.emitter.steering_angle_max = Inf, p.emitter.radius = 0.03f;
        CHECK(refused(&p, 4, true, PBRT_E_INVALID, "steering_angle_max"));
        p = with_array(emitter()), p.emitter.steering_angle_min = NaN, p.emitter.radius = -0.03f;   // the emitter group before the array group
        CHECK(refused(&p, 4, true, PBRT_E_INVALID, "steering_angle_min"));
        p = with_array(emitter()), p.emitter.number_of_elements = NE + 1, p.emitter.opening_angle = 180.0f;
        CHECK(refused(&p, 4, true, PBRT_E_INVALID, "number_of_rays_per_element"));   // (the emitter's rule, not the array's last one)
        p = convex(), p.emitter.radius = 0.0f, p.emitter.opening_angle = 180.0f;   // radius, opening angle, elements
        CHECK(same(text_of(p), "std::isfinite(E.radius) && E.radius > 0.0f"));
        p = convex(), p.emitter.opening_angle = NaN, p.emitter.number_of_elements = 1;
        CHECK(refused(&p, 4, true, PBRT_E_INVALID, "opening_angle"));
        p = convex(), p.primary |= 2u, p.emitter.radius = 0.0f;                    // the primary before the array
        CHECK(same(text_of(p), "primary <= PBRT_US_PRIMARY_EMITTER"));
    }

    // ---- constants ----
    constants_of(linear(), true);
    constants_of(convex(), true);
    {
        // rotations about y by 30 degrees and about (1, 2, 3) / sqrt 14 by 75 degrees (Rodrigues, float64, rounded once), each translated
        pbrt_us_params p = linear();
        p.angles_deg[0] = -15.0f, p.angles_deg[1] = 0.0f, p.angles_deg[2] = 45.0f;
        const double t = 30.0 * M_PI / 180.0;
        const float Ry[12] = {(float)std::cos(t), 0, (float)std::sin(t), 0.01f, 0, 1, 0, -0.02f, (float)-std::sin(t), 0, (float)std::cos(t), 0.5f};
        std::memcpy(p.sensor_to_world, Ry, sizeof Ry);
        constants_of(p, false);
        const double n = std::sqrt(14.0), ax[3] = {1 / n, 2 / n, 3 / n}, th = 75.0 * M_PI / 180.0, c = std::cos(th), s = std::sin(th);
        const double K[3][3] = {{0, -ax[2], ax[1]}, {ax[2], 0, -ax[0]}, {-ax[1], ax[0], 0}};
        float R[12];
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) R[4 * r + k] = (float)((r == k ? c : 0.0) + s * K[r][k] + (1 - c) * ax[r] * ax[k]);
            R[4 * r + 3] = 0.1f * (float)(r + 1);
        }
        std::memcpy(p.sensor_to_world, R, sizeof R);
        p.main_beam_angle = 20.0f, p.cutoff_angle = 35.0f, p.sound_speed = 1480.0f, p.frequency = 3e6f, p.attenuation = 0.3f;
        constants_of(p, false);
    }
    {   // K2 of tests/test_known_answers.py: 64 elements at a pitch of 0.12 mm lie at -3.78 mm .. 3.78 mm
        pbrt_us_params p = linear();
        p.n_elements = 64;
        CHECK(us_elem_x(&p, 0) == -0.0037799999117851257f && us_elem_x(&p, 63) == 0.0037799999117851257f);
        CHECK(std::fabs(us_elem_x(&p, 0) + 0.00378) <= 1e-6 * 0.00378 && std::fabs(us_elem_x(&p, 63) - 0.00378) <= 1e-6 * 0.00378);
        bool sym = true, stated = true;
        for (uint32_t e = 0; e < 64; ++e) {
            sym = sym && us_elem_x(&p, e) == -us_elem_x(&p, 63 - e);
            stated = stated && us_elem_x(&p, e) == (float)((double)p.pitch * ((double)e - 31.5));   // CustomIntegrator.py:248
        }
        CHECK(sym);
        CHECK(stated);
        p.n_elements = 1;
        CHECK(us_elem_x(&p, 0) == 0.0f);
        // K3's attenuation 0.2 dB / (cm MHz) at 5 MHz: -1e-6 * 0.2 * 5e6 = -1 (float operands, one rounding)
        UsRequest rq;
        p = linear();
        CHECK(us_request(&rq, &p, 4, true) == nullptr && std::fabs((double)rq.katt + 1.0) <= 1e-7 && std::fabs((double)rq.two_pi_f - 31415926.5) <= 2.0);
    }

    {   // what the kernels' argument block takes from the request (a stand-in with the members of kernels_us.h UsArgs)
        struct Args {
            pbrt_us_params p;
            float tn[3], am, ac, cos_min, katt, two_pi_f, inv_c;
            uint32_t fuse;
        } a;
        pbrt_us_params p = with_array(emitter());
        p.quirks |= PBRT_USQ_NO_FUSED_BOUNCES;
        UsRequest rq;
        CHECK(us_request(&rq, &p, 4, true) == nullptr);
        us_request_args(rq, &a);
        CHECK(a.p.primary == PBRT_US_PRIMARY_EMITTER && p.primary == (PBRT_US_PRIMARY_EMITTER | PBRT_US_ARRAY_CONVEX));
        a.p.primary = p.primary;
        CHECK(std::memcmp(&a.p, &p, sizeof p) == 0);
        CHECK(a.tn[0] == rq.tn[0] && a.tn[1] == rq.tn[1] && a.tn[2] == rq.tn[2] && a.fuse == 0u);
        CHECK(a.am == rq.am && a.ac == rq.ac && a.cos_min == rq.cos_min && a.katt == rq.katt && a.two_pi_f == rq.two_pi_f && a.inv_c == rq.inv_c);
        p.quirks = PBRT_USQ_REFERENCE;
        CHECK(us_request(&rq, &p, 4, true) == nullptr);
        us_request_args(rq, &a);
        CHECK(a.fuse == 1u);
    }

    // ---- the permutation stride of the emitter regions ----
    for (uint32_t na : {1u, 2u, 9u, 64u})
        for (int permute : {0, 1, 2, 5, 12, -1}) {
            bool zero_rule = true, range = true, coprime = true, parent = true;
            for (uint32_t n = 1; n <= 4096; ++n) {
                const uint32_t m = us_emit_blk_mul(n, na, permute);
                const bool off = n <= 2u * na || permute == 0;
                zero_rule = zero_rule && (m == 0) == off;
                if (off) continue;
                range = range && m >= 1 && m < n;
                coprime = coprime && std::gcd(m, n) == 1u;
                parent = parent && m == parent_blk_mul(n, na, permute);
            }
            CHECK(zero_rule);
            CHECK(range);
            CHECK(coprime);
            CHECK(parent);
        }

    std::printf("{\"checks\": %d, \"failures\": %d}\n", checks, failures);
    return failures ? 1 : 0;
}
