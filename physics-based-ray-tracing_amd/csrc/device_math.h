// device_math.h -- f32 device math of the gfx950 ray-transport kernels.
//
// Numeric contract: IEEE f32, no fast-math, compiled with -ffp-contract=off; every
// fused multiply-add is an explicit __builtin_fmaf in a fixed order; '/' and sqrtf are the
// correctly rounded forms (hipcc default -fhip-fp32-correctly-rounded-divide-sqrt); the only
// transcendental of radiance mode is the fixed polynomial sincos_pi4().  Under this contract the
// radiance kernels reproduce the CPU oracle bit for bit; ultrasound mode additionally calls
// sinf/cosf/expf/acosf (ocml), which agree with libm to a few ulp only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "film_key.h"  // FastDiv, make_fastdiv, udiv_fast: exact division by a launch-uniform divisor, where host-only code reads it too

#define DEV __device__ __forceinline__
#define HDEV __host__ __device__ __forceinline__  // the few statements the host evaluates too (the curved array's element table)

// rank of a lane among the lanes of ballot b below it
DEV uint32_t ballot_rank(unsigned long long b) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u)); }

// ---- short correctly rounded forms -----------------------------------------------------------------------
// A correctly rounded result is unique, so any sequence that provably returns RN(1/b), RN(a/b) or RN(sqrt x) has the bits of
// the compiler's '/' and sqrtf and of the CPU oracle.  The compiler's expansion pays for operand scaling and special values on
// every call (~11 VALU per division, ~13 per sqrtf); these forms are checked bit for bit against '/' and sqrtf on the device
// (tests/native/fp_short_forms.hip), over every f32 input for the one-operand forms.
//
// rcp_core(b): one Newton step on v_rcp_f32 (e = 1 - b y0 is exact because y0 is within an ulp of 1/b).  Equal to RN(1/b) for
// every b with 2^-126 <= |b| <= 2^126 (the device check: all 2^32 inputs, mismatches only for subnormal b and |b| > 2^126);
// rcp_rn adds v_div_fixup for 0, inf and NaN.  The reciprocal of a sqrtf or sqrt_rn result is always in that range.
DEV float rcp_core(float b) {
    const float y0 = __builtin_amdgcn_rcpf(b);
    const float e = __builtin_fmaf(-b, y0, 1.0f);
    return __builtin_fmaf(e, y0, y0);
}
DEV float rcp_rn(float b) { return __builtin_amdgcn_div_fixupf(rcp_core(b), b, 1.0f); }
// sqrt_rn(x): v_sqrt_f32 (not correctly rounded by itself) and a neighbour check (s - 1 ulp and s + 1 ulp by their fma
// residuals), without the compiler's operand scaling and class fix-up.  Equal to sqrtf for every x except 0 < |x| < 2^-104
// (there v_sqrt_f32 or the residuals leave the normal range): +-0, +inf, NaN and negative normals included.
DEV float sqrt_rn(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float dn = __uint_as_float(__float_as_uint(s) - 1u), up = __uint_as_float(__float_as_uint(s) + 1u);
    const float rdn = __builtin_fmaf(-dn, s, x), rup = __builtin_fmaf(-up, s, x);
    float r = rdn <= 0.0f ? dn : s;
    return rup > 0.0f ? up : r;
}
// div_rn(a, b): Markstein's correction on q = a RN(1/b): r = a - b q is exact and q + r y rounds to RN(a/b) while
// 2^-126 <= |b| <= 2^126 and either a == 0 or |a| >= 2^-100 with a quotient 2^-126 <= |a/b| < 2^127 (q = a y must not overflow);
// v_div_fixup for the signs and special operands.  Device check: every divisor mantissa at 11 exponents x 2050 numerators,
// and 1.3e10 random pairs of that domain.
DEV float div_rn(float a, float b) {
    const float y = rcp_core(b);
    const float q = a * y;
    const float r = __builtin_fmaf(-b, q, a);
    return __builtin_amdgcn_div_fixupf(__builtin_fmaf(r, y, q), b, a);
}

struct V3 {
    float x, y, z;
};

DEV V3 v3(float x, float y, float z) { return V3{x, y, z}; }
DEV V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
DEV V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
DEV V3 operator-(V3 a) { return {-a.x, -a.y, -a.z}; }
DEV V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
DEV V3 operator*(V3 a, V3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
HDEV float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
DEV float dot(V3 a, V3 b) { return fma_(a.x, b.x, fma_(a.y, b.y, a.z * b.z)); }
DEV V3 cross(V3 a, V3 b) {
    return {fma_(a.y, b.z, -(a.z * b.y)), fma_(a.z, b.x, -(a.x * b.z)), fma_(a.x, b.y, -(a.y * b.x))};
}
DEV V3 madd(V3 a, float s, V3 b) { return {fma_(a.x, s, b.x), fma_(a.y, s, b.y), fma_(a.z, s, b.z)}; }
DEV V3 normalize(V3 v) {
    float inv = rcp_rn(sqrtf(dot(v, v)));  // the reciprocal of a sqrtf result: inside rcp_rn's range
    return v * inv;
}
DEV float max3(V3 v) { return fmaxf(v.x, fmaxf(v.y, v.z)); }

#define K_PI 3.14159265358979323846f
#define K_INV_PI 0.31830988618379067154f
#define K_PI_OVER_4 0.78539816339744830962f
#define K_RAY_EPS (1500.0f / 16777216.0f)
#define K_SHADOW_EPS (15000.0f / 16777216.0f)
#define K_INF __builtin_huge_valf()

// ---- counter-based RNG: pcg4d keyed (a, b, c, seed) ---------------------------------------------
struct F4 {
    float x, y, z, w;
};
DEV float u01(uint32_t x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }
DEV F4 rng4(uint32_t a, uint32_t b, uint32_t c, uint32_t seed) {
    uint32_t x = a * 1664525u + 1013904223u;
    uint32_t y = b * 1664525u + 1013904223u;
    uint32_t z = c * 1664525u + 1013904223u;
    uint32_t w = seed * 1664525u + 1013904223u;
    x += y * w;
    y += z * x;
    z += x * y;
    w += y * z;
    x ^= x >> 16;
    y ^= y >> 16;
    z ^= z >> 16;
    w ^= w >> 16;
    x += y * w;
    y += z * x;
    z += x * y;
    w += y * z;
    return {u01(x), u01(y), u01(z), u01(w)};
}

// ---- sin/cos on [-pi/4, pi/4] -------------------------------------------------------------------
HDEV void sincos_pi4(float x, float *s, float *c) {
    float x2 = x * x;
    float ps = fma_(x2, 2.7557319223985893e-06f, -1.9841269841269841e-04f);
    ps = fma_(x2, ps, 8.3333333333333332e-03f);
    ps = fma_(x2, ps, -1.6666666666666666e-01f);
    *s = fma_(x * x2, ps, x);
    float pc = fma_(x2, 2.4801587301587302e-05f, -1.3888888888888889e-03f);
    pc = fma_(x2, pc, 4.1666666666666664e-02f);
    pc = fma_(x2, pc, -0.5f);
    *c = fma_(x2, pc, 1.0f);
}

// Mitsuba warp::square_to_uniform_disk_concentric (CustomBSDF.py:48)
DEV void square_to_disk(float sx, float sy, float *dx, float *dy) {
    float x = fma_(2.0f, sx, -1.0f), y = fma_(2.0f, sy, -1.0f);
    bool is_zero = (x == 0.0f) && (y == 0.0f);
    bool q13 = fabsf(x) < fabsf(y);
    float r = q13 ? y : x, rp = q13 ? x : y;
    // sx, sy in [0, 1]: x and y are 0 or multiples of 2^-24 in [-1, 1] and |rp| <= |r|, so r is in [2^-24, 1] and the quotient
    // 0 or in [2^-24, 1] (div_rn's domain); r == 0 only with is_zero, whose quotient is discarded
    float a = is_zero ? 0.0f : K_PI_OVER_4 * div_rn(rp, r);
    float s, c;
    sincos_pi4(a, &s, &c);
    *dx = r * (q13 ? s : c);
    *dy = r * (q13 ? c : s);
}
DEV V3 square_to_cosine_hemisphere(float sx, float sy) {
    float dx, dy;
    square_to_disk(sx, sy, &dx, &dy);
    float z2 = 1.0f - fma_(dx, dx, dy * dy);
    return {dx, dy, sqrt_rn(fmaxf(z2, 0.0f))};  // z2 = 1 - t, t >= 0: 0, >= 1/2, or a multiple of 2^-24 (Sterbenz)
}
DEV V3 square_to_uniform_hemisphere(float sx, float sy) {
    float dx, dy;
    square_to_disk(sx, sy, &dx, &dy);
    float z = 1.0f - fma_(dx, dx, dy * dy);
    float k = sqrt_rn(z + 1.0f);  // z + 1 = 2 - t with t = dx^2 + dy^2 <= 1 (rounded): at least 1 - 2^-23
    return {dx * k, dy * k, z};
}

// Mitsuba coordinate_system(n) == Frame3f(n) (CustomBSDF.py:32)
struct Frame {
    V3 s, t, n;
};
DEV Frame make_frame(V3 n) {
    float sign = copysignf(1.0f, n.z);
    float a = -rcp_rn(sign + n.z);  // |sign + n.z| >= 1: inside rcp_rn's range
    float b = n.x * n.y * a;
    Frame f;
    f.s = {fma_(sign * n.x, n.x * a, 1.0f), sign * b, -sign * n.x};
    f.t = {b, fma_(n.y, n.y * a, sign), -n.y};
    f.n = n;
    return f;
}
// Mitsuba SurfaceInteraction::initialize_sh_frame(): s = normalize(dp_du - n (n . dp_du)), t = n x s -- the frame
// si.wi, si.to_local and si.to_world use (CustomBSDF.py:90,165; CustomIntegrator.py:358).  Zero dp_du: coordinate_system(n).
DEV Frame make_sh_frame(V3 n, V3 dp_du) {
    V3 s = madd(n, -dot(n, dp_du), dp_du);
    float l2 = dot(s, s);
    if (!(l2 > 0.0f)) return make_frame(n);
    Frame f;
    f.s = s * rcp_rn(sqrtf(l2));
    f.t = cross(n, f.s);
    f.n = n;
    return f;
}
DEV V3 to_local(const Frame &f, V3 v) { return {dot(v, f.s), dot(v, f.t), dot(v, f.n)}; }
DEV V3 to_world(const Frame &f, V3 v) {
    return {fma_(f.s.x, v.x, fma_(f.t.x, v.y, f.n.x * v.z)), fma_(f.s.y, v.x, fma_(f.t.y, v.y, f.n.y * v.z)),
            fma_(f.s.z, v.x, fma_(f.t.z, v.y, f.n.z * v.z))};
}

// Mitsuba SurfaceInteraction::offset_p / spawn_ray (CustomIntegrator.py:324,359)
DEV V3 offset_origin(V3 p, V3 ng, V3 d) {
    float mag = (1.0f + fmaxf(fabsf(p.x), fmaxf(fabsf(p.y), fabsf(p.z)))) * K_RAY_EPS;
    mag = copysignf(mag, dot(ng, d));
    return madd(ng, mag, p);
}

// row-major 3x4 affine transform
DEV V3 xf_point(const float *m, V3 p) {
    return {fma_(m[0], p.x, fma_(m[1], p.y, fma_(m[2], p.z, m[3]))), fma_(m[4], p.x, fma_(m[5], p.y, fma_(m[6], p.z, m[7]))),
            fma_(m[8], p.x, fma_(m[9], p.y, fma_(m[10], p.z, m[11])))};
}
DEV V3 xf_vec(const float *m, V3 v) {
    return {fma_(m[0], v.x, fma_(m[1], v.y, m[2] * v.z)), fma_(m[4], v.x, fma_(m[5], v.y, m[6] * v.z)),
            fma_(m[8], v.x, fma_(m[9], v.y, m[10] * v.z))};
}

DEV float mis_weight(float a, float b) {
    a *= a;
    b *= b;
    float w = a / (a + b);
    return __builtin_isfinite(w) ? w : 0.0f;
}
