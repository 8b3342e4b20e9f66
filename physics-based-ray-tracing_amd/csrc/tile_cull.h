// Which primitives can the camera rays of a film rectangle meet?  (the keep table of the first brute-force bounce:
// kernels_radiance.h k_tile_keep builds one word per 64 paths, device_scene.h brute_intersect skips the cleared bits.)
// Plain C++ (no HIP), so that tests/native/tile_cull_check.cpp can build it on its own; under hipcc the one function is also
// a device function.
//
// tile_cull_keep(cam, x0, y0, x1, y1, P) answers for the rays camera_ray() makes from the film positions
// [x0, x1 + 1] x [y0, y1 + 1] (pixels, inclusive: px + jitter can round up to px + 1).  It returns false only if it can prove, in
// double, that the kernel's FLOAT test of P rejects every such ray; anything it cannot bound -- a non-finite input, a camera
// matrix that is not a rotation times one scale, a camera in or near the primitive's plane, a far clip so large that the float
// test loses its grip, cones and cylinders -- is kept.
//
// The rays.  In camera space a ray points along (a, b, 1), a = (1 - 2 sx) tan_x, b = (1 - 2 sy) tan_y, so the rays of the
// rectangle fill a four-sided cone with its apex at the camera position `org`.  The float ray is (o_f, d_f) with
// o_f = org + s d_f + delta, s = near / dc.z >= 0.  d_f carries the roundings of film_coord, two normalisations and the matrix:
// a few 2^-24 of a unit vector, which moves (a, b) by at most that times 1 / dc.z^2; the cone is widened by
// EPS_AB = 64 * 2^-24 * (1 + tan_x^2 + tan_y^2) in a and b.  |delta| <= DELTA = 8 * 2^-24 * (|org|_1 + s_max) is the rounding of the
// madd that makes o_f.  Every point o_f + t d_f, t >= 0, of a float ray is then org + (s + t) d_f + delta: inside the widened cone
// up to DELTA.  With unit inward normals n_k of the four side planes:  n_k . (X - org) >= -DELTA  for every such point X.
//
// Planar primitives (brute_planar_run).  With tvec = o_f - v0, N = e1 x e2:  us = tvec . (d x e2), vs = d . (tvec x e1),
// det = e1 . (d x e2), ts = e2 . (tvec x e1) = tvec . N; the float test accepts only if (after the common sign flip) det_f > 0,
// us_f, vs_f, ts_f >= 0, us_f <= det_f, vs_f <= det_f (triangle: us_f + vs_f <= det_f) and ts_f <= tmax * det_f.  Each is a
// triple product of float data evaluated in about ten roundings, so with GAMMA = K * 2^-24, K = 16, and T >= |tvec|:
//   |us_f - us| <= eta_u = GAMMA T |e2|,  |vs_f - vs| <= eta_v = GAMMA T |e1|,  |det_f - det| <= eta_d = GAMMA |e1| |e2|,
//   |ts_f - ts| <= eta_t = GAMMA T |e1| |e2|,
// and a SAFETY factor of 4 on GAMMA on top.  T = |org - v0| + s_max + DELTA.  ts is constant up to the near-clip offset:
// |ts| >= ts_low = |(org - v0) . N| - (s_max + DELTA) |N| - eta_t.  Camera rays have a finite tmax = (far - near) / dc.z <= tmax_hi
// (the longest 1 / dc.z of the rectangle); an accepted candidate has ts_f <= tmax * det_f up to one rounding, so
//   |det| >= det_low = ts_low / (tmax_hi (1 + 2^-22)) - eta_d.
// If ts_low <= 0 or det_low <= 0 nothing is known: keep.  Otherwise ts_f and det_f have the signs of ts and det, the exact
// crossing of the float ray's line with the plane lies at t = ts / det >= 0, i.e. on the ray, and its exact parameters obey
//   -m <= u, v <= 1 + m  (triangle: u + v <= 1 + 2 m),  m = (max(eta_u, eta_v) + eta_d) / det_low  --  eta * tmax / |ts| in short.
// m > 1/4: keep (this is the camera in or near the plane, and the huge far clip).  So an accepted ray crosses the primitive
// inflated by m in its own (u, v) at a point of the widened cone; the inflated primitive is convex, and if all its corners lie
// beyond one side plane, n_k . (V - org) < -DELTA, no such point exists and the primitive is culled for the rectangle.
//
// Spheres (sphere_hit).  f = o_f - c, bp = -f . d, perp = f + bp d, disc = r^2 - |perp|^2 >= 0 is required; the float |perp|^2 is
// off by at most GAMMA |f|^2 (SAFETY included), so an accepted ray's line passes within r_eff, r_eff^2 = r^2 + GAMMA F^2,
// F = |org - c| + s_max + DELTA.  The accepted root must also be >= 0 in float.  If the ray origins are well outside,
// |org - c| - s_max - DELTA >= 2 r_eff, then |bp| >= 0.86 |f| and cc = |f|^2 - r^2 >= 0.75 |f|^2 keep their signs in float, both roots
// have the sign of bp, and an accepted ray has bp > 0: the point of the line nearest to c, within r_eff of it, lies on the ray
// and so in the widened cone.  The sphere is culled if  n_k . (c - org) < -(r_eff + DELTA)  for one side plane, and kept if the
// origins are not well outside.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/pbrt_hip.h"

#if defined(__HIPCC__)
#define TILE_CULL_FN __host__ __device__ inline
#else
#define TILE_CULL_FN inline
#endif

#define TILE_CULL_K 16.0        // roundings allowed for in one float quantity of the tests
#define TILE_CULL_SAFETY 4.0    // the stated safety factor on top
#define TILE_CULL_M_CAP 0.25    // margin in the primitive's (u, v) beyond which nothing is culled

TILE_CULL_FN bool tile_cull_keep(const pbrt_camera &cam, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const pbrt_prim &P) {
    const double U = 1.0 / 16777216.0;  // 2^-24
    const double GAMMA = TILE_CULL_K * TILE_CULL_SAFETY * U;
    const uint32_t type = P.type;
    if (type != PBRT_PRIM_PARALLELOGRAM && type != PBRT_PRIM_TRIANGLE && type != PBRT_PRIM_SPHERE) return true;
    if (x1 < x0 || y1 < y0 || cam.film_w == 0 || cam.film_h == 0) return true;
    // ---- the camera: finite, and a rotation times one positive scale (rows of the 3x3 part against each other)
    double M[3][3], org[3];
    double fin = 0.0;  // stays 0 while everything that went in is finite (x - x is NaN for inf and NaN)
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            M[r][c] = (double)cam.to_world[4 * r + c];
            fin += M[r][c] - M[r][c];
        }
        org[r] = (double)cam.to_world[4 * r + 3];
        fin += org[r] - org[r];
    }
    const double tx = (double)cam.tan_half_fov_x, near = (double)cam.near_clip, far = (double)cam.far_clip;
    const double ty = tx * (double)cam.film_h / (double)cam.film_w;
    fin += (tx - tx) + (near - near) + (far - far);
    for (int k = 0; k < 12; ++k) fin += (double)P.g[k] - (double)P.g[k];
    if (!(fin == 0.0)) return true;
    if (!(tx > 0.0) || !(near >= 0.0) || !(far > near)) return true;
    double G[3][3];  // M^T M
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) G[i][j] = M[0][i] * M[0][j] + M[1][i] * M[1][j] + M[2][i] * M[2][j];
    const double s2 = (G[0][0] + G[1][1] + G[2][2]) / 3.0;
    if (!(s2 > 0.0)) return true;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (!(fabs(G[i][j] - (i == j ? s2 : 0.0)) <= 1e-4 * s2)) return true;
    // ---- the widened cone of the rectangle's rays: (a, b) ranges in camera space, corner directions and side planes in the world
    const double W = (double)cam.film_w, H = (double)cam.film_h;
    const double eps_ab = 64.0 * U * (1.0 + tx * tx + ty * ty);
    const double ax0 = (1.0 - 2.0 * ((double)x1 + 1.0) / W) * tx - eps_ab, ax1 = (1.0 - 2.0 * (double)x0 / W) * tx + eps_ab;
    const double by0 = (1.0 - 2.0 * ((double)y1 + 1.0) / H) * ty - eps_ab, by1 = (1.0 - 2.0 * (double)y0 / H) * ty + eps_ab;
    const double amax = fmax(fabs(ax0), fabs(ax1)), bmax = fmax(fabs(by0), fabs(by1));
    const double inv_z_max = sqrt(amax * amax + bmax * bmax + 1.0) * (1.0 + 8.0 * U);  // 1 / dc.z, the longest over the rectangle
    const double s_max = near * inv_z_max;
    const double tmax_hi = (far - near) * inv_z_max * (1.0 + 8.0 * U);
    const double DELTA = 8.0 * U * (fabs(org[0]) + fabs(org[1]) + fabs(org[2]) + s_max);
    const double ca[4] = {ax0, ax1, ax1, ax0}, cb[4] = {by0, by0, by1, by1};  // the corners, going round
    double wd[4][3], ctr[3];
    for (int k = 0; k < 4; ++k)
        for (int r = 0; r < 3; ++r) wd[k][r] = M[r][0] * ca[k] + M[r][1] * cb[k] + M[r][2];
    for (int r = 0; r < 3; ++r) ctr[r] = M[r][0] * 0.5 * (ax0 + ax1) + M[r][1] * 0.5 * (by0 + by1) + M[r][2];
    double n[4][3];  // unit inward normals of the side planes through org
    for (int k = 0; k < 4; ++k) {
        const double *A = wd[k], *B = wd[(k + 1) & 3];
        double c[3] = {A[1] * B[2] - A[2] * B[1], A[2] * B[0] - A[0] * B[2], A[0] * B[1] - A[1] * B[0]};
        const double len = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        const double side = c[0] * ctr[0] + c[1] * ctr[1] + c[2] * ctr[2];
        if (!(len > 0.0) || side == 0.0) return true;
        const double sc = (side > 0.0 ? 1.0 : -1.0) / len;
        n[k][0] = c[0] * sc;
        n[k][1] = c[1] * sc;
        n[k][2] = c[2] * sc;
    }
    if (type == PBRT_PRIM_SPHERE) {
        const double c[3] = {(double)P.g[0] - org[0], (double)P.g[1] - org[1], (double)P.g[2] - org[2]};
        const double r = fabs((double)P.g[3]);
        const double dist = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        const double F = dist + s_max + DELTA;
        const double r_eff = sqrt(r * r + GAMMA * F * F);
        if (!(dist - s_max - DELTA >= 2.0 * r_eff)) return true;  // ray origins in or near the sphere
        const double lim = -(r_eff + DELTA) * (1.0 + 1e-9);
        for (int k = 0; k < 4; ++k)
            if (n[k][0] * c[0] + n[k][1] * c[1] + n[k][2] * c[2] < lim) return false;
        return true;
    }
    // ---- planar: the margin m of the float test in the primitive's own (u, v)
    double v0[3], e1[3], e2[3];
    for (int r = 0; r < 3; ++r) {
        v0[r] = (double)P.g[r] - org[r];  // relative to the apex
        e1[r] = (double)P.g[3 + r];
        e2[r] = (double)P.g[6 + r];
    }
    const double N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double l1 = sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]), l2 = sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
    const double lN = sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
    const double T = sqrt(v0[0] * v0[0] + v0[1] * v0[1] + v0[2] * v0[2]) + s_max + DELTA;
    const double eta_u = GAMMA * T * l2, eta_v = GAMMA * T * l1, eta_d = GAMMA * l1 * l2, eta_t = GAMMA * T * l1 * l2;
    const double ts_low = fabs(v0[0] * N[0] + v0[1] * N[1] + v0[2] * N[2]) - (s_max + DELTA) * lN - eta_t;
    if (!(ts_low > 0.0)) return true;
    const double det_low = ts_low / (tmax_hi * (1.0 + 4.0 * U)) - eta_d;
    if (!(det_low > 0.0)) return true;
    const double m = (fmax(eta_u, eta_v) + eta_d) / det_low;
    if (!(m <= TILE_CULL_M_CAP)) return true;
    // corners of the inflated primitive: parallelogram [-m, 1 + m]^2; triangle u, v >= -m, u + v <= 1 + 2 m
    const bool tri = type == PBRT_PRIM_TRIANGLE;
    const double hi = tri ? 1.0 + 3.0 * m : 1.0 + m;
    const double cu[4] = {-m, hi, -m, hi}, cv[4] = {-m, -m, hi, hi};
    const int nc = tri ? 3 : 4;
    const double lim = -DELTA * (1.0 + 1e-9) - 1e-12 * T;
    for (int k = 0; k < 4; ++k) {
        bool out = true;
        for (int q = 0; q < nc; ++q) {
            const double X[3] = {v0[0] + cu[q] * e1[0] + cv[q] * e2[0], v0[1] + cu[q] * e1[1] + cv[q] * e2[1],
                                 v0[2] + cu[q] * e1[2] + cv[q] * e2[2]};
            out = out && (n[k][0] * X[0] + n[k][1] * X[1] + n[k][2] * X[2] < lim);
        }
        if (out) return false;
    }
    return true;
}
