"""Sector scans restated in NumPy for test_scan_restatement.py (CPU) and test_gpu_scan.py (GPU), sharing no text with
the kernels.

  pixels            the pixel tables of a polar scan: x = ox + rho sin(theta), z = oz + rho cos(theta) in float64, rounded once
  sector            the sector the GPU test lays over a walk case (tests/walk_cases.py): (n_theta, n_rho) = the case's (nx, nz), rho = its z
  per_pixel         a restatement that takes axes x [nx], z [nz], evaluated pixel by pixel on one-pixel axes: the beamformers'
                    restatements (das_util, convex_util, nlbf_util, iq_util) are functions of a pixel's position only, so a pixel
                    table needs no restatement of its own
  scan_convert      the scan conversion of include/pbrt_hip.h in float64, or with the three interpolations in np.float32 (the floor)

The bound of the scan conversion.  A pixel's value is three interpolations v0 + w (v1 - v0) of samples no larger than M = max |corner|.
One interpolation in float32 rounds the difference (|v1 - v0| <= 2 M: 2 u M, times w <= 1) and the multiply-add (u M): 3 u M.  The two
along rho enter the one along theta with weights that add up to 1 (3 u M), which adds its own 3 u M.  Each weight is a float64 rounded
once to float32 (u w, times a difference <= 2 M: 2 u M along rho, 2 u M along theta).  That is 10 u M; doubled for the second-order
terms, as das_util doubles K_POS: C_SC = 20.  It is used only where the float32 floor is zero (a constant image, say); elsewhere the
bound is the project's four times the floor."""
import functools

import numpy as np

import convex_util as cu
import das_util as du
import iq_util as iu
import nlbf_util as nu
from oracle import beamform as obf
from walk_cases import C0, CASES, T, geometry

C_SC = 20.0
EDGE_UV = 1e-6      # an output pixel with u or v this close to 0 or to n - 1 may fall on either side in another order of f64 operations
F_D = 2.5e6         # the demodulation frequency of the I/Q cases (test_gpu_iq.py's)


def pixels(rhos, thetas, origin=(0.0, 0.0)):
    th, rho = np.asarray(thetas, np.float64)[:, None], np.asarray(rhos, np.float64)[None, :]
    return (origin[0] + rho * np.sin(th)).astype(np.float32), (origin[1] + rho * np.cos(th)).astype(np.float32)


def sector_axes(name):
    """(thetas [n_theta] radians, rhos [n_rho]) of the sector over a walk case: +-20 degrees, 0.137 degrees off axis, on the line of
    elements; +-25 degrees around the centre of curvature on the curved array; rho is the case's z"""
    g = geometry(name)
    n_theta = len(g["x"])
    if np.ndim(g["elem"]) == 2:
        thetas = np.radians(np.linspace(-25.0, 25.0, n_theta))
    else:
        thetas = np.radians(np.linspace(-20.0, 20.0, n_theta) + 0.137)
    return thetas, g["z"].astype(np.float64)


def per_pixel(fn, px, pz):
    """fn(x [1], z [1]) -> an array [..., 1, 1] or a tuple of such; evaluated at every pixel of the tables and stacked to [..., n0, n1]"""
    n0, n1 = px.shape
    first = fn(px[0, :1], pz[0, :1])
    many = isinstance(first, tuple)
    outs = None
    for i in range(n0):
        for j in range(n1):
            r = fn(px[i, j:j + 1], pz[i, j:j + 1])
            r = r if many else (r,)
            if outs is None:
                outs = [np.empty(np.shape(v)[:-2] + (n0, n1), np.asarray(v).dtype) for v in r]
            for o, v in zip(outs, r):
                o[..., i, j] = np.asarray(v)[..., 0, 0]
    return tuple(outs) if many else outs[0]


@functools.lru_cache(maxsize=None)
def sector(name, thetas_deg=None):
    """a walk case on its sector (thetas_deg: another (lo, hi) in degrees): the case's tables, px / pz, left_out and n_a [A, n0, n1]"""
    g = dict(geometry(name))
    thetas, rhos = sector_axes(name)
    if thetas_deg is not None:
        thetas = np.radians(np.linspace(thetas_deg[0], thetas_deg[1], len(thetas)))
    px, pz = pixels(rhos, thetas)
    kw = g["kw"]
    left_out, n_a = per_pixel(lambda x, z: nu.margins(g["tx"], g["elem"], x, z, T, g["fs"], C0, f_number=kw["f_number"],
                                                      interpolation=kw["interpolation"]), px, pz)
    g.update(px=px, pz=pz, thetas=thetas, rhos=rhos, left_out=left_out, n_a=n_a)
    return g


def rf_data(name):
    g = geometry(name)
    rng = np.random.default_rng(sum(map(ord, name)) * 11 + 3)
    return rng.standard_normal((g["A"], g["E"], T)).astype(np.float32)


def iq_data(name):
    g = geometry(name)
    rng = np.random.default_rng(sum(map(ord, name)) * 13 + 5)
    return (rng.standard_normal((g["A"], g["E"], T)) + 1j * rng.standard_normal((g["A"], g["E"], T))).astype(np.complex64)


def das_reference(g, data, literal=False):
    """delay-and-sum on the pixel tables in float64 and the project's per-pixel tolerance -> (image, tol, n_terms), each [n0, n1].
    The tolerance is das_util.tolerance's / convex_util.das_tolerance's: (K_SUM n_terms + K_POS) 2^-24 das(M), M = du.abs_envelope(data).
    literal: those two functions themselves, pixel by pixel (oracle/beamform.py's loops take tens of milliseconds per one-pixel call:
    test_scan_restatement.py does it on the small cases); else the same formula with nlbf_util's delay-and-sum, which states the
    same rules -- the CPU test holds the two to each other."""
    args, tail = (g["tx"], g["elem"]), (g["fs"], C0)
    table = np.ndim(g["elem"]) == 2
    if literal:
        def one(x, z):
            if table:
                tol, n_terms = cu.das_tolerance(data, *args, x, z, *tail, **g["kw"])
                return cu.das(data, *args, x, z, *tail, **g["kw"])[0], tol, n_terms
            tol, n_terms = du.tolerance(data, *args, x, z, *tail, **g["kw"])
            return obf.das_beamform(data, *args, x, z, *tail, **g["kw"]), tol, n_terms
    else:
        M = du.abs_envelope(data)

        def one(x, z):
            img, _ = nu.beamform("das", data, *args, x, z, *tail, **g["kw"])
            bound, _ = nu.beamform("das", M, *args, x, z, *tail, **g["kw"])
            n_terms = sum(ok.sum(axis=0) for _, ok in nu.delayed(M, *args, x, z, *tail, f_number=g["kw"]["f_number"],
                                                                interpolation=g["kw"]["interpolation"])).astype(np.float64)
            return img, (du.K_SUM * n_terms + du.K_POS) * du.U32 * bound, n_terms
    return per_pixel(one, g["px"], g["pz"])


def nl_reference(g, data, method, p):
    """p-DAS / F-DMAS on the pixel tables -> (float64 image, B, float32 image)"""
    def one(x, z):
        ref, B = nu.beamform(method, data, g["tx"], g["elem"], x, z, g["fs"], C0, p=p, **g["kw"])
        f32, _ = nu.beamform(method, data, g["tx"], g["elem"], x, z, g["fs"], C0, p=p, dtype=np.float32, **g["kw"])
        return ref, B, f32.astype(np.float64)
    return per_pixel(one, g["px"], g["pz"])


def iq_reference(g, iq):
    def one(x, z):
        ref, B = iu.iq_beamform(iq, g["tx"], g["elem"], x, z, g["fs"], C0, F_D, **g["kw"])
        f32, _ = iu.iq_beamform(iq, g["tx"], g["elem"], x, z, g["fs"], C0, F_D, dtype=np.float32, **g["kw"])
        return ref, B, f32.astype(np.complex128)
    return per_pixel(one, g["px"], g["pz"])


# ---- scan conversion ----------------------------------------------------------------------------------------------------------
def polar_coordinates(theta0, dtheta, rho0, drho, origin, x, z):
    """(u, v) [nx, nz]: the fractional indices of every output pixel along theta and along rho, float32 axes read as float64"""
    X, Z = np.meshgrid(du.f64(x).ravel(), du.f64(z).ravel(), indexing="ij")
    dx, dz = X - origin[0], Z - origin[1]
    return (np.arctan2(dx, dz) - theta0) / dtheta, (np.sqrt(dx * dx + dz * dz) - rho0) / drho


def scan_convert(src, theta0, dtheta, rho0, drho, origin, x, z, fill=0.0, dtype=np.float64):
    """-> dict(out [nx, nz], inside, edge, i, j, scale): out in `dtype` arithmetic (the weights are float32 values in either case),
    `fill` outside; edge: u or v within EDGE_UV of 0 or of n - 1; (i, j) the lower corner of the cell an inside pixel reads (its
    read set is the four samples (i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1)); scale = max |corner|"""
    src = np.asarray(src, np.float32)
    nt, nr = src.shape
    u, v = polar_coordinates(theta0, dtheta, rho0, drho, origin, x, z)
    inside = (u >= 0) & (u <= nt - 1) & (v >= 0) & (v <= nr - 1)
    edge = (np.minimum(np.abs(u), np.abs(u - (nt - 1))) < EDGE_UV) | (np.minimum(np.abs(v), np.abs(v - (nr - 1))) < EDGE_UV)
    i = np.clip(np.floor(np.where(inside, u, 0)), 0, nt - 2).astype(int)
    j = np.clip(np.floor(np.where(inside, v, 0)), 0, nr - 2).astype(int)
    wu, wv = (u - i).astype(np.float32).astype(dtype), (v - j).astype(np.float32).astype(dtype)
    s = src.astype(dtype)
    c00, c01, c10, c11 = s[i, j], s[i, j + 1], s[i + 1, j], s[i + 1, j + 1]
    with np.errstate(invalid="ignore", over="ignore"):
        a = c00 + wv * (c01 - c00)
        b = c10 + wv * (c11 - c10)
        val = a + wu * (b - a)
    out = np.where(inside, val, dtype(fill)).astype(dtype)
    with np.errstate(invalid="ignore"):
        scale = np.max(np.abs(np.stack([c00, c01, c10, c11]).astype(np.float64)), axis=0)
    return dict(out=out, inside=inside, edge=edge, i=i, j=j, scale=scale)


def reads(conv, ti, tj):
    """[nx, nz]: the inside pixels whose four corners include the sample (ti, tj)"""
    i, j = conv["i"], conv["j"]
    return conv["inside"] & ((i == ti) | (i + 1 == ti)) & ((j == tj) | (j + 1 == tj))


def scan_convert_bound(src, theta0, dtheta, rho0, drho, origin, x, z):
    """-> (float64 restatement dict, per-pixel bound, the float32 floor): four times the floor on the scale max |corner|, or
    C_SC 2^-24 on that scale where the floor is zero"""
    ref = scan_convert(src, theta0, dtheta, rho0, drho, origin, x, z)
    f32 = scan_convert(src, theta0, dtheta, rho0, drho, origin, x, z, dtype=np.float32)
    use = ref["inside"] & (ref["scale"] > 0)
    floor = float((np.abs(f32["out"].astype(np.float64) - ref["out"])[use] / ref["scale"][use]).max()) if use.any() else 0.0
    rel = 4.0 * floor if floor > 0 else C_SC * du.U32
    return ref, rel * ref["scale"], floor
