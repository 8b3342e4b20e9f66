"""The convex (curved) transducer array of DESIGN.md D18 restated in float64 NumPy, for test_convex_array.py (CPU) and
test_gpu_convex_array.py (GPU).  The CPU oracle does not know the array; like cylinder_util.py and roughconductor_util.py this module
is the independent statement the kernels are held to:

  element_table    (x, z, nx, nz) per element, the geometry of CustomEmmitter.py:41-47 with the centre of curvature at the origin
  tx_delays        (x_e sin a + (z_e - R) cos a) / c: the plane wave along (sin a, 0, cos a), referenced to the apex (0, 0, R)
  plane_hit        first hit of a ray with a parallelogram (the plate of the acquisition tests)
  directivity      the receive weight of CustomIntegrator.py:289-304 against a given normal
  echo_model       for every (angle, transmit element, receive element): arrival time in samples, bin, directivity factor
  das              the delay-and-sum of include/pbrt_hip.h on an element table, with the aperture in the element's frame
"""
import numpy as np

import das_util as du


def element_table(n, radius, opening_deg):
    """[n, 4] float64: (R sin th, R cos th, sin th, cos th), th = linspace(-span / 2, span / 2, n)"""
    span = np.deg2rad(float(opening_deg))
    th = np.linspace(-span / 2, span / 2, int(n))
    return np.stack([radius * np.sin(th), radius * np.cos(th), np.sin(th), np.cos(th)], axis=1)


def tx_delays(elem, radius, angles_deg, c):
    """[n_angles, n] float64"""
    a = np.deg2rad(np.asarray(angles_deg, np.float64))[:, None]
    return (elem[None, :, 0] * np.sin(a) + (elem[None, :, 1] - radius) * np.cos(a)) / c


def linear_delays(x, angles_deg, c):
    a = np.deg2rad(np.asarray(angles_deg, np.float64))[:, None]
    return np.asarray(x, np.float64)[None, :] * np.sin(a) / c


def xf_point(M, p):
    M = np.asarray(M, np.float64).reshape(3, 4)
    return M[:, :3] @ np.asarray(p, np.float64) + M[:, 3]


def xf_vec(M, v):
    M = np.asarray(M, np.float64).reshape(3, 4)
    return M[:, :3] @ np.asarray(v, np.float64)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def plane_hit(o, d, p0, e1, e2):
    """first hit of the ray o + t d with the parallelogram p0 + u e1 + v e2, u, v in [0, 1] -> t, or None"""
    n = np.cross(e1, e2)
    den = float(np.dot(n, d))
    if den == 0.0:
        return None
    t = float(np.dot(n, p0 - o)) / den
    if t <= 0:
        return None
    q = o + t * d - p0
    G = np.array([[e1 @ e1, e1 @ e2], [e1 @ e2, e2 @ e2]])
    u, v = np.linalg.solve(G, np.array([q @ e1, q @ e2]))
    return t if (0 <= u <= 1 and 0 <= v <= 1) else None


def directivity(alpha, am, ac):
    """CustomIntegrator.py:289-304: 1 up to the main beam angle, a ramp down to 0 at the cut-off"""
    return 1.0 if alpha <= am else ((ac - alpha) / (ac - am) if alpha <= ac else 0.0)


def echo_model(M, elem, radius, angles_deg, c, fs, am_deg, ac_deg, plate, emitter_psi_deg=None, axis_normal=False):
    """One bounce of the deterministic primary rays on a plate (p0, e1, e2), for every (angle a, transmit element e, receive element r):
    -> dict of [A, E, E] arrays: s (arrival in samples: (t_emit + t_hit + |p - target| / c) fs), alpha (directivity angle against the
    receive element's normal -- against the array axis with axis_normal, the WRONG model a test wants to tell apart), D (the factor),
    and hit [A, E].  t_emit = tx_delays, or with emitter_psi_deg (CustomEmitter rays without jitter, steered to psi whatever the angle
    index): the emitter's own -(x_e sin psi) / c (CustomEmmitter.py:93) and direction (sin psi, 0, cos psi)."""
    A, E = len(angles_deg), len(elem)
    am, ac = np.deg2rad(am_deg), np.deg2rad(ac_deg)
    tx = tx_delays(elem, radius, angles_deg, c)
    pos = [xf_point(M, [e[0], 0.0, e[1]]) for e in elem]
    nrm = [unit(xf_vec(M, [0.0, 0.0, 1.0])) if axis_normal else unit(xf_vec(M, [e[2], 0.0, e[3]])) for e in elem]
    s = np.full((A, E, E), np.nan)
    alpha = np.full((A, E, E), np.nan)
    D = np.zeros((A, E, E))
    hit = np.zeros((A, E), bool)
    for a in range(A):
        ang = np.deg2rad(float(angles_deg[a] if emitter_psi_deg is None else emitter_psi_deg))
        d = unit(xf_vec(M, [np.sin(ang), 0.0, np.cos(ang)]))
        for e in range(E):
            t_emit = tx[a, e] if emitter_psi_deg is None else -(elem[e, 0] * np.sin(ang)) / c
            t = plane_hit(pos[e], d, *plate)
            if t is None:
                continue
            hit[a, e] = True
            p = pos[e] + t * d
            for r in range(E):
                tv = pos[r] - p
                dist = np.linalg.norm(tv)
                s[a, e, r] = (t_emit + t / c + dist / c) * fs
                alpha[a, e, r] = abs(np.arccos(np.clip(np.dot(nrm[r], -tv / dist), -1.0, 1.0)))
                D[a, e, r] = directivity(alpha[a, e, r], am, ac)
    return dict(s=s, alpha=alpha, D=D, hit=hit, ac=ac)


def predicted_words(model, T, tie=1e-3, cut=1e-4):
    """-> (sure, unsure, left_out_share): sets of channel words (a, r, bin).  `sure`: words a kept pair deposits into; `unsure`: the
    candidate bins of the pairs left out -- arrival within `tie` samples of a rounding tie (both neighbours), or directivity angle
    within `cut` rad of the cut-off; the share of pairs left out among those whose ray hits"""
    s, alpha, D, ac = model["s"], model["alpha"], model["D"], model["ac"]
    sure, unsure = set(), set()
    n_pairs = n_out = 0
    A, E, _ = s.shape
    for a in range(A):
        for e in range(E):
            if not model["hit"][a, e]:
                continue
            for r in range(E):
                n_pairs += 1
                v = s[a, e, r]
                near_tie = abs(v - np.floor(v) - 0.5) < tie
                near_cut = abs(alpha[a, e, r] - ac) < cut
                bins = {int(np.floor(v)), int(np.floor(v)) + 1} if near_tie else {int(np.rint(v))}
                bins = {b for b in bins if 0 <= b < T}
                if near_tie or near_cut:
                    n_out += 1
                    unsure |= {(a, r, b) for b in bins}
                elif D[a, e, r] != 0.0:
                    sure |= {(a, r, b) for b in bins}
    return sure, unsure, n_out / max(n_pairs, 1)


def words_of(buf):
    """the non-zero words of a channel buffer [A, E, T] as a set of (a, r, bin)"""
    return {tuple(int(v) for v in w) for w in np.argwhere(np.asarray(buf) != 0)}


def das(data, tx, elem, x, z, fs, c, t0=0.0, f_number=1.0, interpolation="linear", compound="sum"):
    """delay-and-sum on an element table in float64 (include/pbrt_hip.h pbrt_das_beamform_probe): every operand read as float32 first.
    -> (image [nx, nz], n_terms, excluded, ties) with the meaning of das_util.contributions: a pixel is `excluded` when one of its
    pairs lies within du.EDGE_SAMPLES of a range boundary or within du.EDGE_APERTURE (relative to the depth d_n) of the aperture edge."""
    data = du.f64(data)
    A, E, T = data.shape
    tx, el, gx, gz = du.f64(tx).reshape(A, E), du.f64(elem).reshape(E, 4), du.f64(x).ravel(), du.f64(z).ravel()
    c, fs, t0, fn = float(np.float32(c)), float(np.float32(fs)), float(np.float32(t0)), float(np.float32(f_number or 0.0))
    X, Z = np.meshgrid(gx, gz, indexing="ij")
    dx = X[None] - el[:, 0, None, None]
    dz = Z[None] - el[:, 1, None, None]
    dist = np.sqrt(dx * dx + dz * dz)
    dn = dx * el[:, 2, None, None] + dz * el[:, 3, None, None]
    dt = dx * el[:, 3, None, None] - dz * el[:, 2, None, None]
    if fn > 0:
        use = (dn > 0) & (2.0 * fn * np.abs(dt) <= dn)
        edge = (np.abs(2.0 * fn * np.abs(dt) - dn) < du.EDGE_APERTURE * np.abs(dn) + 1e-300) | (np.abs(dn) < 1e-300)
    else:
        use = np.ones(dist.shape, bool)
        edge = np.zeros(dist.shape, bool)
    img = np.zeros(X.shape)
    n_terms = np.zeros(X.shape)
    excluded = edge.any(axis=0)
    ties = np.zeros(X.shape, bool)
    ee = np.arange(E)[:, None, None]
    for a in range(A):
        t_tx = np.min(tx[a][:, None, None] + dist / c, axis=0)
        s = (t_tx[None] + dist / c - t0) * fs
        if interpolation == "nearest":
            r = np.rint(s)
            ok = (r >= 0) & (r <= T - 1) & use
            near = (np.abs(s + 0.5) < du.EDGE_SAMPLES) | (np.abs(s - (T - 0.5)) < du.EDGE_SAMPLES)
            ties |= (ok & (np.abs(s - np.floor(s) - 0.5) < du.EDGE_SAMPLES)).any(axis=0)
            idx = np.clip(r, 0, T - 1).astype(int)
            val = data[a][ee, idx]
        else:
            f = np.floor(s)
            ok = (((f >= 0) & (f < T - 1)) | (s == T - 1)) & use
            near = (np.abs(s) < du.EDGE_SAMPLES) | (np.abs(s - (T - 1)) < du.EDGE_SAMPLES)
            i0 = np.clip(f, 0, T - 1).astype(int)
            i1 = np.clip(i0 + 1, 0, T - 1)
            w = s - f
            v0, v1 = data[a][ee, i0], data[a][ee, i1]
            val = v0 + w * (v1 - v0)
        excluded |= (near & use).any(axis=0)
        img += np.where(ok, val, 0.0).sum(axis=0)
        n_terms += ok.sum(axis=0)
    if compound == "mean":
        img /= A
    return img, n_terms, excluded, ties


def das_tolerance(data, tx, elem, x, z, fs, c, **kw):
    """the per-pixel tolerance of tests/das_util.py, unchanged: (K_SUM n_terms + K_POS) 2^-24 das(M), M = du.abs_envelope(data)"""
    bound, n_terms, _, _ = das(du.abs_envelope(data), tx, elem, x, z, fs, c, **kw)   # (n_terms does not depend on the data)
    return (du.K_SUM * n_terms + du.K_POS) * du.U32 * bound, n_terms
