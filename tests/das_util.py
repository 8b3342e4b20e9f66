"""Shared by the delay-and-sum tests (test_das_restatement.py on the CPU, test_gpu_das_shapes.py on the GPU): which (angle, element)
pairs a pixel sums by the rules of oracle/beamform.py, and the per-pixel tolerance a float32 kernel is held to against that f64
restatement."""
import numpy as np

from oracle import beamform as obf

U32 = 2.0 ** -24     # unit roundoff of float32
K_SUM = 1.0          # f32 sum of n terms in any order: error <= (n - 1) u sum |term|
K_POS = 16.0         # per term: the position fraction kept in f32 (<= 2.5 u samples) times the slope (<= 2 max|v|), the
#                      f32 difference and multiply-add of the interpolation (<= 3 u max|v|), the final rounding -- 9 u, doubled
EDGE_SAMPLES = 1e-6  # a position this close to a range boundary may fall on either side of it in another order of f64 operations
EDGE_APERTURE = 1e-9  # (relative to z) the same for the receive-aperture edge


def f64(a):
    """the restatement reads every operand as float32 first"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def positions(tx, ex, x, z, fs, c, t0):
    """-> for every angle a: (s [E, nx, nz] sample positions, dx [E, nx, nz] lateral offsets), as oracle/beamform.py forms them"""
    tx, ex, gx, gz = f64(tx), f64(ex), f64(x).ravel(), f64(z).ravel()
    c, fs, t0 = float(np.float32(c)), float(np.float32(fs)), float(np.float32(t0))
    X, Z = np.meshgrid(gx, gz, indexing="ij")
    dx = X[None] - ex[:, None, None]
    dist = np.sqrt(dx ** 2 + Z[None] ** 2)
    for a in range(tx.shape[0]):
        t_tx = np.min(tx[a][:, None, None] + dist / c, axis=0)
        yield (t_tx + dist / c - t0) * fs, dx


def first_arrival(tx, ex, x, z, c):
    """t_tx[a, ix, iz] = min_e (tx[a, e] + |(x, z) - (x_e, 0)| / c) in f64"""
    tx, ex, gx, gz = f64(np.atleast_2d(tx)), f64(ex), f64(x).ravel(), f64(z).ravel()
    c = float(np.float32(c))
    X, Z = np.meshgrid(gx, gz, indexing="ij")
    dist = np.sqrt((X[None] - ex[:, None, None]) ** 2 + Z[None] ** 2)
    return np.stack([np.min(tx[a][:, None, None] + dist / c, axis=0) for a in range(tx.shape[0])])


def contributions(tx, ex, x, z, T, fs, c, t0=0.0, f_number=1.0, interpolation="linear", weights=()):
    """-> (sums, excluded, ties): sums[k][ix, iz] = sum of weights[k][a, e] over the pairs (a, e) that pixel (ix, iz) adds, by the
    range and aperture rules of oracle/beamform.py, in f64; excluded[ix, iz]: some pair lies within EDGE_SAMPLES of a range boundary
    or within EDGE_APERTURE z of the aperture edge, where a kernel may take the other side; ties[ix, iz] (nearest): some pair it
    adds lies within EDGE_SAMPLES of a half sample, where another order of f64 operations may round to the other neighbour"""
    tx = np.atleast_2d(np.asarray(tx))
    z64 = f64(z).ravel()[None, None, :]
    fn = float(np.float32(f_number or 0.0))
    sums = [np.zeros((len(np.ravel(x)), len(np.ravel(z)))) for _ in weights]
    excluded = np.zeros((len(np.ravel(x)), len(np.ravel(z))), bool)
    ties = excluded.copy()
    for a, (s, dx) in enumerate(positions(tx, ex, x, z, fs, c, t0)):
        if fn > 0:
            half = z64 / (2.0 * fn)
            use = np.abs(dx) <= half
            excluded |= (np.abs(np.abs(dx) - half) < EDGE_APERTURE * np.abs(z64)).any(axis=0)
        else:
            use = np.ones(s.shape, bool)
        if interpolation == "nearest":
            r = np.rint(s)
            ok = (r >= 0) & (r <= T - 1)
            near = (np.abs(s + 0.5) < EDGE_SAMPLES) | (np.abs(s - (T - 0.5)) < EDGE_SAMPLES)
            ties |= (ok & use & (np.abs(s - np.floor(s) - 0.5) < EDGE_SAMPLES)).any(axis=0)
        else:
            f = np.floor(s)
            ok = ((f >= 0) & (f < T - 1)) | (s == T - 1)
            near = (np.abs(s) < EDGE_SAMPLES) | (np.abs(s - (T - 1)) < EDGE_SAMPLES)
        ok &= use
        excluded |= (near & use).any(axis=0)
        for k, w in enumerate(weights):
            sums[k] += np.tensordot(np.asarray(w, np.float64)[a], ok, axes=(0, 0))
    return sums, excluded, ties


def abs_envelope(data):
    """M[a, e, t] = max |data[a, e, t']| over |t' - t| <= 1: linear interpolation of M anywhere in [t, t + 1] is at least
    max(|data[t]|, |data[t + 1]|), so the restatement run on M bounds sum_terms max(|v0|, |v1|) from above -- the size of every
    term and half of every slope"""
    m = np.abs(np.asarray(data, np.float32))
    out = m.copy()
    out[..., 1:] = np.maximum(out[..., 1:], m[..., :-1])
    out[..., :-1] = np.maximum(out[..., :-1], m[..., 1:])
    return out


def tolerance(data, tx, ex, x, z, fs, c, t0=0.0, f_number=1.0, interpolation="linear", compound="sum"):
    """per-pixel tolerance of a float32 delay-and-sum against obf.das_beamform on the same operands:
        tol = (K_SUM n_terms + K_POS) 2^-24 obf(M)[pixel],   M = abs_envelope(data)
    n_terms: the (angle, element) pairs the pixel adds.  A pixel that adds none must be exactly 0."""
    kw = dict(t0=t0, f_number=f_number, interpolation=interpolation)
    A, E, T = np.shape(data)
    n_terms = obf.das_beamform(np.ones((A, E, T), np.float32), tx, ex, x, z, fs, c, compound="sum", **kw)
    bound = obf.das_beamform(abs_envelope(data), tx, ex, x, z, fs, c, compound=compound, **kw)
    return (K_SUM * n_terms + K_POS) * U32 * bound, n_terms
