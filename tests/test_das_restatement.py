"""The f64 restatement of delay-and-sum (oracle/beamform.py::das_beamform), which the GPU tests measure the HIP kernel against, pinned
on the CPU: against a literal scalar loop over the definition of include/pbrt_hip.h at the range and aperture boundaries, and the
per-pixel tolerance of tests/das_util.py shown to flag the kernel bugs the GPU tests are meant to catch."""
import math

import numpy as np
import pytest

import das_util as du
from oracle import beamform as obf


def das_loop(data, tx, ex, x, z, fs, c, t0=0.0, f_number=1.0, interpolation="linear", compound="sum"):
    """the definition, one pixel, angle and element at a time: out[ix][iz] = sum_a sum_e data[a][e](s), s = (t_tx + d_e / c - t0) fs,
    t_tx = min_e' (tx[a][e'] + d_e' / c), d_e = |(x, z) - (x_e, 0)|; linear: floor(s) in [0, T - 1) or s == T - 1, the weight
    rounded to f32; nearest: round half to even into [0, T - 1]; receive aperture |x - x_e| <= z / (2 f_number) for f_number > 0"""
    data = np.asarray(data, np.float32)
    A, E, T = data.shape
    tx = [[float(v) for v in row] for row in du.f64(np.reshape(tx, (A, E)))]
    ex, gx, gz = [float(v) for v in du.f64(ex)], [float(v) for v in du.f64(x)], [float(v) for v in du.f64(z)]
    fs, c, t0, fn = (float(np.float32(v)) for v in (fs, c, t0, f_number or 0.0))
    out = np.zeros((len(gx), len(gz)))
    for ix, px in enumerate(gx):
        for iz, pz in enumerate(gz):
            acc = 0.0
            for a in range(A):
                t_tx = min(tx[a][e] + math.sqrt((px - ex[e]) ** 2 + pz ** 2) / c for e in range(E))
                for e in range(E):
                    if fn > 0 and abs(px - ex[e]) > pz / (2.0 * fn):
                        continue
                    s = (t_tx + math.sqrt((px - ex[e]) ** 2 + pz ** 2) / c - t0) * fs
                    tr = [float(v) for v in data[a, e]]
                    if interpolation == "nearest":
                        r = round(s)                       # Python rounds half to even, as rint does
                        if 0 <= r <= T - 1:
                            acc += tr[r]
                    else:
                        i0 = math.floor(s)
                        if 0 <= i0 < T - 1:
                            w = float(np.float32(s - i0))
                            acc += tr[i0] + w * (tr[i0 + 1] - tr[i0])
                        elif s == T - 1:
                            acc += tr[T - 1]
            out[ix, iz] = acc / A if compound == "mean" else acc
    return out


def _tiny(seed, A, E, T, nx=4, nz=5, delays="plane"):
    rng = np.random.default_rng(seed)
    c, fs = 1540.0, 10e6        # positions of about 2.5 - 10.5 samples, t0 moves them by -1.5 / +2.2
    data = rng.normal(size=(A, E, T)).astype(np.float32)
    ex = (3e-4 * (np.arange(E) - (E - 1) / 2)).astype(np.float32)
    if delays == "plane":
        th = np.deg2rad(np.linspace(-10, 10, A))
        tx = ex[None, :] * np.sin(th)[:, None] / c
    else:
        tx = rng.uniform(0, 4 / fs, size=(A, E))
    x = np.linspace(-6e-4, 6e-4, nx)
    z = np.linspace(2e-4, 8e-4, nz)
    return data, tx.astype(np.float32), ex, x, z, fs, c


@pytest.mark.parametrize("interp", ["linear", "nearest"])
@pytest.mark.parametrize("compound", ["sum", "mean"])
@pytest.mark.parametrize("f_number", [0.0, 0.8])
@pytest.mark.parametrize("t0", [0.0, 1.5e-7, -2.2e-7])
def test_restatement_equals_the_literal_loop(interp, compound, f_number, t0):
    for seed, (A, E, T, delays) in enumerate([(1, 1, 12, "plane"), (3, 5, 12, "plane"), (2, 4, 9, "random"), (3, 2, 3, "random")]):
        data, tx, ex, x, z, fs, c = _tiny(seed, A, E, T, delays=delays)
        kw = dict(t0=t0, f_number=f_number, interpolation=interp, compound=compound)
        ref = obf.das_beamform(data, tx, ex, x, z, fs, c, **kw)
        loop = das_loop(data, tx, ex, x, z, fs, c, **kw)
        assert np.allclose(ref, loop, rtol=1e-12, atol=1e-12), (A, E, T)
        if T >= 9:
            assert (loop != 0).any()


# Exact geometry: c = 1, fs = 1 and a 3-4-5 triangle -- the element at x = 0, the pixel at (3, 4): distance 5, first arrival 5 (the
# other element is kept out of the minimum by its delay), s = 10 - t0 with no rounding anywhere.
_EX = np.array([0.0, 1.0], np.float32)
_TX = np.array([[0.0, 100.0]], np.float32)


def _ramp(T):
    d = np.zeros((1, 2, T), np.float32)
    d[0, 0] = np.arange(1, T + 1)
    return d


@pytest.mark.parametrize("interp,T,t0,want", [
    ("linear", 12, 10.0, 1.0),      # s = 0: sample 0
    ("linear", 12, 10.25, 0.0),     # s = -0.25: outside
    ("linear", 12, -1.0, 12.0),     # s = 11 = T - 1: exactly the last sample
    ("linear", 12, -1.25, 0.0),     # s = 11.25: outside
    ("linear", 12, -0.5, 11.5),     # s = 10.5: between the last two
    ("nearest", 12, 10.5, 1.0),     # s = -0.5: rounds to (minus) zero, sample 0
    ("nearest", 12, 10.75, 0.0),    # s = -0.75: rounds to -1, outside
    ("nearest", 12, -1.5, 0.0),     # s = T - 0.5 = 11.5: rounds half to even, to 12, outside
    ("nearest", 11, -0.5, 11.0),    # s = T - 0.5 = 10.5: rounds half to even, to 10 = T - 1
    ("nearest", 12, 7.5, 3.0),      # s = 2.5: to 2 (half to even)
    ("nearest", 12, 6.5, 5.0),      # s = 3.5: to 4
])
def test_range_boundaries_are_pinned(interp, T, t0, want):
    data = _ramp(T)
    kw = dict(t0=t0, f_number=0.0, interpolation=interp)
    # (element 1's trace is zero: its term, at another position, adds nothing)
    ref = obf.das_beamform(data, _TX, _EX, [3.0], [4.0], 1.0, 1.0, **kw)
    loop = das_loop(data, _TX, _EX, [3.0], [4.0], 1.0, 1.0, **kw)
    assert ref[0, 0] == loop[0, 0] == want


_JUST_OUT = float(np.nextafter(np.float32(4.0), np.float32(5.0)))


@pytest.mark.parametrize("f_number,px", [(0.5, 4.0), (0.5, -4.0), (0.5, 5.0), (0.5, _JUST_OUT), (1.0, 2.0), (1.0, 3.0), (1.0, -1.0)])
def test_aperture_edge_is_inside(f_number, px):
    """|x - x_e| = z / (2 f#) exactly (z = 4) for one element: it is in the aperture; one float32 step further out it is not.
    Constant traces 1 (element 0) and 2 (element 1), zero delays, a long record: every term is in range, so the pixel's value says
    which elements are in the aperture"""
    T = 64
    data = np.zeros((1, 2, T), np.float32)
    data[0, 0], data[0, 1] = 1.0, 2.0
    tx = np.zeros((1, 2), np.float32)
    kw = dict(f_number=f_number, interpolation="linear")
    ref = obf.das_beamform(data, tx, _EX, [px], [4.0], 1.0, 1.0, **kw)
    loop = das_loop(data, tx, _EX, [px], [4.0], 1.0, 1.0, **kw)
    half = 4.0 / (2 * f_number)
    want = sum(w for w, e in zip((1.0, 2.0), _EX) if abs(px - float(e)) <= half)
    assert ref[0, 0] == loop[0, 0] == want
    assert any(abs(abs(px - float(e)) - half) <= 1e-6 for e in _EX)


def _mutants(data, tx, ex, fs, c, t0):
    """the restatement's operands as a kernel with one of the bugs the GPU tests look for would read them -> {name: (operands, pixels
    the bug reaches)} (None: every pixel that adds a term)"""
    A, E, _ = data.shape
    last = (A - 1) // 5 * 5          # the first angle of the last trip of 5
    drop = data.copy()
    drop[:, E // 3] = 0.0
    shifted = tx.copy()
    shifted[2] = tx[3]
    no_trip = data.copy()
    no_trip[last:] = 0.0
    zero_tx = tx.copy()
    zero_tx[last:] = 0.0
    return {
        "one element dropped": ((drop, tx, ex, fs, c, t0), _only(data.shape, e=E // 3)),
        "angle 3's delays for angle 2": ((data, shifted, ex, fs, c, t0), _only(data.shape, a=2)),
        "positions 1/8 sample late": ((data, tx, ex, fs, c, t0 - 0.125 / fs), None),
        "sound speed 1e-4 off": ((data, tx, ex, fs, c * (1 + 1e-4), t0), None),
        "last trip's data not read": ((no_trip, tx, ex, fs, c, t0), _only(data.shape, a=slice(last, None))),
        "last trip's angles zero": ((data, zero_tx, ex, fs, c, t0), _only(data.shape, a=slice(last, None))),
    }


def _only(shape, a=slice(None), e=slice(None)):
    w = np.zeros(shape, np.float32)
    w[a, e] = 1.0
    return w


def test_tolerance_flags_the_kernel_bugs_it_is_meant_to_catch():
    """11 plane-wave angles (two full trips of 5 and one of 1), 24 elements, f-number 1 and t0 != 0: every mutant of the operands
    moves more than 90 % of the pixels it reaches (98.7 - 100 % measured) by more than the per-pixel tolerance, and the tolerance
    leaves room for float32 rounding of the result ten times over"""
    rng = np.random.default_rng(17)
    A, E, T, c, fs, t0 = 11, 24, 600, 1540.0, 20e6, 2e-7
    data = rng.normal(size=(A, E, T)).astype(np.float32)
    ex = (3e-4 * (np.arange(E) - (E - 1) / 2)).astype(np.float32)
    th = np.deg2rad(np.linspace(-15, 15, A))
    tx = (ex[None, :] * np.sin(th)[:, None] / c).astype(np.float32)
    x, z = np.linspace(-5e-3, 5e-3, 16), np.linspace(2e-3, 1.4e-2, 20)
    kw = dict(t0=t0, f_number=1.0)
    ref = obf.das_beamform(data, tx, ex, x, z, fs, c, **kw)
    tol, n_terms = du.tolerance(data, tx, ex, x, z, fs, c, **kw)
    inside = n_terms > 0
    assert inside.mean() > 0.5 and (n_terms[inside] >= 11).all()
    # the tolerance is room for rounding, and not more: the reference rounded to float32 sits inside it, ten times over
    assert (np.abs(ref.astype(np.float32) - ref) * 10 <= tol + (ref == 0)).all()
    for name, ((d, t, e, f, cc, tt), reach) in _mutants(data, tx, ex, fs, c, t0).items():
        mut = obf.das_beamform(d, t, e, x, z, f, cc, t0=tt, f_number=1.0)
        where = inside if reach is None else obf.das_beamform(reach, tx, ex, x, z, fs, c, **kw) > 0
        assert where.sum() >= 20, name
        flagged = np.abs(mut - ref) > tol
        assert flagged[where].mean() > 0.9, (name, flagged[where].mean())
