"""k_das_beamform and k_das_first_arrival (csrc/kernels_beamform.h) at the shapes the 5 x 64 probe never reaches: a second trip of
angles (A > 5), a second block of elements (E > 64), a ragged share of the four waves (E % 4 != 0, E < 4), focused and random
transmit delays, permuted elements, z rows at and below 0, t0 != 0, grids that are not whole 8 x 8 tiles and a z-tile count that
the 16 XCD bands do not divide.  Every case is checked four ways:
  a. constant traces with integer weights: every term is exact, so the image must equal, bit for bit, the sum of the weights over
     the (angle, element) pairs oracle/beamform.py's rules add -- the count, the angle index and the element index in turn;
  b. random traces against oracle/beamform.py at the per-pixel tolerance of tests/das_util.py;
  c. an output buffer filled with NaN first: every pixel is written (including the tiles that see no element), also on a second call
     into the same buffer;
  d. the table path (das_first_arrival, then das_beamform(table=...)) equals the plain call bit for bit, and the table equals the
     f64 first arrival."""
import numpy as np
import pytest

import das_util as du
from oracle import beamform as obf

pytestmark = pytest.mark.gpu

PITCH, C = 3e-4, 1540.0

# (A, E, T, nx, nz, delays, permuted, interpolation, compound, f_number, t0 as a fraction of the longest time, z rows)
CASES = [
    (1, 1, 2, 1, 7, "plane", False, "linear", "sum", 0.0, 0.0, "pos"),
    (4, 2, 3, 7, 8, "focused", False, "linear", "mean", 1.0, 0.1, "pos"),
    (5, 3, 257, 8, 9, "random", True, "nearest", "sum", 0.0, -0.1, "neg"),
    (6, 5, 257, 9, 127, "plane", False, "linear", "sum", 1.5, 0.05, "pos"),
    (10, 63, 10000, 9, 8 * 37 + 3, "plane", False, "linear", "sum", 1.0, 0.0, "pos"),
    (11, 128, 10000, 127, 9, "plane", False, "linear", "mean", 1.0, -0.05, "pos"),
    (64, 192, 257, 9, 17, "random", True, "linear", "mean", 0.0, 0.1, "pos"),
    (64, 65, 3, 8, 8, "focused", True, "nearest", "mean", 1.0, -0.1, "pos"),
    (1, 64, 10000, 127, 7, "focused", False, "nearest", "sum", 1.0, 0.1, "pos"),
    (6, 130, 257, 7, 127, "focused", True, "linear", "sum", 1.0, -0.1, "pos"),
    (5, 64, 10000, 8, 127, "plane", False, "linear", "sum", 1.0, 0.0, "pos"),
    (11, 2, 2, 127, 1, "random", False, "linear", "sum", 0.0, 0.0, "neg"),
    (4, 192, 2, 1, 127, "plane", True, "nearest", "mean", 0.0, 0.05, "neg"),
    (10, 3, 257, 8, 8 * 37 + 3, "random", False, "nearest", "sum", 1.0, -0.05, "pos"),
    (5, 1, 3, 9, 9, "plane", False, "nearest", "mean", 0.0, 0.1, "neg"),
]


def _case_id(cs):
    A, E, T, nx, nz, dl, perm, interp, comp, fn, t0f, zm = cs
    return f"A{A}-E{E}-T{T}-{nx}x{nz}-{dl}{'-perm' if perm else ''}-{interp}-{comp}-f{fn}-t0{t0f:+}-z{zm}"


def _geometry(seed, A, E, T, nx, nz, delays, permuted, t0_frac, zrows):
    """-> (tx [A, E], ex [E], x [nx], z [nz], fs, t0): an f32 probe of pitch 0.3 mm, a grid reaching past the array on both sides (some
    tiles see no element at f-number > 0), fs such that the deepest pixels lie past the end of the record, t0 a fraction of it"""
    rng = np.random.default_rng(seed)
    ex = (PITCH * (np.arange(E) - (E - 1) / 2)).astype(np.float32)
    if permuted:
        ex = ex[rng.permutation(E)]
    half = PITCH * E / 2 + 0.01
    x = np.linspace(-half, half, nx) if nx > 1 else np.array([0.37 * PITCH])
    if zrows == "neg":      # rows at and below 0 (z = 0 exactly among them)
        dz = np.float32(2.5e-4)
        z = (dz * (np.arange(nz) - min(2, nz - 1))).astype(np.float32)
    else:
        z = np.linspace(1e-3, 3e-2, nz) if nz > 1 else np.array([1.2e-2])
    if delays == "plane":
        th = np.deg2rad(np.linspace(-15, 15, A))
        tx = ex[None, :].astype(np.float64) * np.sin(th)[:, None] / C
    elif delays == "focused":  # a virtual point source 2 cm in front of the array, swept across it
        xf = np.linspace(-PITCH * E / 2, PITCH * E / 2, A)
        r = np.hypot(ex[None, :] - xf[:, None], 0.02)
        tx = (r.max(axis=1, keepdims=True) - r) / C
    else:
        tx = rng.uniform(0.0, 2e-6, size=(A, E))
    tx = tx.astype(np.float32)
    longest = 2 * np.hypot(np.abs(x).max() + PITCH * E, np.abs(z).max()) / C + float(tx.max())
    fs = 1.3 * (T - 1) / longest
    return tx, ex, x.astype(np.float32), z.astype(np.float32), fs, t0_frac * longest


def _nan_buffer(mi, cx, shape, dtype=np.float32):
    return mi.DeviceBuffer.from_host(cx, np.full(shape, np.nan, dtype))


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_das_at_shapes_beyond_the_probe(mi, case):
    A, E, T, nx, nz, delays, permuted, interp, compound, fnum, t0_frac, zrows = case
    seed = CASES.index(case)
    tx, ex, x, z, fs, t0 = _geometry(seed, A, E, T, nx, nz, delays, permuted, t0_frac, zrows)
    kw = dict(t0=t0, f_number=fnum, interpolation=interp, compound=compound)
    cx = mi.default_context()
    d_x, d_z = mi.DeviceBuffer.from_host(cx, x), mi.DeviceBuffer.from_host(cx, z)

    # d. the first-arrival table against f64, then kept for the table path
    tab = mi.das_first_arrival(tx, ex, d_x, d_z, C)
    t_ref = du.first_arrival(tx, ex, x, z, C)
    t_got = tab.numpy()
    assert t_got.shape == (A, nx, nz)
    assert (np.abs(t_got - t_ref) <= 1e-15 * (np.abs(t_ref) + np.abs(du.f64(tx)).max())).all()

    # a. constant traces: the count, which angle, which element -- exact
    ai, ei = np.meshgrid(np.arange(A), np.arange(E), indexing="ij")
    weights = [np.ones((A, E)), ai + 1.0, ei + 1.0]
    sums, excluded, ties = du.contributions(tx, ex, x, z, T, fs, C, t0=t0, f_number=fnum, interpolation=interp, weights=weights)
    assert excluded.mean() < 0.01, excluded.sum()
    assert sums[0].max() > 0, "the case adds no term anywhere"
    keep = ~excluded
    out = _nan_buffer(mi, cx, (nx, nz))
    out_tab = _nan_buffer(mi, cx, (nx, nz))
    d_data = mi.DeviceBuffer(cx, (A, E, T))
    for k, (w, want) in enumerate(zip(weights, sums)):
        d_data.upload(np.broadcast_to(w.astype(np.float32)[:, :, None], (A, E, T)))
        want = (want / A if compound == "mean" else want).astype(np.float32)
        got = mi.das_beamform(d_data, tx, ex, d_x, d_z, fs, C, out=out, **kw).numpy()
        got_tab = mi.das_beamform(d_data, tx, ex, d_x, d_z, fs, C, out=out_tab, table=tab, **kw).numpy()
        if k == 0:   # c. the NaN the buffers held is gone: every pixel written, by the plain and the table path
            assert not np.isnan(got).any() and not np.isnan(got_tab).any()
        bad = keep & (got != want)
        assert not bad.any(), (k, np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])
        assert np.array_equal(got_tab, got)

    # b. random traces against the restatement at the per-pixel tolerance, into the buffers used above (c: a second call)
    rng = np.random.default_rng(1000 + seed)
    data = rng.normal(size=(A, E, T)).astype(np.float32)
    d_data.upload(data)
    got = mi.das_beamform(d_data, tx, ex, d_x, d_z, fs, C, out=out, **kw).numpy()
    got_tab = mi.das_beamform(d_data, tx, ex, d_x, d_z, fs, C, out=out_tab, table=tab, **kw).numpy()
    fresh = mi.das_beamform(d_data, tx, ex, d_x, d_z, fs, C, out=_nan_buffer(mi, cx, (nx, nz)), **kw).numpy()
    host = mi.das_beamform(data, tx, ex, x, z, fs, C, **kw)
    assert np.array_equal(got, fresh) and np.array_equal(got_tab, got) and np.array_equal(host, got)   # d. bit for bit
    ref = obf.das_beamform(data, tx, ex, x, z, fs, C, **kw)
    tol, n_terms = du.tolerance(data, tx, ex, x, z, fs, C, **kw)
    keep &= ~ties
    assert keep.mean() > 0.97
    err = np.abs(got.astype(np.float64) - ref)
    over = keep & (err > tol)
    assert not over.any(), (np.argwhere(over)[:5].tolist(), err[over][:5], tol[over][:5])
    assert (got[keep & (n_terms == 0)] == 0).all()
    live = keep & (n_terms > 0)
    print(f"\n{_case_id(case)}: pixels {nx * nz}, with terms {int(live.sum())}, excluded {int((~keep).sum())}, "
          f"max err / tol {float((err[live] / tol[live]).max()) if live.any() else 0.0:.3g}")
