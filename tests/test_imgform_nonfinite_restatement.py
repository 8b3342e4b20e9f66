"""What test_gpu_imgform_nonfinite.py relies on, pinned with no device: NaN, +inf and -inf samples and samples rescaled by 4^+-30
through the restatements of tests/nlbf_util.py and tests/iq_util.py.

  A  a few bad samples in standard-normal data: the float32 and the float64 restatement give every kept pixel the same class (finite,
     NaN, +inf, -inf) for delay-and-sum, p-DAS (p = 2, 3), F-DMAS and I/Q delay-and-sum; a bad sample in a trace that no pixel's
     aperture reaches changes no bit; the pixels left out (nlbf_util.margins and nlbf_util.near_bad) stay below the project's 2 %
  B  every sample NaN: NaN exactly where a kept pixel uses an element, +0.0 elsewhere
  C  one bad sample through the FIR and the demodulator: the closed-form masks |n - j| <= K and |m D - j| <= K
  D  data times 4^+-30: the float32 restatement's image scales bit for bit (every operation of the stated arithmetic is exactly
     homogeneous under a power of four -- the square root of 4^k is 2^k -- and nothing under- or overflows)

The cases, sites, shapes and data of both files are defined here."""
import functools

import numpy as np
import pytest

import iq_util as iu
import nlbf_util as nu
from walk_cases import C0, T, geometry

NAMES = ("a1_e3_small_lin_f0_sum", "a5_e64_lin_f1_sum", "a6_e65_near_f1_mean", "a6_e3_wide_lin_f1_mean", "a5_e16_convex_lin_f1_sum",
         "a11_e130_small_lin_f1_mean", "a11_e130_small_near_f0_sum")
# bad samples that kept pixels read, per case (nlbf_util.bad_sites adds one in an unreached trace where the case has such a trace)
N_SITES = {"a1_e3_small_lin_f0_sum": 2, "a5_e64_lin_f1_sum": 5, "a6_e65_near_f1_mean": 4, "a6_e3_wide_lin_f1_mean": 3,
           "a5_e16_convex_lin_f1_sum": 4, "a11_e130_small_lin_f1_mean": 5, "a11_e130_small_near_f0_sum": 6}
BAD = (np.nan, np.inf, -np.inf)
METHODS = (("das", 1.0), ("pdas", 2.0), ("pdas", 3.0), ("fdmas", 2.0))
IQ_PARTS = ("re", "im", "both")
F_D = 2.5e6
CAP = 0.02                                  # test_the_grids_leave_out_at_most_two_per_cent
SCALES = (4.0 ** 30, 4.0 ** -30)
#             nx, nz, K
FIR_SHAPES = ((3, 5, 8), (2, 300, 40), (2, 257, 1024), (1, 600, 1024), (2, 512, 0))
#               n, T, K, D       (2048 / 8 = 256 outputs fill one workgroup exactly, 2049 start a second one)
RF2IQ_SHAPES = ((3, 5, 8, 1), (7, 300, 40, 1), (2, 257, 1024, 1), (2, 1030, 16, 4), (1, 513, 3, 8), (2, 700, 40, 3), (1, 2048, 16, 8),
                (1, 2049, 16, 8))
# no mixed phase f_d (t0 + j / fs) is an exact quarter cycle: there sincospif returns an exact 0 where NumPy's cosine does not
RF2IQ_FS, RF2IQ_FD, RF2IQ_T0 = 20.0e6, 2.3e6, 1.7e-6


def _seed(name):
    return sum(map(ord, name))


@functools.lru_cache(maxsize=None)
def clean(name):
    """standard-normal channel data [A, E, T] of a case"""
    g = geometry(name)
    return np.random.default_rng(_seed(name) * 11 + 3).standard_normal((g["A"], g["E"], T)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def clean_iq(name):
    g = geometry(name)
    rng = np.random.default_rng(_seed(name) * 13 + 5)
    return (rng.standard_normal((g["A"], g["E"], T)) + 1j * rng.standard_normal((g["A"], g["E"], T))).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def sites(name):
    """-> (sites, the site no pixel reaches or None, kept [nx, nz]: the pixels neither margins nor near_bad leave out)"""
    g = geometry(name)
    s, idle = nu.bad_sites(g, T, C0, N_SITES[name], _seed(name))
    return s, idle, ~(g["left_out"] | nu.near_bad(g, T, C0, s))


def bad_iq(iq, where, value, part):
    """I/Q data with `value` in the real part, the imaginary part or both at every site"""
    out = np.array(iq, copy=True)
    pairs = out.view(np.float32).reshape(out.shape + (2,))
    for a, e, t in where:
        if part in ("re", "both"):
            pairs[a, e, t, 0] = value
        if part in ("im", "both"):
            pairs[a, e, t, 1] = value
    return out


def restated(name, method, p, data, dtype):
    g = geometry(name)
    with np.errstate(invalid="ignore", over="ignore"):
        return nu.beamform(method, data, g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, p=p, dtype=dtype, **g["kw"])


def restated_iq(name, iq, dtype):
    g = geometry(name)
    with np.errstate(invalid="ignore", over="ignore"):
        return iu.iq_beamform(iq, g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, F_D, dtype=dtype, **g["kw"])


@functools.lru_cache(maxsize=None)
def expected(name, bad, method, p):
    """classes of the float32 restatement's image of the data with the bad samples -- the arithmetic the header states"""
    return nu.classes(restated(name, method, p, nu.with_bad(clean(name), sites(name)[0], BAD[bad]), np.float32)[0])


@functools.lru_cache(maxsize=None)
def expected_iq(name, bad, part):
    return nu.classes(restated_iq(name, bad_iq(clean_iq(name), sites(name)[0], BAD[bad], part), np.float32)[0])


def fir_input(nx, nz, K):
    """standard-normal columns and random non-zero taps"""
    rng = np.random.default_rng(nx * 1000 + nz + K)
    x = rng.standard_normal((nx, nz)).astype(np.float32)
    h = (rng.standard_normal(2 * K + 1) / np.sqrt(2 * K + 1)).astype(np.float32)
    assert np.all(h != 0) and np.all(x != 0)
    return x, h


def bad_indices(n, stride=1):
    """where the bad sample sits: both ends, the middle, and the two samples either side of the first workgroup's last output"""
    return sorted({0, n // 2, n - 1} | {j for j in (255 * stride, 256 * stride) if j < n})


# ---- A ------------------------------------------------------------------------------------------------------------------------
def test_the_sites_are_read_and_leave_out_no_more_than_the_cap():
    idle_cases = 0
    for name in NAMES:
        g = geometry(name)
        where, idle, kept = sites(name)
        M = nu.read_mask(g, T, C0)
        assert 2 <= len(where) <= 6, name
        for site in where:
            assert M[site] == (site != idle), (name, site)
        if idle is not None:
            idle_cases += 1
            assert not M[:, idle[1]].any(), name                 # no kept pixel reads any sample of that element
        share = 1.0 - kept.mean()
        print(f"\n{name}: {len(where)} sites, {int((~kept).sum())} of {kept.size} pixels left out ({share:.3%})")
        assert share <= CAP, (name, share)
    assert idle_cases >= 1


@pytest.mark.parametrize("name", NAMES)
def test_a_bad_sample_gives_both_restatements_the_same_classes(name):
    where, idle, kept = sites(name)
    data, iq = clean(name), clean_iq(name)
    for b, value in enumerate(BAD):
        for method, p in METHODS:
            want = expected(name, b, method, p)
            f64 = nu.classes(restated(name, method, p, nu.with_bad(data, where, value), np.float64)[0])
            assert np.array_equal(f64[kept], want[kept]), (name, value, method, p)
            hit = int((want[kept] != nu.FINITE).sum())
            assert 0 < hit < kept.sum(), (name, value, method, p, hit)
            if np.isnan(value):
                assert np.all(want[kept][want[kept] != nu.FINITE] == nu.NAN)
        for part in IQ_PARTS:
            want = expected_iq(name, b, part)
            f64 = nu.classes(restated_iq(name, bad_iq(iq, where, value, part), np.float64)[0])
            assert np.array_equal(f64[kept], want[kept]), (name, value, part)
            assert 0 < int((want[kept] != nu.FINITE).any(axis=-1).sum()) < kept.sum()
        # every site that is read reaches a pixel of its own: the mask of all sites is the union of the single sites' masks
        if b == 0:
            union = np.zeros(kept.shape, bool)
            for site in where:
                one = nu.classes(restated(name, "das", 1.0, nu.with_bad(data, [site], value), np.float32)[0]) != nu.FINITE
                assert (one & kept).any() == (site != idle), (name, site)
                union |= one
            assert np.array_equal(union[kept], (expected(name, 0, "das", 1.0) != nu.FINITE)[kept])
    print(f"\n{name}: {int((expected(name, 0, 'das', 1.0)[kept] != nu.FINITE).sum())} pixels read a bad sample")


def test_a_bad_sample_outside_every_aperture_changes_no_bit():
    seen = 0
    for name in NAMES:
        idle = sites(name)[1]
        if idle is None:
            continue
        seen += 1
        for value in BAD:
            for method, p in METHODS:
                got = restated(name, method, p, nu.with_bad(clean(name), [idle], value), np.float32)[0]
                assert np.array_equal(got, restated(name, method, p, clean(name), np.float32)[0]), (name, value, method)
            got = restated_iq(name, bad_iq(clean_iq(name), [idle], value, "both"), np.float32)[0]
            assert np.array_equal(got, restated_iq(name, clean_iq(name), np.float32)[0]), (name, value)
    assert seen >= 1


# ---- B ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_sample_nan(name):
    g = geometry(name)
    keep = ~g["left_out"]
    uses = g["n_a"].sum(axis=0) > 0
    if name == "a6_e3_wide_lin_f1_mean":
        assert not uses[:8].any() and not uses[16:].any() and uses[8:16].any()        # the outer x tiles see no element
    data = np.full((g["A"], g["E"], T), np.nan, np.float32)
    for dtype in (np.float32, np.float64):
        imgs = [restated(name, method, p, data, dtype)[0] for method, p in METHODS]
        iq = restated_iq(name, data.astype(np.complex64) * (1 + 1j), dtype)[0]
        # (the restatement multiplies a zero sum by the transmit phase, which can give -0.0; the kernel adds every term to +0.0, and the
        # GPU test asks for +0.0)
        for img in imgs + [iq.real, iq.imag]:
            assert np.isnan(img[keep & uses]).all() and np.all(img[keep & ~uses] == 0.0)


# ---- C ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nz,K", FIR_SHAPES)
def test_fir_masks(nx, nz, K):
    x, h = fir_input(nx, nz, K)
    ref = nu.fir(x, h)
    for j in bad_indices(nz):
        for value in BAD:
            xb = x.copy()
            xb[nx - 1, j] = value
            with np.errstate(invalid="ignore"):
                got = nu.fir(xb, h)
            mask = nu.fir_bad_mask(nz, K, j)
            assert np.array_equal(~np.isfinite(got[nx - 1]), mask), (j, value)
            assert np.array_equal(got[nx - 1][~mask], ref[nx - 1][~mask]) and np.array_equal(got[:nx - 1], ref[:nx - 1])
            if np.isnan(value):
                assert np.isnan(got[nx - 1][mask]).all()
            else:     # one infinite product per output: its sign is the tap's times the sample's
                n = np.arange(nz)[mask]
                assert np.array_equal(got[nx - 1][mask], np.sign(h[K + n - j]).astype(np.float64) * value)


@pytest.mark.parametrize("n,Tn,K,D", RF2IQ_SHAPES)
def test_rf2iq_masks(n, Tn, K, D):
    x, h = fir_input(n, Tn, K)
    args = (RF2IQ_FS, RF2IQ_T0, RF2IQ_FD, D, h)
    ref32 = iu.rf2iq(x, *args, dtype=np.float32)[0]
    # no phase, as the float32 fraction of a cycle the kernel takes the cosine and sine of, is an exact quarter cycle
    cyc = float(np.float32(RF2IQ_FD)) * (float(np.float32(RF2IQ_T0)) + np.arange(Tn) / float(np.float32(RF2IQ_FS)))
    ph = (cyc - np.floor(cyc)).astype(np.float32)
    assert np.all(4.0 * ph != np.rint(4.0 * ph))
    for j in bad_indices(Tn, D):
        mask = iu.rf2iq_bad_mask(Tn, K, D, j)
        for value in BAD:
            xb = x.copy()
            xb[n - 1, j] = value
            with np.errstate(invalid="ignore"):
                f32, f64 = iu.rf2iq(xb, *args, dtype=np.float32)[0], iu.rf2iq(xb, *args)[0]
            c32, c64 = nu.classes(f32), nu.classes(f64)
            assert np.array_equal(c32, c64), (j, value)
            assert np.array_equal((c32[n - 1] != nu.FINITE).any(axis=-1), mask) and np.array_equal((c32[n - 1] != nu.FINITE).all(axis=-1), mask)
            assert np.array_equal(f32[n - 1][~mask], ref32[n - 1][~mask]) and np.array_equal(f32[:n - 1], ref32[:n - 1])
            assert np.all(c32[n - 1][mask] == nu.NAN) if np.isnan(value) else np.all(c32[n - 1][mask] >= nu.POS_INF)


# ---- D ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_rescaling_the_float32_restatement(name):
    data, iq = clean(name), clean_iq(name)
    for s in SCALES:
        s32 = np.float32(s)
        scaled = data * s32
        assert np.array_equal(scaled.astype(np.float64), data.astype(np.float64) * s) and np.isfinite(scaled).all()      # nothing flushed
        for method, p in (("das", 1.0), ("pdas", 2.0), ("fdmas", 2.0)):
            img = restated(name, method, p, data, np.float32)[0]
            assert img.dtype == np.float32 and np.array_equal(restated(name, method, p, scaled, np.float32)[0], s32 * img), (name, s, method)
        img = restated_iq(name, iq, np.float32)[0]
        assert np.array_equal(restated_iq(name, iq * s32, np.float32)[0], s * img), (name, s)


@pytest.mark.parametrize("n,Tn,K,D", RF2IQ_SHAPES)
def test_rescaling_the_float32_demodulator(n, Tn, K, D):
    x, h = fir_input(n, Tn, K)
    args = (RF2IQ_FS, RF2IQ_T0, RF2IQ_FD, D, h)
    ref = iu.rf2iq(x, *args, dtype=np.float32)[0]
    for s in SCALES:
        assert np.array_equal(iu.rf2iq(x * np.float32(s), *args, dtype=np.float32)[0], s * ref), s
