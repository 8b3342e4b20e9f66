"""What test_gpu_doppler_edges.py relies on, pinned with no device: NaN, +inf and -inf samples through the slow-time autocorrelation,
NaN, +inf, -inf, negative and -0.0 acf values through the maps, and ensembles rescaled by 2^+-24, through the restatement
tests/doppler_util.py (include/pbrt_hip.h: "Non-finite samples get no special treatment").

  A  one bad component in a few pixels of an ensemble: the float32 and the float64 restatement give every plane of every pixel the same
     class (finite, NaN, +inf, -inf; no pixel is left out), all three planes of a pixel that holds a bad sample are non-finite, every
     other pixel has the clean ensemble's values
  B  one bad acf value: the two restatements agree in class for velocity and amplitude; outside the footprint |dx| <= kx // 2,
     |dz| <= kz // 2 both maps are the clean ones; R0 is read by the amplitude only and R1 by the velocity only; NaN fills the
     footprint, +inf in R0 is +inf, -inf or a negative R0 is NaN, R0 = -0.0 under a 1 x 1 window is -0.0 (the root of -0.0), and an
     infinite R1 component gives a finite velocity (atan2 of an infinity is a multiple of pi / 4) on which the two restatements
     differ by no more than the second term of doppler_util.velocity_bound
  C  the ensemble times 2^+-24: the float32 restatement's acf is the clean one times 4^+-24 value for value, the velocity under a
     3 x 5 Hamming window keeps its values and the amplitude is the clean one times 2^+-24; every non-zero acf value stays far inside
     the normal range of float32

The cases, sites and data of both files are defined here."""
import functools
import math

import numpy as np
import pytest

import doppler_util as du
import nlbf_util as nu

BAD = (np.nan, np.inf, -np.inf)
BAD_IDS = ("nan", "plus_inf", "minus_inf")
PARTS = ("re", "im", "both")
SHAPE = (13, 37)
NYQ = 0.3
#            N, degree of the wall filter (None: no filter)
ENSEMBLES = ((8, None), (8, 0), (8, 2), (17, 3), (3, 1), (2, 0))
# flat = 37 ix + iz: 63 | 64 is the boundary between two waves, 255 | 256 between the two workgroups of the autocorrelation
PAIRS = (((0, 0), (12, 36)), ((1, 26), (1, 27)), ((6, 33), (6, 34)))
WINDOWS = tuple((w, k) for k in ((1, 1), (3, 5), (5, 3), (15, 15)) for w in ("boxcar", "hamming"))
MAP_SITES = ((0, 0), (12, 36), (7, 31), (8, 32), (3, 18))       # corners, both sides of the tile boundaries 7 | 8 and 31 | 32, the interior
NEGATIVE_R0 = -1.0e6                                            # (against R0 of about 1 .. 4 around it: negative under every window's smallest weight)
SCALE_CASES = ((8, 2), (17, 3), (8, None), (64, 0))
SCALE_K = (24, -24)
SCALE_WINDOW = ("hamming", (3, 5))


def wall(mi, N, d):
    return None if d is None else mi.wall_basis(N, d)


@functools.lru_cache(maxsize=None)
def ensemble(N, d):
    """the clean ensemble of a case [N, 13, 37] complex64: noise plus a clutter polynomial of the filter's degree, 1e3 times stronger"""
    x = du.ensemble(np.random.default_rng(77 * N + (d or 0)), N, SHAPE, d=d or 0)
    x.setflags(write=False)
    return x


def acf_runs(N):
    """six runs of three sites (frame, ix, iz) each: one pixel of every pair per run -- its neighbour is the clean witness -- and the
    frames 0 (x_0, which the wall filter subtracts from every sample), N // 2 and N - 1 rotated over the pixels"""
    frames = (0, N // 2, N - 1)
    assert PAIRS[1] == ((63 // 37, 63 % 37), (64 // 37, 64 % 37)) and PAIRS[2] == ((255 // 37, 255 % 37), (256 // 37, 256 % 37))
    return [[(frames[(j + r) % 3], *PAIRS[j][side]) for j in range(3)] for side in (0, 1) for r in range(3)]


def bad_ensemble(x, run, value, part):
    """a copy of the ensemble with `value` in the real part, the imaginary part or both at every site of the run"""
    out = np.array(x, copy=True)
    pairs = out.view(np.float32).reshape(out.shape + (2,))
    for n, ix, iz in run:
        if part in ("re", "both"):
            pairs[n, ix, iz, 0] = value
        if part in ("im", "both"):
            pairs[n, ix, iz, 1] = value
    return out


def bad_pixels(run):
    m = np.zeros(SHAPE, bool)
    for _, ix, iz in run:
        m[ix, iz] = True
    return m


def restated_acf(x, q, dtype):
    with np.errstate(invalid="ignore", over="ignore"):
        return du.autocorr(x, q, dtype=dtype)[0]


@functools.lru_cache(maxsize=None)
def tone_acf():
    """the acf of test_maps_against_the_restatement on 13 x 37"""
    a = du.autocorr(du.tone(np.random.default_rng(7), 8, SHAPE))[0].astype(np.float32)
    a.setflags(write=False)
    return a


def map_cases():
    """(label, [(plane, ix, iz, value), ..]): every site in every plane with every bad value, one site with the same bad value in both
    R1 planes (atan2 of two infinities), one negative finite R0 and one R0 = -0.0"""
    cases = [(f"plane {p} at {s} = {v}", [(p,) + s + (v,)]) for s in MAP_SITES for p in range(3) for v in BAD]
    cases += [(f"both R1 planes at (3, 18) = {v}", [(0, 3, 18, v), (1, 3, 18, v)]) for v in BAD]
    cases += [("negative R0 at (7, 31)", [(2, 7, 31, NEGATIVE_R0)]), ("R0 = -0.0 at (8, 32)", [(2, 8, 32, -0.0)])]
    return cases


OVERLAP = [(0, 3, 18, np.inf), (0, 4, 19, -np.inf),(2, 8, 32, np.inf), (2, 7, 31, -np.inf)]   # opposite infinities, footprints that overlap


def bad_acf(edits):
    a = np.array(tone_acf(), copy=True)
    for p, ix, iz, v in edits:
        a[p, ix, iz] = v
    return a


def footprint(edits, kernel, planes=(0, 1, 2)):
    """[13, 37]: the pixels within kx // 2 rows and kz // 2 columns of an edited site of one of `planes`"""
    ix, iz = np.meshgrid(np.arange(SHAPE[0]), np.arange(SHAPE[1]), indexing="ij")
    m = np.zeros(SHAPE, bool)
    for p, sx, sz, _ in edits:
        if p in planes:
            m |= (np.abs(ix - sx) <= kernel[0] // 2) & (np.abs(iz - sz) <= kernel[1] // 2)
    return m


def restated_maps(acf, window, kernel, dtype):
    with np.errstate(invalid="ignore", over="ignore"):
        return du.maps(acf, NYQ, window, kernel, dtype=dtype)


@functools.lru_cache(maxsize=None)
def clean_maps(window, kernel, dtype):
    return restated_maps(tone_acf(), window, kernel, dtype)


ANGLE_BOUND = NYQ / math.pi * 8.0 * du.F32_EPS * math.pi          # the second term of doppler_util.velocity_bound: atan2f and the product


# ---- A ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", ENSEMBLES)
def test_a_bad_sample_gives_both_restatements_the_same_classes(mi, N, d):
    x, q = ensemble(N, d), wall(mi, N, d)
    clean32, clean64 = restated_acf(x, q, np.float32), restated_acf(x, q, np.float64)
    assert np.isfinite(clean32).all()
    seen = set()
    for run in acf_runs(N):
        hit = bad_pixels(run)
        seen |= {(n, ix, iz) for n, ix, iz in run}
        for value in BAD:
            for part in PARTS:
                xb = bad_ensemble(x, run, value, part)
                f32, f64 = restated_acf(xb, q, np.float32), restated_acf(xb, q, np.float64)
                c32 = nu.classes(f32)
                assert np.array_equal(c32, nu.classes(f64)), (N, d, run, value, part)
                assert np.all(c32[:, hit] != nu.FINITE) and np.all(c32[:, ~hit] == nu.FINITE), (N, d, run, value, part)
                assert np.array_equal(f32[:, ~hit], clean32[:, ~hit]) and np.array_equal(f64[:, ~hit], clean64[:, ~hit])
    # every pixel of every pair was bad in one run and a witness in another; every frame of the three was used
    assert {s[1:] for s in seen} == {p for pair in PAIRS for p in pair} and {s[0] for s in seen} == {0, N // 2, N - 1}


# ---- B ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,kernel", WINDOWS)
def test_a_bad_acf_value_through_the_maps(window, kernel):
    c32, c64 = clean_maps(window, kernel, np.float32), clean_maps(window, kernel, np.float64)
    nyq = float(np.float32(NYQ))
    for label, edits in map_cases():
        acf = bad_acf(edits)
        m32, m64 = restated_maps(acf, window, kernel, np.float32), restated_maps(acf, window, kernel, np.float64)
        for name in ("velocity", "amplitude"):
            assert np.array_equal(nu.classes(m32[name]), nu.classes(m64[name])), (label, name)
        fp_vel, fp_amp = footprint(edits, kernel, (0, 1)), footprint(edits, kernel, (2,))
        for m, c in ((m32, c32), (m64, c64)):       # outside the footprint of the planes a map reads, that map is the clean one
            assert np.array_equal(m["velocity"][~fp_vel], c["velocity"][~fp_vel]), label
            assert np.array_equal(m["amplitude"][~fp_amp], c["amplitude"][~fp_amp]), label
        assert fp_vel.any() != fp_amp.any()
        value = edits[0][3]
        inside = m32["amplitude"][fp_amp] if fp_amp.any() else m32["velocity"][fp_vel]
        if np.isnan(value):
            assert np.isnan(inside).all(), label
        elif fp_amp.any():
            if value == np.inf:
                assert np.all(inside == np.inf), label
            elif value == -np.inf or value == NEGATIVE_R0:
                assert np.isnan(inside).all(), label
            else:                                    # -0.0: the root of -0.0 is -0.0 where the window is the pixel itself
                assert value == 0.0 and np.signbit(value) and np.isfinite(inside).all()
                if kernel == (1, 1):
                    for m in (m32, m64):
                        assert m["amplitude"][8, 32] == 0.0 and np.signbit(m["amplitude"][8, 32]), label
        else:                                        # an infinite R1 component: atan2 of an infinity is finite
            assert np.isfinite(inside).all() and np.all(np.abs(inside) <= nyq * (1 + 4 * du.F32_EPS)), label
            assert np.abs(m32["velocity"] - m64["velocity"])[fp_vel].max() <= ANGLE_BOUND, label
            # .. and one of 0, +-pi / 4, +-pi / 2, +-3 pi / 4, +-pi
            turns = m64["velocity"][fp_vel] / nyq * 4.0
            assert np.abs(turns - np.rint(turns)).max() <= 1e-12, label


@pytest.mark.parametrize("window,kernel", WINDOWS)
def test_opposite_infinities_whose_footprints_overlap(window, kernel):
    """where +inf and -inf meet in one sum the restatement gives NaN, elsewhere what the single site gives: the two agree in class"""
    acf = bad_acf(OVERLAP)
    m32, m64 = restated_maps(acf, window, kernel, np.float32), restated_maps(acf, window, kernel, np.float64)
    for name in ("velocity", "amplitude"):
        assert np.array_equal(nu.classes(m32[name]), nu.classes(m64[name])), name
    both_vel = footprint(OVERLAP[:1], kernel) & footprint(OVERLAP[1:2], kernel)
    both_amp = footprint(OVERLAP[2:3], kernel) & footprint(OVERLAP[3:], kernel)
    assert both_vel.any() == both_amp.any() == (kernel != (1, 1))
    assert np.isnan(m32["velocity"][both_vel]).all() and np.isnan(m32["amplitude"][both_amp]).all()
    assert np.isfinite(m32["velocity"][~both_vel]).all() and np.all(m32["amplitude"][footprint(OVERLAP[2:3], kernel) & ~both_amp] == np.inf)


# ---- C ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", SCALE_CASES)
def test_rescaling_the_float32_restatement(mi, N, d):
    x, q = ensemble(N, d), wall(mi, N, d)
    acf = restated_acf(x, q, np.float32)
    window, kernel = SCALE_WINDOW
    m = restated_maps(acf, window, kernel, np.float32)
    for k in SCALE_K:
        scaled = (x * np.float32(2.0 ** k)).astype(np.complex64)
        assert np.array_equal(scaled.astype(np.complex128), x.astype(np.complex128) * 2.0 ** k)          # nothing rounded or flushed
        got = restated_acf(scaled, q, np.float32)
        assert np.array_equal(got, acf * 4.0 ** k), (N, d, k)
        tiny, huge = float(np.abs(got[got != 0]).min()), float(np.abs(got).max())
        print(f"\nN = {N}, degree {d}, 2^{k}: |acf| from {tiny:.3e} to {huge:.3e}")
        assert tiny >= 2.0 ** -100 and huge <= 2.0 ** 100 and (got != 0).all()       # (float32 is normal from 2^-126 to 2^128)
        ms = restated_maps(got.astype(np.float32), window, kernel, np.float32)
        assert np.array_equal(got.astype(np.float32).astype(np.float64), got)
        assert np.array_equal(ms["velocity"], m["velocity"]) and np.array_equal(ms["amplitude"], m["amplitude"] * 2.0 ** k), (N, d, k)
