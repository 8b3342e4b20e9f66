"""Colour and power Doppler on the device at its edges (include/pbrt_hip.h "Range and non-finite values"), held to the
restatement tests/doppler_util.py; tests/test_doppler_nonfinite_restatement.py defines the cases, sites and data used here and pins on
the CPU what the restatement itself says of them.  (Every instance of k_doppler_autocorr and the thin images of k_doppler_maps are
cases of tests/test_gpu_doppler.py.)

  B  a bad sample (NaN, +inf, -inf; real part, imaginary part or both) in three pixels of an ensemble: the device's class (finite, NaN,
     +inf, -inf) of every plane and pixel is the float32 restatement's, every pixel without a bad sample has the bits of the device's
     clean run -- the neighbour across a wave and across a workgroup boundary among them -- and the host form equals the dev form
  C  a bad acf value through the maps, per site, plane, value and window: classes as the float32 restatement's, the clean run's bits
     outside the footprint and in the map that does not read the plane, the float64 angle to atan2f's share of the velocity bound where
     an infinite R1 leaves the velocity finite, sqrtf's -0.0 and NaN for R0 = -0.0 and R0 < 0; two opposite infinities that overlap
  E  the ensemble times 2^+-24: acf times 4^+-24, the velocity and the amplitude times 2^+-24, bit for bit; samples of 2^-80, whose
     squares vanish: zero motion and zero power
  F  doppler_render at decimation 4 under mean removal and a 3 x 5 Hamming window on the moving plate of D24; then other ensemble
     lengths and scans on the same integrator, whose cached plan must not show through; then the D12 plate, whose channel buffer
     holds NaN echoes

No pixel is left out anywhere but by the velocity rule's 10 % (test_gpu_doppler.py)."""
import math

import numpy as np
import pytest

import doppler_util as du
import nlbf_util as nu
from test_doppler_nonfinite_restatement import (ANGLE_BOUND, BAD, BAD_IDS, ENSEMBLES, NEGATIVE_R0, NYQ, OVERLAP, PARTS, SCALE_CASES, SCALE_K,
                                                SHAPE, WINDOWS, acf_runs, bad_acf, bad_ensemble, bad_pixels, ensemble, footprint, map_cases,
                                                restated_acf, restated_maps, tone_acf, wall)
from test_gpu_doppler import PRF, RENDER, _held
from test_gpu_imgform_nonfinite import _d12_scene

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _wall_args(d):
    return ("none", 0) if d is None else ("poly", d)


# ---- B ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", range(len(BAD)), ids=BAD_IDS)
@pytest.mark.parametrize("N,d", ENSEMBLES)
def test_a_bad_sample_pixel_by_pixel(mi, N, d, bad):
    cx = mi.default_context()
    x, q, value = ensemble(N, d), wall(mi, N, d), BAD[bad]
    clean = mi.doppler_autocorr(x, *_wall_args(d))
    assert clean.shape == (3,) + SHAPE and np.isfinite(clean).all()
    for run in acf_runs(N):
        hit = bad_pixels(run)
        for part in PARTS:
            xb = bad_ensemble(x, run, value, part)
            want = nu.classes(restated_acf(xb, q, np.float32))
            got = mi.doppler_autocorr(xb, *_wall_args(d))
            cls = nu.classes(got)
            assert np.array_equal(cls, want), (N, d, run, value, part, np.argwhere(cls != want)[:8].tolist())
            assert np.all(cls[:, hit] != nu.FINITE) and np.array_equal(bits(got)[:, ~hit], bits(clean)[:, ~hit]), (N, d, run, value, part)
            dev = mi.doppler_autocorr(mi.DeviceBuffer.from_host(cx, xb), *_wall_args(d)).numpy()
            assert np.array_equal(dev, got, equal_nan=True), (N, d, run, value, part)


# ---- C ------------------------------------------------------------------------------------------------------------------------
def _check_maps(mi, window, kernel, label, edits, clean):
    acf = bad_acf(edits)
    vel, amp = mi.doppler_maps(acf, NYQ, window, kernel)
    m32, m64 = restated_maps(acf, window, kernel, np.float32), restated_maps(acf, window, kernel, np.float64)
    for got, name in ((vel, "velocity"), (amp, "amplitude")):
        cls, want = nu.classes(got), nu.classes(m32[name])
        assert np.array_equal(cls, want), (label, name, np.argwhere(cls != want)[:8].tolist())
    # outside the footprint of the planes a map reads -- everywhere, for the map that does not read the edited plane -- the clean run's bits
    fp_vel, fp_amp = footprint(edits, kernel, (0, 1)), footprint(edits, kernel, (2,))
    assert np.array_equal(bits(vel)[~fp_vel], bits(clean[0])[~fp_vel]) and np.array_equal(bits(amp)[~fp_amp], bits(clean[1])[~fp_amp]), label
    # where an infinite R1 leaves the velocity finite: the float64 angle, to atan2f's six ulp and the product
    fin = fp_vel & np.isfinite(m32["velocity"])
    if fin.any():
        assert np.abs(vel.astype(np.float64) - m64["velocity"])[fin].max() <= ANGLE_BOUND, label
    return vel, amp


@pytest.mark.parametrize("window,kernel", WINDOWS)
def test_a_bad_acf_value_through_the_maps(mi, window, kernel):
    clean = mi.doppler_maps(tone_acf(), NYQ, window, kernel)
    assert np.isfinite(clean[0]).all() and np.isfinite(clean[1]).all()
    for label, edits in map_cases():
        vel, amp = _check_maps(mi, window, kernel, label, edits, clean)
        if edits[0][3] == NEGATIVE_R0:
            assert np.isnan(amp[7, 31])
            assert np.isnan(amp[footprint(edits, kernel)]).all()
        if edits[0][3] == 0.0:                       # R0 = -0.0
            assert np.isfinite(amp).all()
            if kernel == (1, 1):
                assert bits(amp)[8, 32] == 0x80000000, label        # sqrtf(-0.0f) = -0.0f: a 1 x 1 window leaves the plane as it is
    _check_maps(mi, window, kernel, "opposite infinities", OVERLAP, clean)
    # and the dev form, on the case with the most classes in it
    cx = mi.default_context()
    hv, ha = mi.doppler_maps(bad_acf(OVERLAP), NYQ, window, kernel)
    dv, da = mi.doppler_maps(mi.DeviceBuffer.from_host(cx, bad_acf(OVERLAP)), NYQ, window, kernel)
    assert np.array_equal(dv.numpy(), hv, equal_nan=True) and np.array_equal(da.numpy(), ha, equal_nan=True)


# ---- E ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", SCALE_CASES)
def test_rescaled_ensembles_scale_the_maps_bit_for_bit(mi, N, d):
    x = ensemble(N, d)
    acf = mi.doppler_autocorr(x, *_wall_args(d))
    maps = {k: mi.doppler_maps(acf, NYQ, "hamming", k) for k in ((1, 1), (3, 5))}
    for k in SCALE_K:
        scaled = (x * np.float32(2.0 ** k)).astype(np.complex64)
        got = mi.doppler_autocorr(scaled, *_wall_args(d))
        want = np.ldexp(acf, 2 * k)
        assert np.isfinite(want).all() and (want != 0).all() and np.array_equal(bits(got), bits(want)), (N, d, k)
        for kernel, (vel, amp) in maps.items():
            v, a = mi.doppler_maps(got, NYQ, "hamming", kernel)
            assert np.array_equal(bits(v), bits(vel)) and np.array_equal(bits(a), bits(np.ldexp(amp, k))), (N, d, k, kernel)


@pytest.mark.parametrize("wall_filter", ["none", "mean"])
def test_samples_whose_squares_vanish_read_as_zero_motion_and_zero_power(mi, wall_filter):
    """Two rows of pixels hold samples of 2^-80 (1 + i) in every frame, two more +-2^-80 +- 2^-80 i with random signs: every product
    is at most 2^-157 in magnitude, below half the smallest subnormal, and rounds to a zero.  Equal samples: acf, velocity and
    amplitude are +0.0 bit for bit.  Random signs: a fused multiply-add that rounds a negative product into a +0.0 sum gives -0.0 (the
    restatement's separate product and sum give +0.0), so R1 there is a zero of either sign; R0, a sum of squares, the velocity (exactly
    0 where R1 compares equal to zero) and the amplitude are +0.0."""
    rng = np.random.default_rng(80)
    x = np.array(ensemble(8, 0), copy=True)
    tiny = np.float32(2.0 ** -80)
    x[:, 3:5, :] = tiny * (1 + 1j)
    signs = rng.choice([-1.0, 1.0], size=(8, 2, 37)) + 1j * rng.choice([-1.0, 1.0], size=(8, 2, 37))
    x[:, 9:11, :] = (tiny * signs).astype(np.complex64)
    assert np.all(np.abs(x[:, 3:5].real) == tiny) and np.all(np.abs(x[:, 9:11].imag) == tiny)
    acf = mi.doppler_autocorr(x, wall_filter)
    assert not bits(acf)[:, 3:5].any() and not acf[:, 9:11].any() and not bits(acf)[2, 9:11].any()
    other = np.ones(SHAPE, bool)
    other[3:5] = other[9:11] = False
    assert np.array_equal(bits(acf)[:, other], bits(mi.doppler_autocorr(ensemble(8, 0), wall_filter))[:, other]) and (acf[2][other] > 0).all()
    vel, amp = mi.doppler_maps(acf, NYQ, "hamming", (1, 1))
    assert not bits(vel)[~other].any() and not bits(amp)[~other].any() and (amp[other] > 0).all()
    disp = mi.get_power_doppler_map(x, wall_filter, dynamic_range=40.0)
    assert np.isfinite(disp).all() and np.array_equal(disp, mi.log_compress(mi.get_power_doppler_map(x, wall_filter), 40.0))
    assert np.array_equal(mi.get_power_doppler_map(x, wall_filter), amp) and not disp[~other].any() and disp.max() == 1.0


# ---- F ------------------------------------------------------------------------------------------------------------------------
CONFIG = dict(decimation=4, wall_filter="mean", smoothing="hamming", kernel=(3, 5))
STEP = du.LAM / 2


def _numpy(bufs):
    return {k: v.numpy() for k, v in bufs.items()}


@pytest.fixture(scope="module")
def plate(mi):
    """doppler_render on the eight plate scenes, dz = +-lambda / 16, in CONFIG: the images and the buffers of each call"""
    out = {}
    for sign in (-1, +1):
        scenes = du.plate_scenes(mi, sign * du.LAM / 16)
        bufs = {}
        vel, disp, (xs, zs) = mi.doppler_render(scenes, PRF, buffers=bufs, **CONFIG, **RENDER)
        out[sign] = dict(vel=vel, disp=disp, xs=xs, zs=zs, scenes=scenes, **_numpy(bufs))
    return out


@pytest.mark.parametrize("sign", [+1, -1])
def test_doppler_render_at_decimation_4_under_a_window(mi, plate, sign):
    """held the way test_doppler_render_on_the_moving_plate holds the 1 x 1 case: the acf on the call's own frames, amplitude and
    velocity on the call's own acf by the rule of test_maps_against_the_restatement, the display, and the physics on the smoothed
    planes.  (The CPU reference chain at decimation 4 gives -0.2425 and +0.2470 on 13 and 14 pixels, and the velocity rule leaves out
    0 of 95.  No degree-1 filter here: the tone makes one turn over the 8 pulses, and the linear filter biases it to -+0.297 in the
    reference chain itself.)"""
    r = plate[sign]
    assert r["frames"].shape == (8, 5, 19) and r["acf"].shape == (3, 5, 19) and r["vel"].shape == r["disp"].shape == (19, 5)
    nyq = mi.nyquist_velocity(du.PLATE["c"], PRF, du.PLATE["f"])
    q = mi.wall_basis(8, 0)
    f64, B = du.autocorr(r["frames"], q)
    f32, _ = du.autocorr(r["frames"], q, dtype=np.float32)
    for plane, name in enumerate(("Re R1", "Im R1", "R0")):
        _held(f"plate {sign:+d}, D = 4, mean, {name}", r["acf"][plane], f64[plane], f32[plane], B[plane])
    window, kernel = CONFIG["smoothing"], CONFIG["kernel"]
    m64, m32 = du.maps(r["acf"], nyq, window, kernel), du.maps(r["acf"], nyq, window, kernel, dtype=np.float32)
    floor = max(du.floor_of(m32["planes"][p], m64["planes"][p], m64["B"][p]) for p in range(3))
    _held(f"plate {sign:+d}, D = 4, amplitude", r["amplitude"], m64["amplitude"], m32["amplitude"], m64["B_amp"])
    bound, kept = du.velocity_bound(m64, nyq, floor)
    err = np.abs(r["vel"].T.astype(np.float64) - m64["velocity"])
    print(f"plate {sign:+d}, D = 4, velocity: left out {int((~kept).sum())} of {kept.size}, worst error / bound {float((err[kept] / bound[kept]).max()):.3f}")
    assert (~kept).sum() <= 0.1 * kept.size and np.all(err[kept] <= bound[kept])
    assert np.array_equal(r["disp"].T, mi.log_compress(r["amplitude"], RENDER["dynamic_range"]))
    s = m64["planes"]
    keep = s[2] >= 0.1 * s[2].max()
    med = float(np.median(np.arctan2(s[1], s[0])[keep])) / math.pi
    expected = -4.0 * sign / 16.0
    print(f"doppler_render D = 4, 3 x 5 hamming, dz = {sign:+d} lambda/16: median arg R1 / pi = {med:+.4f} on {int(keep.sum())} of {keep.size} "
          f"pixels (expected {expected:+.4f})")
    assert keep.sum() >= 4 and med * expected > 0 and abs(med - expected) <= 0.1 * abs(expected)
    assert np.sign(np.median(r["vel"].T[keep])) == -sign


def test_doppler_render_again_on_the_same_integrator(mi, plate):
    """the plan and its ensemble, acf and map buffers are cached on the first scene's integrator under (plan key, N): a shorter
    ensemble, a larger scan and the first configuration again, each held bit for bit to the chain on that call's own frames (the rule
    of test_doppler_render_on_device_returns_the_same_bits), each with buffers of its own shapes"""
    scenes = plate[+1]["scenes"]
    nyq = mi.nyquist_velocity(du.PLATE["c"], PRF, du.PLATE["f"])
    larger = dict(RENDER, x_range=(RENDER["x_range"][0], RENDER["x_range"][1] + STEP), z_range=(RENDER["z_range"][0], RENDER["z_range"][1] + STEP))
    seen = []
    for N, kw, shape in ((4, RENDER, (5, 19)), (8, larger, (6, 20)), (8, RENDER, (5, 19))):
        bufs = {}
        vel, disp, (xs, zs) = mi.doppler_render(scenes[:N], PRF, buffers=bufs, **CONFIG, **kw)
        assert (len(xs), len(zs)) == shape and vel.shape == disp.shape == shape[::-1]
        assert bufs["frames"].shape == (N,) + shape and bufs["acf"].shape == (3,) + shape and bufs["amplitude"].shape == shape
        b = _numpy(bufs)
        assert np.isfinite(b["frames"]).all() and b["frames"].any(axis=(1, 2)).all()
        acf = mi.doppler_autocorr(b["frames"], "mean")
        v, a = mi.doppler_maps(acf, nyq, CONFIG["smoothing"], CONFIG["kernel"])
        assert np.array_equal(bits(b["acf"]), bits(acf)) and np.array_equal(bits(b["amplitude"]), bits(a)), (N, shape)
        assert np.array_equal(bits(vel.T), bits(v)) and np.array_equal(bits(disp.T), bits(mi.log_compress(a, RENDER["dynamic_range"]))), (N, shape)
        seen.append(b["acf"])
    assert not np.array_equal(seen[0], seen[2])          # four pulses and eight are different ensembles: nothing was handed back unchanged


def test_doppler_render_on_the_d12_plate(mi, ob):
    """DESIGN D12: the 0-degree plane wave on a plate that faces the probe exactly leaves NaN echoes in the channel buffer, which the
    pulse, rf2iq's low-pass and the beamformer spread.  Eight identical scenes, 13 x 37 pixels at lambda / 2 from 10 mm down, across
    the depth from which the NaN echoes are read (picked on the CPU oracle's acquisition, whose first NaN echo the test asserts to lie
    at sample 800: 15 mm): acf and velocity are NaN exactly at the pixels whose ensemble holds a NaN and finite elsewhere, the amplitude
    is NaN there, and the power display is NaN everywhere -- k_log_compress's stated rule."""
    edits = dict(pulse_model="gaussian", angles=[0.0])
    scenes = [_d12_scene(mi, **edits) for _ in range(8)]
    ui = scenes[0].integrator()
    buf, _ = ob.OracleScene.from_scene(scenes[0]).us_acquire(ui.us_params(scenes[0]), ui.seed, ui.paths_per_ray)
    nan_at = np.flatnonzero(np.isnan(np.asarray(buf).reshape(32, 4000)).any(axis=0))
    assert nan_at[0] == 800 and nan_at[-1] < 900
    bufs = {}
    vel, disp, (xs, zs) = mi.doppler_render(scenes, PRF, x_range=(-6 * STEP, 5.75 * STEP), z_range=(0.010, 0.010 + 35.75 * STEP), kernel=(1, 1),
                                            buffers=bufs)
    b = _numpy(bufs)
    assert (len(xs), len(zs)) == (13, 37) and b["frames"].shape == (8, 13, 37)
    bad = np.isnan(b["frames"]).any(axis=0)
    print(f"D12 plate: {int(bad.sum())} of {bad.size} pixels hold a NaN in their ensemble")
    assert bad.any() and not bad.all() and not np.isinf(b["frames"].view(np.float32)).any()
    assert not bad[:, :8].any() and bad[:, -8:].all()         # clean above the plate's first echo, NaN below it
    assert np.array_equal(np.isnan(b["acf"]), np.broadcast_to(bad, (3,) + bad.shape)) and np.isfinite(b["acf"][:, ~bad]).all()
    assert np.array_equal(np.isnan(vel.T), bad) and np.isfinite(vel.T[~bad]).all()
    assert np.isnan(b["amplitude"][bad]).all() and np.isfinite(b["amplitude"][~bad]).all()
    assert np.isnan(disp).all()
