"""I/Q beamforming on the device: k_rf2iq, k_iq_beamform and k_iq_modulus against the float64 restatement of
tests/iq_util.py, the refusals, and us_render(iq=True) end to end.

The shapes are those of test_gpu_nlbf.py, the smallest at which the walk can still go wrong: 1 / 5 / 6 / 11 transmissions, 3 / 64 / 65 /
130 elements, scans of 9 x 13, 24 x 16 and 9 x 17 pixels (partial 8 x 8 tiles), traces of 160 complex samples; the demodulator at a trace
shorter than its taps, a second workgroup with one output at the largest K, and decimations whose last window is partial.

The tolerance is the project's scheme, not a constant: per case the device's largest |got - float64| / B over the pixels kept must be at
most FOUR TIMES the float32 floor, the largest |float32 restatement - float64| / B (B: the size of what is added up, iq_util).  Every
case prints both before it asserts; DESIGN.md D20 records the largest ratio."""
import ctypes as C

import numpy as np
import pytest

import convex_util as cu
import das_util as du
import iq_util as iu
import nlbf_util as nu
from conftest import scene_path
from walk_cases import C0, CASES, T, geometry
from walk_cases import FS as FS_IQ

pytestmark = pytest.mark.gpu

F_D = 2.5e6


def normal_iq(name):
    g = geometry(name)
    rng = np.random.default_rng(sum(map(ord, name)) * 5 + 1)
    return (rng.standard_normal((g["A"], g["E"], T)) + 1j * rng.standard_normal((g["A"], g["E"], T))).astype(np.complex64)


def device_image(mi, g, iq, f_d, form="dev"):
    """the library's image: form 'dev' (pbrt_iq_beamform_dev), 'table' (_table_dev) or 'host' (pbrt_iq_beamform)"""
    args = (g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, f_d)
    if form == "host":
        return mi.iq_beamform(iq, *args, **g["kw"])
    cx = mi.default_context()
    d = mi.DeviceBuffer.from_host(cx, iq)
    table = mi.das_first_arrival(g["tx"], g["elem"], g["x"], g["z"], C0) if form == "table" else None
    out = mi.iq_beamform(d, *args, table=table, **g["kw"])
    assert isinstance(out, mi.DeviceBuffer) and out.dtype == np.complex64
    return out.numpy()


# ---- demodulation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t0", [0.0, 1.7e-6])
@pytest.mark.parametrize("n,Tn,K,D", [(3, 5, 8, 1), (7, 300, 40, 1), (2, 257, 1024, 1), (2, 1030, 16, 4), (1, 513, 3, 8)])
def test_rf2iq(mi, n, Tn, K, D, t0):
    rng = np.random.default_rng(n * 100000 + Tn * 10 + K + D)
    x = rng.standard_normal((n, Tn)).astype(np.float32)
    h = (rng.standard_normal(2 * K + 1) / np.sqrt(2 * K + 1)).astype(np.float32)
    fs, f_d = 20.0e6, 2.3e6
    got = mi.rf2iq(x, f_d, fs, t0=t0, decimation=D, taps=h)
    Td = -(-Tn // D)
    assert got.shape == (n, Td) and got.dtype == np.complex64
    ref, B = iu.rf2iq(x, fs, t0, f_d, D, h)
    f32, _ = iu.rf2iq(x, fs, t0, f_d, D, h, dtype=np.float32)
    used = B > 0
    floor = float((np.abs(f32 - ref)[used] / B[used]).max())
    ratio = float((np.abs(got.astype(np.complex128) - ref)[used] / B[used]).max())
    print(f"\nrf2iq n={n} T={Tn} K={K} D={D} t0={t0}: float32 floor {floor:.3e}, device {ratio:.3e} ({ratio / floor:.2f} x)")
    assert used.all() and ratio <= 4.0 * floor
    cx = mi.default_context()
    dev = mi.rf2iq(mi.DeviceBuffer.from_host(cx, x), f_d, fs, t0=t0, decimation=D, taps=h)
    assert isinstance(dev, mi.DeviceBuffer) and dev.dtype == np.complex64 and dev.shape == (n, Td)
    assert np.array_equal(dev.numpy(), got)


def test_rf2iq_default_lowpass_and_leading_axes(mi):
    """[A, E, T] in gives [A, E, Td] out; the default taps are lowpass_taps(fc * bandwidth / 200, fs)"""
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 3, 400)).astype(np.float32)
    got = mi.rf2iq(x, 5e6, 50e6, decimation=4)
    assert got.shape == (2, 3, 100)
    assert np.array_equal(got, mi.rf2iq(x, 5e6, 50e6, decimation=4, taps=mi.lowpass_taps(2.5e6, 50e6)))
    assert np.array_equal(got.reshape(6, 100), mi.rf2iq(x.reshape(6, 400), 5e6, 50e6, decimation=4))


# ---- the I/Q walk --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_device_against_the_float64_restatement(mi, name):
    g = geometry(name)
    iq = normal_iq(name)
    keep = ~g["left_out"]
    unused = (g["n_a"].sum(axis=0) == 0) & keep
    args = (iq, g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, F_D)
    ref, B = iu.iq_beamform(*args, **g["kw"])
    f32, _ = iu.iq_beamform(*args, dtype=np.float32, **g["kw"])
    got = device_image(mi, g, iq, F_D)
    assert got.shape == ref.shape and got.dtype == np.complex64
    used = keep & (B > 0)
    floor = float((np.abs(f32 - ref)[used] / B[used]).max())
    ratio = float((np.abs(got.astype(np.complex128) - ref)[used] / B[used]).max())
    print(f"\n{name}: float32 floor {floor:.3e}, device {ratio:.3e} ({ratio / floor:.2f} x), {int(used.sum())} pixels, "
          f"{int(g['left_out'].sum())} left out")
    assert np.all(got[unused] == 0.0)                               # a pixel that uses no element is exactly (0, 0)
    assert ratio <= 4.0 * floor, (name, ratio, floor)
    # the first-arrival table changes no bit, nor does staging the arguments from host memory
    assert np.array_equal(device_image(mi, g, iq, F_D, "table"), got), name
    assert np.array_equal(device_image(mi, g, iq, F_D, "host"), got), name


@pytest.mark.parametrize("name", ["a5_e64_lin_f1_sum", "a6_e65_near_f1_mean", "a5_e16_convex_lin_f1_sum"])
def test_device_with_a_time_origin(mi, name):
    """das.t0 = 1.7 us: the sample index follows t_tx + d / c - t0, the re-modulation the absolute t_tx and d / c"""
    g = geometry(name)
    t0 = 1.7e-6
    iq = normal_iq(name)
    kw = dict(g["kw"], t0=t0)
    left_out, n_a = nu.margins(g["tx"], g["elem"], g["x"], g["z"], T, g["fs"], C0, t0=t0, f_number=kw["f_number"],
                               interpolation=kw["interpolation"])
    args = (g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, F_D)
    ref, B = iu.iq_beamform(iq, *args, **kw)
    f32, _ = iu.iq_beamform(iq, *args, dtype=np.float32, **kw)
    got = mi.iq_beamform(iq, *args, **kw)
    used = ~left_out & (B > 0)
    floor = float((np.abs(f32 - ref)[used] / B[used]).max())
    ratio = float((np.abs(got.astype(np.complex128) - ref)[used] / B[used]).max())
    print(f"\n{name} t0={t0}: float32 floor {floor:.3e}, device {ratio:.3e} ({ratio / floor:.2f} x), {int(used.sum())} pixels, "
          f"{int(left_out.sum())} left out")
    assert left_out.mean() <= 0.02 and used.sum() >= 0.5 * used.size
    assert ratio <= 4.0 * floor
    table = mi.das_first_arrival(g["tx"], g["elem"], g["x"], g["z"], C0)
    dev = mi.iq_beamform(mi.DeviceBuffer.from_host(mi.default_context(), iq), *args, table=table, **kw).numpy()
    assert np.array_equal(dev, got)


def test_zero_aperture_tiles_are_exactly_zero(mi):
    g = geometry("a6_e3_wide_lin_f1_mean")
    none = g["n_a"].sum(axis=0) == 0
    assert none[:8].all() and none[16:].all() and not none[8:16].all()       # the outer x tiles see no element, the middle one does
    iq = normal_iq("a6_e3_wide_lin_f1_mean")
    for form in ("dev", "table"):
        got = device_image(mi, g, iq, F_D, form)
        assert np.all(got[none & ~g["left_out"]] == 0.0) and np.any(got[8:16] != 0.0)
        assert not np.signbit(got[:8].real).any() and not np.signbit(got[:8].imag).any()


@pytest.mark.parametrize("name", ["a5_e64_lin_f1_sum", "a6_e65_near_f1_mean", "a1_e3_small_lin_f0_sum", "a5_e16_convex_lin_f1_sum"])
def test_constant_traces_give_the_closed_forms(mi, name):
    """traces == (0.75, 0) without a carrier: every product and partial sum is exact, Re = n_terms 0.75 (/ A for mean, one rounding)
    and Im = 0"""
    g = geometry(name)
    v = 0.75
    n_terms, keep = g["n_a"].sum(axis=0), ~g["left_out"]
    iq = np.full((g["A"], g["E"], T), v, np.complex64)
    got = device_image(mi, g, iq, 0.0)
    want = np.float32(n_terms * v)
    if g["kw"]["compound"] == "mean":
        want = want / np.float32(g["A"])
    assert n_terms.max() >= 3 and np.array_equal(got.real[keep], want.astype(np.float32)[keep]) and np.all(got.imag[keep] == 0.0)


@pytest.mark.parametrize("name", ["a5_e64_lin_f1_sum", "a6_e65_near_f1_mean", "a6_e16_convex_small_near_f0_mean"])
def test_without_a_carrier_it_is_rf_delay_and_sum(mi, name):
    g = geometry(name)
    rng = np.random.default_rng(len(name))
    data = rng.standard_normal((g["A"], g["E"], T)).astype(np.float32)
    args = (g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0)
    got = device_image(mi, g, data.astype(np.complex64), 0.0)
    ref, _ = nu.beamform("das", data, *args, **g["kw"])
    tol_of = cu.das_tolerance if g["elem"].ndim == 2 else du.tolerance
    tol, n_terms = tol_of(data, *args, **g["kw"])
    keep = ~g["left_out"]
    assert np.any(ref[keep] != 0) and np.all(got.imag == 0.0)
    assert np.all(np.abs(got.real.astype(np.float64) - ref)[keep] <= tol[keep])
    assert np.all(got[(n_terms == 0) & keep] == 0.0)


# ---- the modulus ---------------------------------------------------------------------------------------------------------------
def _fma32(x, y, z):
    """fmaf(x, y, z) of float32 arrays, rounded once: x * y is exact in float64 (48 bits), TwoSum gives the float64 sum s and its
    error e exactly, and s + e rounds to the float32 that s rounds to unless s lies exactly midway between two float32 values (the
    midpoints are float64 numbers, so the exact sum cannot pass one that s does not reach) -- there the sign of e decides"""
    a, b = x.astype(np.float64) * y.astype(np.float64), z.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = a + b
        bb = s - a
        e = (a - (s - bb)) + (b - bb)
        r = s.astype(np.float32)
        up, dn = np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))
        mid_up, mid_dn = 0.5 * (r.astype(np.float64) + up.astype(np.float64)), 0.5 * (r.astype(np.float64) + dn.astype(np.float64))
        r = np.where(np.isfinite(s) & (s == mid_up) & (e > 0), up, r)
        r = np.where(np.isfinite(s) & (s == mid_dn) & (e < 0), dn, r)
    return r.astype(np.float32)


def test_modulus(mi, capi):
    rng = np.random.default_rng(9)
    iq = ((rng.standard_normal((7, 5000)) + 1j * rng.standard_normal((7, 5000))) * 10.0 ** rng.uniform(-3, 3, (7, 5000))).astype(np.complex64)
    iq[3, 17] = np.nan + 1j
    iq[4, 4999] = np.complex64(complex(2.0, np.inf))
    got = mi.iq_envelope(iq)                                          # nz = 5000: no limit, where pbrt_envelope stops at 4096
    assert got.shape == iq.shape and got.dtype == np.float32
    ref = np.abs(iq.astype(np.complex128))
    bad = np.isnan(ref)
    assert bad.sum() == 1 and np.array_equal(np.isnan(got), bad) and got[4, 4999] == np.inf       # one NaN pixel stays one NaN pixel
    # one ulp, as the unit in the last place RELATIVE to the value, 2^-23 |ref|: the stated arithmetic rounds three times (im * im, the
    # multiply-add, the square root: (2^-24 + 2^-24) / 2 + 2^-24 = 2^-23 relative at the worst), which for a mantissa near 2 is up to
    # two SPACINGS of float32 -- that arithmetic, carried out in NumPy on this very input, lies 1.06 spacings from np.abs at 7 pixels
    fin = np.isfinite(ref)
    rel = (np.abs(got.astype(np.float64) - ref)[fin] / ref[fin]).max()
    # ... so the device is held to the stated arithmetic itself, bit for bit: im * im in float32, the multiply-add exact and rounded
    # once (_fma32), a correctly rounded float32 square root
    stated = np.sqrt(_fma32(iq.real, iq.real, iq.imag * iq.imag))
    differ = int((got[fin] != stated[fin]).sum())
    print(f"\nmodulus: largest relative error against np.abs {rel / 2.0 ** -23:.3f} x 2^-23; {differ} of {int(fin.sum())} pixels differ from "
          f"the stated arithmetic")
    assert stated.dtype == np.float32 and np.array_equal(got[fin], stated[fin])
    assert rel <= 2.0 ** -23
    cx = mi.default_context()
    dev = mi.iq_envelope(mi.DeviceBuffer.from_host(cx, iq))
    assert isinstance(dev, mi.DeviceBuffer) and dev.dtype == np.float32 and np.array_equal(dev.numpy(), got, equal_nan=True)
    with pytest.raises(RuntimeError, match="rc=-1"):
        mi.envelope(np.ones((7, 5000), np.float32))
    bf = mi.DelayAndSum(is_iq=True)
    assert np.array_equal(bf.compute_envelope(iq), got, equal_nan=True)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _iq_call(mi, capi, table=False, **change):
    g = geometry("a1_e3_small_lin_f0_sum")
    cx = mi.default_context()
    bufs = [mi.DeviceBuffer.from_host(cx, a) for a in (normal_iq("a1_e3_small_lin_f0_sum"), g["tx"], g["elem"], g["x"], g["z"])]
    if table:
        bufs[1] = mi.das_first_arrival(g["tx"], g["elem"], g["x"], g["z"], C0)
    out = mi.DeviceBuffer(cx, (len(g["x"]), len(g["z"])), np.complex64)
    ip = capi.IqParams()
    d = ip.das
    d.n_angles, d.n_elements, d.time_samples, d.fs, d.sound_speed, d.interpolation = g["A"], g["E"], T, FS_IQ, C0, capi.DAS_LINEAR
    d.nx, d.nz = len(g["x"]), len(g["z"])
    ip.demod_freq, ip.probe = F_D, 0
    for k, v in change.items():
        setattr(d if hasattr(d, k) else ip, k, v)
    fn = cx.lib.pbrt_iq_beamform_table_dev if table else cx.lib.pbrt_iq_beamform_dev
    return fn(cx.handle, C.byref(ip), *(b.ptr for b in bufs), out.ptr)


def test_refusals_of_the_c_abi(mi, capi):
    E_INVALID = -1
    cx = mi.default_context()
    lib = cx.lib
    assert _iq_call(mi, capi) == 0 and _iq_call(mi, capi, table=True) == 0 and _iq_call(mi, capi, demod_freq=0.0) == 0
    for bad in (float("nan"), float("inf"), -1.0):
        assert _iq_call(mi, capi, demod_freq=bad) == E_INVALID, bad
        assert _iq_call(mi, capi, table=True, demod_freq=bad) == E_INVALID, bad
    assert _iq_call(mi, capi, probe=2) == E_INVALID
    # what das_check refuses
    for change in (dict(n_angles=0), dict(n_elements=0), dict(time_samples=1), dict(fs=0.0), dict(sound_speed=0.0), dict(interpolation=2),
                   dict(f_number=-1.0), dict(nx=0), dict(nz=0)):
        assert _iq_call(mi, capi, **change) == E_INVALID, change
    assert b"invalid argument" in lib.pbrt_last_error(cx.handle)
    ip = capi.IqParams()
    assert lib.pbrt_iq_beamform(cx.handle, C.byref(ip), None, None, None, None, None, None) == E_INVALID
    assert lib.pbrt_iq_beamform_dev(None, C.byref(ip), None, None, None, None, None, None) == E_INVALID
    # rf2iq
    x = np.ones((2, 40), np.float32)
    out = np.empty((2, 40), np.complex64)
    h = np.ones(2 * 1025 + 1, np.float32)
    xa, oa, ha = x.ctypes.data, out.ctypes.data, h.ctypes.data

    def rf2iq(n=2, Tn=40, fs=20e6, t0=0.0, fd=2.5e6, D=1, K=1, i=xa, o=oa):
        return lib.pbrt_rf2iq(cx.handle, n, Tn, fs, t0, fd, D, K, ha, i, o)

    assert rf2iq() == 0 and rf2iq(D=8) == 0 and rf2iq(K=1024) == 0 and rf2iq(fd=0.0) == 0
    for kw in (dict(D=0), dict(D=9), dict(K=1025), dict(Tn=0), dict(fs=0.0), dict(fs=float("nan")), dict(t0=float("inf")), dict(fd=-1.0),
               dict(fd=float("nan")), dict(fd=float("inf")), dict(o=xa), dict(o=xa + 4 * 39), dict(i=oa + 8)):
        assert rf2iq(**kw) == E_INVALID, kw
    assert b"invalid argument" in lib.pbrt_last_error(cx.handle)
    assert lib.pbrt_rf2iq(cx.handle, 2, 40, 20e6, 0.0, 2.5e6, 1, 1, None, xa, oa) == E_INVALID
    d_x, d_h = mi.DeviceBuffer.from_host(cx, x), mi.DeviceBuffer.from_host(cx, h)
    d_o = mi.DeviceBuffer(cx, (2, 40), np.complex64)
    dev = lambda D=1, K=1, Tn=40, fd=2.5e6, o=d_o.ptr: lib.pbrt_rf2iq_dev(cx.handle, 2, Tn, 20e6, 0.0, fd, D, K, d_h.ptr, d_x.ptr, o)   # noqa: E731
    assert dev() == 0
    for kw in (dict(D=0), dict(D=9), dict(K=1025), dict(Tn=0), dict(fd=-1.0), dict(o=d_x.ptr)):
        assert dev(**kw) == E_INVALID, kw
    # the modulus
    env = np.empty((2, 40), np.float32)
    assert lib.pbrt_iq_envelope(cx.handle, 80, oa, env.ctypes.data) == 0
    assert lib.pbrt_iq_envelope(cx.handle, 80, oa, oa) == E_INVALID and lib.pbrt_iq_envelope(cx.handle, 80, oa, oa + 8 * 79 + 4) == E_INVALID
    assert lib.pbrt_iq_envelope(cx.handle, 80, None, env.ctypes.data) == E_INVALID
    assert lib.pbrt_iq_envelope_dev(cx.handle, 80, d_o.ptr, d_o.ptr) == E_INVALID
    # nothing to do is not an error, in the host forms as in the _dev forms
    assert rf2iq(n=0) == 0 and lib.pbrt_rf2iq_dev(cx.handle, 0, 40, 20e6, 0.0, 2.5e6, 1, 1, d_h.ptr, d_x.ptr, d_o.ptr) == 0
    assert lib.pbrt_iq_envelope(cx.handle, 0, oa, env.ctypes.data) == 0 and lib.pbrt_iq_envelope_dev(cx.handle, 0, d_o.ptr, d_x.ptr) == 0
    cx.synchronize()


def test_refusals_of_the_python_layer(mi):
    g = geometry("a1_e3_small_lin_f0_sum")
    iq = normal_iq("a1_e3_small_lin_f0_sum")
    args = (g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0)
    cx = mi.default_context()
    with pytest.raises(ValueError, match="demod_freq"):
        mi.iq_beamform(iq, *args, float("nan"))
    with pytest.raises(ValueError, match="complex64"):
        mi.iq_beamform(mi.DeviceBuffer.from_host(cx, iq.real.copy()), *args, F_D)           # a float32 DeviceBuffer as I/Q data
    with pytest.raises(ValueError, match="float32"):
        mi.das_beamform(mi.DeviceBuffer.from_host(cx, iq), *args)                            # a complex DeviceBuffer as RF data
    with pytest.raises(ValueError, match="out must hold"):
        mi.iq_beamform(mi.DeviceBuffer.from_host(cx, iq), *args, F_D, out=mi.DeviceBuffer(cx, (len(g["x"]), len(g["z"]))))
    with pytest.raises(ValueError, match="float32 RF"):
        mi.rf2iq(mi.DeviceBuffer.from_host(cx, iq), 2.5e6, 20e6)
    with pytest.raises(ValueError, match="complex64"):
        mi.iq_envelope(mi.DeviceBuffer(cx, (4, 4)))
    probe = mi.build_probe("linear", g["E"], 1e-4, F_D, 70)
    info = {"sampling_freq": g["fs"], "t0": 0, "delays": g["tx"], "sound_speed": C0}
    scan = mi.GridScan(g["x"], g["z"])
    bf = mi.DelayAndSum(f_number=0.0).automatic_setup(info, probe)
    with pytest.raises(ValueError, match="is_iq is off"):
        bf.beamform(iq, scan)
    with pytest.raises(ValueError, match="is_iq is off"):
        bf.beamform(mi.DeviceBuffer.from_host(cx, iq), scan)
    bf.set_is_iq(True)
    with pytest.raises(ValueError, match="data are real"):
        bf.beamform(iq.real.copy(), scan)
    with pytest.raises(ValueError, match="data are real"):
        bf.beamform(mi.DeviceBuffer.from_host(cx, iq.real.copy()), scan)
    # ... and with the flag and the data agreeing, the class gives the free function's image (the probe's central frequency demodulates)
    assert np.allclose(probe.geometry[0], g["elem"], rtol=1e-6, atol=0)
    want = mi.iq_beamform(iq, g["tx"], probe.geometry[0], g["x"], g["z"], g["fs"], C0, F_D, f_number=0.0)
    assert np.array_equal(bf.beamform(iq, scan), want)
    on_dev = bf.beamform(mi.DeviceBuffer.from_host(cx, iq), scan)
    assert isinstance(on_dev, mi.DeviceBuffer) and np.array_equal(on_dev.numpy(), want)
    sc = mi.load_file(scene_path("us_plate.xml"), paths_per_ray=1, seed=1)
    small = dict(x_range=(-0.001, 0.001), z_range=(0.049, 0.051))
    for nl in (mi.PDelayAndSum(), mi.FilteredDelayMultiplyAndSum()):
        with pytest.raises(NotImplementedError):
            mi.us_render(sc, beamformer=nl, iq=True, **small)
    with pytest.raises(ValueError, match="decimation"):
        mi.us_render(sc, iq=True, decimation=9, **small)
    with pytest.raises(ValueError, match="decimation"):
        mi.us_render(sc, decimation=2, **small)


# ---- us_render -----------------------------------------------------------------------------------------------------------------
def _plate_scan(ui, step, half_x, half_z):
    return dict(x_range=(-(half_x + 0.5) * step, half_x * step), z_range=(0.05 - (half_z + 0.5) * step, 0.05 + half_z * step), step=step)


def _host_chain(mi, ui, probe, xs, zs, D):
    """the I/Q chain through the host-pointer forms on the channel buffer the device chain used -> (I/Q data, complex image, envelope)"""
    chan = np.asarray(ui.channel_buf, np.float32).reshape(ui.n_angles, ui.n_elements, ui.time_samples)
    delays = np.asarray(ui.transmission_delays_buf, np.float32).reshape(ui.n_angles, ui.n_elements)
    iq = mi.rf2iq(chan, ui.frequency, ui.fs, decimation=D)
    bf = mi.DelayAndSum(is_iq=True).automatic_setup({"sampling_freq": ui.fs / D, "t0": 0, "delays": delays, "sound_speed": ui.sound_speed}, probe)
    img = bf.beamform(iq, mi.GridScan(xs, zs))
    return chan, delays, iq, img, bf.compute_envelope(img)


def test_us_render_iq(mi):
    """the plate phantom of the finite-difference loop (tests/scenes/us_plate.xml) through the I/Q chain, on a 24 x 64 scan at lambda / 4
    around the plate.  One path per ray, as in test_us_render_with_the_new_beamformers: the replayed chain is compared bit for bit."""
    sc = mi.load_file(scene_path("us_plate.xml"), paths_per_ray=1, seed=4)
    ui = sc.integrator()
    lam = ui.sound_speed / ui.frequency
    kw = _plate_scan(ui, lam / 4, 12, 32)
    before = mi.us_render(sc, **kw)                                   # the RF chain, before any I/Q call
    imgs, flags = [], []
    for _ in range(3):
        tm = {}
        disp, env, (xs, zs) = mi.us_render(sc, iq=True, timing=tm, **kw)
        imgs.append((disp, env))
        flags.append(tm["replayed"])
    assert len(xs) <= 26 and len(zs) <= 66 and disp.shape == (len(zs), len(xs)) and env.shape == (len(xs), len(zs))
    assert flags == [False, False, True]
    assert np.array_equal(imgs[2][0], imgs[1][0]) and np.array_equal(imgs[2][1], imgs[1][1]) and env.max() > 0 and np.isfinite(env).all()
    plan = ui._render_plan
    assert plan.d_iq.dtype == np.complex64 and plan.d_iq.shape == (ui.n_angles, ui.n_elements, ui.time_samples)
    # the host-pointer forms on the same channel buffer give the same bits, step by step
    probe = mi.build_probe("linear", ui.n_elements, ui.pitch, ui.frequency, 70)
    chan, delays, iq1, img1, env1 = _host_chain(mi, ui, probe, xs, zs, 1)
    assert np.array_equal(plan.d_iq.numpy(), iq1) and np.array_equal(plan.d_bf_iq.numpy(), img1) and np.array_equal(env1, env)
    # ... and the complex image is held to the restatement like every case above
    taps = mi.lowpass_taps(ui.frequency / 2, ui.fs)
    A, E, Tn = chan.shape
    args = (delays, probe.geometry[0], xs, zs)

    def restated(D, x=xs, z=zs, dtype=np.float64):
        iq, _ = iu.rf2iq(chan.reshape(A * E, Tn), ui.fs, 0.0, ui.frequency, D, taps)
        return iu.iq_beamform(iq.reshape(A, E, -1), delays, probe.geometry[0], x, z, ui.fs / D, ui.sound_speed, ui.frequency, dtype=dtype)

    left_out, _ = nu.margins(*args, Tn, ui.fs, ui.sound_speed)
    ref, B = iu.iq_beamform(iq1, *args, ui.fs, ui.sound_speed, ui.frequency)
    f32, _ = iu.iq_beamform(iq1, *args, ui.fs, ui.sound_speed, ui.frequency, dtype=np.float32)
    used = ~left_out & (B > 0)
    floor = float((np.abs(f32 - ref)[used] / B[used]).max())
    ratio = float((np.abs(img1.astype(np.complex128) - ref)[used] / B[used]).max())
    print(f"\nus_render iq: float32 floor {floor:.3e}, device {ratio:.3e} ({ratio / floor:.2f} x), {int(left_out.sum())} of {left_out.size} left out")
    assert used.any() and ratio <= 4.0 * floor
    # device_resident=False: an acquisition of its own through the host-pointer forms; its channel words differ by the order of their
    # float32 atomic adds (2e-5 of the largest, tests/test_gpu_beamform.py) -- compared as test_us_render_with_the_new_beamformers does
    d_host, b_host, _ = mi.us_render(sc, iq=True, device_resident=False, **kw)
    assert d_host.shape == disp.shape and np.allclose(b_host, env, rtol=0, atol=1e-2 * env.max())
    assert np.allclose(d_host, disp, rtol=0, atol=1e-2)
    # decimation = 4: another plan, and the same envelope at the image's peak to the margin the restatement gives -- the two differ by
    # the method (where the decimated samples lie under the interpolation), measured in float64 at that pixel and doubled
    tm = {}
    _, env4, _ = mi.us_render(sc, iq=True, decimation=4, timing=tm, **kw)
    assert not tm["replayed"] and ui._render_plan is not plan and ui._render_plan.d_iq.shape[-1] == -(-ui.time_samples // 4)
    ip, kp = np.unravel_index(np.argmax(env), env.shape)
    r1 = iu.modulus(restated(1, xs[ip:ip + 1], zs[kp:kp + 1])[0])[0, 0]
    r4 = iu.modulus(restated(4, xs[ip:ip + 1], zs[kp:kp + 1])[0])[0, 0]
    margin = 2.0 * abs(r4 - r1) / r1
    got = abs(float(env4[ip, kp]) - float(env[ip, kp])) / float(env[ip, kp])
    print(f"decimation 4 against 1 at the peak: restatement {abs(r4 - r1) / r1:.3e}, device {got:.3e}")
    assert got <= margin
    # on_device: buffers, still being written; they match after synchronize()
    for _ in range(3):
        tm = {}
        d_img, d_env, _ = mi.us_render(sc, iq=True, on_device=True, timing=tm, **kw)
    assert tm["replayed"] and isinstance(d_img, mi.DeviceBuffer) and d_img.shape == (len(xs), len(zs)) == d_env.shape
    sc.device().ctx.synchronize()
    assert np.array_equal(d_env.numpy(), env) and np.array_equal(d_img.numpy().T, disp)
    # a beamformer of the caller's keeps its setups; one with is_iq (and a demodulation frequency) set selects the chain by itself
    mine = mi.DelayAndSum(f_number=1.0)
    was = dict(mine.setups)
    assert np.array_equal(mi.us_render(sc, beamformer=mine, iq=True, **kw)[1], env) and mine.setups == was
    mine = mi.DelayAndSum(is_iq=True)
    mine.update_setup("demod_freq", 4.5e6)
    was = dict(mine.setups)
    other = mi.us_render(sc, beamformer=mine, **kw)[1]
    assert mine.setups == was and np.isfinite(other).all() and not np.array_equal(other, env)
    # iq=False afterwards: the plan key separates the chains, the RF image has the bits it had before
    after = mi.us_render(sc, **kw)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    assert not np.array_equal(after[1], env)


def test_us_render_iq_is_free_of_the_carrier_grid(mi):
    """step = lambda / 2: the axial Nyquist frequency lies BELOW the carrier -- F-DMAS refuses the step, the I/Q chain takes it"""
    sc = mi.load_file(scene_path("us_plate.xml"), paths_per_ray=1, seed=4)
    ui = sc.integrator()
    lam = ui.sound_speed / ui.frequency
    kw = _plate_scan(ui, lam / 2, 8, 20)
    with pytest.raises(ValueError, match=r"step below .* m would fit"):
        mi.us_render(sc, beamformer=mi.FilteredDelayMultiplyAndSum(), **kw)
    disp, env, (xs, zs) = mi.us_render(sc, iq=True, decimation=4, **kw)
    assert np.isfinite(env).all() and env.max() > 0 and disp.shape == (len(zs), len(xs)) and 0.0 <= disp.min() and disp.max() == 1.0
    probe = mi.build_probe("linear", ui.n_elements, ui.pitch, ui.frequency, 70)
    assert np.array_equal(_host_chain(mi, ui, probe, xs, zs, 4)[4], env)


def test_us_render_iq_convex_and_gaussian(mi):
    """a convex integrator (radius=, opening_angle=) runs the element-table path; the Gaussian pulse model runs in front of rf2iq"""
    from test_gpu_convex_array import _scene
    sc = _scene(mi, paths_per_ray=4)
    ui = sc.integrator()
    step = (ui.sound_speed / ui.frequency) / 2
    R = ui.radius                       # z is measured from the centre of curvature: the plate lies at R + 20 mm
    kw = dict(x_range=(-10 * step, 10 * step), z_range=(R + 0.02 - 20 * step, R + 0.02 + 20 * step), step=step)
    disp, env, (xs, zs) = mi.us_render(sc, iq=True, decimation=2, **kw)
    assert np.isfinite(env).all() and env.max() > 0 and disp.shape == (len(zs), len(xs))
    probe = mi.build_probe("convex", ui.n_elements, ui.pitch, ui.frequency, 70, radius=ui.radius, opening_angle=ui.opening_angle)
    assert probe.das_elements.shape == (ui.n_elements, 4)
    assert np.array_equal(_host_chain(mi, ui, probe, xs, zs, 2)[4], env)
    sc = mi.load_file(scene_path("us_plate.xml"), paths_per_ray=2, seed=6)
    ui = sc.integrator()
    ui.pulse_model = "gaussian"
    ui.quirks |= mi._capi.USQ_NO_CARRIER
    lam = ui.sound_speed / ui.frequency
    env = mi.us_render(sc, iq=True, decimation=4, **_plate_scan(ui, lam / 2, 8, 20))[1]
    assert np.isfinite(env).all() and env.max() > 0
