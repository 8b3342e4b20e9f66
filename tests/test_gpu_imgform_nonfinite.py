"""Non-finite and rescaled samples through the walk (delay-and-sum, p-DAS, F-DMAS, I/Q delay-and-sum), k_axial_fir and k_rf2iq on the
device.  include/pbrt_hip.h: "Non-finite samples get no special treatment" -- and by DESIGN.md D12 the channel buffer of an ordinary
plate phantom holds NaN echoes, so NaN is a legitimate input.  What a pixel must be is the stated arithmetic's answer, which the float32
restatements of tests/nlbf_util.py and tests/iq_util.py carry out; tests/test_imgform_nonfinite_restatement.py pins on the CPU that
their float64 forms agree with them, and defines the cases, sites, shapes and data used here.

  A  2 - 6 bad samples (NaN, +inf, -inf) in standard-normal data, pixel by pixel: the device's class (finite, NaN, +inf, -inf) of every
     kept pixel and component is the restatement's, every pixel the restatement leaves finite has the bits of the clean data's image,
     and the table and host forms equal the plain one
  B  every sample NaN: NaN where a kept pixel uses an element, +0.0 elsewhere -- a tile that leaves early and an element outside the
     aperture are never read
  C  one bad sample through k_axial_fir and k_rf2iq: non-finite exactly at |n - j| <= K (|m D - j| <= K), every other output has the
     clean run's bits
  D  data times 4^+-30: the image scales bit for bit (p-DAS at p = 3, whose powf is not exactly homogeneous: the 4 x float32-floor
     scheme of test_gpu_nlbf.py on the scaled data)
  E  k_rf2iq at every decimation 1 .. 8, with full and partial last windows and an output count at and just past a workgroup
  F  the D12 plate phantom through us_render with p-DAS, F-DMAS and the I/Q chain at decimation 1 and 4
and the refusals of overlapping buffers and of an `out` of the wrong size in axial_fir.

Pixels left out: those of nlbf_util.margins and those with a pair next to a bad sample within das_util.EDGE_SAMPLES of a whole (half)
sample (nlbf_util.near_bad, bad_reads); never more than the project's 2 % (the restatement leaves out none for the bad samples)."""
import numpy as np
import pytest

import iq_util as iu
import nlbf_util as nu
from oracle import beamform as obf
from test_imgform_nonfinite_restatement import (BAD, CAP, F_D, FIR_SHAPES, IQ_PARTS, METHODS, NAMES, RF2IQ_FD, RF2IQ_FS, RF2IQ_SHAPES,
                                                RF2IQ_T0, SCALES, bad_indices, bad_iq, clean, clean_iq, expected, expected_iq, fir_input,
                                                restated, sites)
from walk_cases import C0, T, geometry

pytestmark = pytest.mark.gpu

BAD_IDS = ["nan", "plus_inf", "minus_inf"]
E_INVALID = -1


def bits(a):
    """the words of a float32 or complex64 array, [..., 1] or [..., 2]"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(a.shape + (a.dtype.itemsize // 4,))


_tables = {}


def image(mi, name, data, method, p=2.0, form="dev"):
    """the library's image of a case: method 'das' | 'pdas' | 'fdmas' | 'iq'; form 'dev', 'table' (the first-arrival table) or 'host'"""
    g = geometry(name)
    args = (g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0)
    if method == "iq":
        fn, args, kw = mi.iq_beamform, args + (F_D,), g["kw"]
    elif method == "das":
        fn, kw = mi.das_beamform, g["kw"]
    else:
        fn, kw = mi.nonlinear_beamform, dict(g["kw"], method=method, p=p)
    if form == "host":
        return fn(data, *args, **kw)
    cx = mi.default_context()
    table = None
    if form == "table":
        if name not in _tables:
            _tables[name] = mi.das_first_arrival(g["tx"], g["elem"], g["x"], g["z"], C0)
        table = _tables[name]
    return fn(mi.DeviceBuffer.from_host(cx, data), *args, table=table, **kw).numpy()


_clean_images = {}


def clean_image(mi, name, method, p=2.0):
    key = (name, method, p)
    if key not in _clean_images:
        _clean_images[key] = image(mi, name, clean_iq(name) if method == "iq" else clean(name), method, p)
        assert np.isfinite(_clean_images[key]).all()
    return _clean_images[key]


def _check_classes(mi, name, data, method, p, want, kept, label):
    got = image(mi, name, data, method, p)
    ref = clean_image(mi, name, method, p)
    cls = nu.classes(got)
    wrong = kept & (cls != want).reshape(kept.shape + (-1,)).any(axis=-1)
    assert not wrong.any(), (label, np.argwhere(wrong)[:8].tolist(), cls[wrong][:8].tolist(), want[wrong][:8].tolist())
    finite = kept & (want == nu.FINITE).reshape(kept.shape + (-1,)).all(axis=-1)
    assert finite.any() and np.array_equal(bits(got)[finite], bits(ref)[finite]), label
    for form in ("table", "host"):
        assert np.array_equal(image(mi, name, data, method, p, form), got, equal_nan=True), (label, form)
    return int((kept & ~finite).sum())


# ---- A ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", range(len(BAD)), ids=BAD_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_a_bad_sample_pixel_by_pixel(mi, name, bad):
    where, idle, kept = sites(name)
    value = BAD[bad]
    assert 1.0 - kept.mean() <= CAP
    hit = []
    for method, p in METHODS:
        hit.append(_check_classes(mi, name, nu.with_bad(clean(name), where, value), method, p, expected(name, bad, method, p), kept,
                                  (name, value, method, p)))
    for part in IQ_PARTS:
        hit.append(_check_classes(mi, name, bad_iq(clean_iq(name), where, value, part), "iq", 0.0, expected_iq(name, bad, part), kept,
                                  (name, value, "iq", part)))
    print(f"\n{name} {BAD_IDS[bad]}: {len(where)} sites, {int((~kept).sum())} of {kept.size} pixels left out, non-finite pixels per method "
          f"(das, p-DAS 2, p-DAS 3, F-DMAS, I/Q re / im / both) {hit}")
    assert min(hit) > 0


# ---- B ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_sample_nan(mi, name):
    g = geometry(name)
    keep = ~g["left_out"]
    uses = g["n_a"].sum(axis=0) > 0
    if name == "a6_e3_wide_lin_f1_mean":
        assert not uses[:8].any() and not uses[16:].any() and uses[8:16].any()        # the outer x tiles see no element
    rf = np.full((g["A"], g["E"], T), np.nan, np.float32)
    iq = np.full((g["A"], g["E"], T), np.nan + 1j * np.nan, np.complex64)
    for method, p in METHODS + (("iq", 0.0),):
        for form in ("dev", "table"):
            got = bits(image(mi, name, iq if method == "iq" else rf, method, p, form))
            nan = ((got & 0x7FFFFFFF) > 0x7F800000).all(axis=-1)
            zero = (got == 0).all(axis=-1)                                           # +0.0 in every component: no bit set
            assert np.array_equal(nan[keep], uses[keep]) and np.array_equal(zero[keep], ~uses[keep]), (name, method, p, form)


# ---- C ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nz,K", FIR_SHAPES)
def test_axial_fir_one_bad_sample(mi, nx, nz, K):
    x, h = fir_input(nx, nz, K)
    ref = mi.axial_fir(x, h)
    assert np.isfinite(ref).all()
    cx = mi.default_context()
    for j in bad_indices(nz):
        mask = nu.fir_bad_mask(nz, K, j)
        for value in BAD:
            xb = x.copy()
            xb[nx - 1, j] = value
            got = mi.axial_fir(xb, h)
            assert np.array_equal(~np.isfinite(got[nx - 1]), mask), (j, value)
            assert np.array_equal(bits(got[nx - 1][~mask]), bits(ref[nx - 1][~mask])) and np.array_equal(bits(got[:nx - 1]), bits(ref[:nx - 1]))
            if np.isnan(value):
                assert np.isnan(got[nx - 1][mask]).all()
            else:      # one infinite product per output, which every later multiply-add keeps: the tap's sign times the sample's
                n = np.arange(nz)[mask]
                assert np.array_equal(got[nx - 1][mask], np.sign(h[K + n - j]) * np.float32(value)), (j, value)
            if j == nz // 2:
                dev = mi.axial_fir(mi.DeviceBuffer.from_host(cx, xb), h).numpy()
                assert np.array_equal(dev, got, equal_nan=True)


@pytest.mark.parametrize("n,Tn,K,D", RF2IQ_SHAPES)
def test_rf2iq_one_bad_sample(mi, n, Tn, K, D):
    x, h = fir_input(n, Tn, K)
    kw = dict(t0=RF2IQ_T0, decimation=D, taps=h)
    ref = mi.rf2iq(x, RF2IQ_FD, RF2IQ_FS, **kw)
    assert np.isfinite(ref).all()
    for j in bad_indices(Tn, D):
        mask = iu.rf2iq_bad_mask(Tn, K, D, j)
        for value in BAD:
            xb = x.copy()
            xb[n - 1, j] = value
            got = mi.rf2iq(xb, RF2IQ_FD, RF2IQ_FS, **kw)
            with np.errstate(invalid="ignore"):
                want = nu.classes(iu.rf2iq(xb, RF2IQ_FS, RF2IQ_T0, RF2IQ_FD, D, h, dtype=np.float32)[0])
            cls = nu.classes(got)
            assert np.array_equal((cls[n - 1] != nu.FINITE).any(axis=-1), mask), (j, value)
            assert np.array_equal(cls, want), (j, value)
            assert np.array_equal(bits(got[n - 1][~mask]), bits(ref[n - 1][~mask])) and np.array_equal(bits(got[:n - 1]), bits(ref[:n - 1]))
            if np.isnan(value):
                assert np.all(cls[n - 1][mask] == nu.NAN)


# ---- D ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_rescaled_data_scale_the_image_bit_for_bit(mi, name):
    g = geometry(name)
    data, iq = clean(name), clean_iq(name)
    keep = ~g["left_out"]
    for s in SCALES:
        s32 = np.float32(s)
        for method, p in (("das", 1.0), ("pdas", 2.0), ("fdmas", 2.0)):
            want = s32 * clean_image(mi, name, method, p)
            assert np.isfinite(want).all() and np.array_equal(bits(image(mi, name, data * s32, method, p)), bits(want)), (name, s, method)
        want = (s32 * clean_image(mi, name, "iq")).astype(np.complex64)
        assert np.array_equal(bits(image(mi, name, iq * s32, "iq")), bits(want)), (name, s, "iq")
        # p = 3: powf is not exactly homogeneous -- the scheme of test_gpu_nlbf.py on the scaled data
        scaled = data * s32
        ref, B = restated(name, "pdas", 3.0, scaled, np.float64)
        f32, _ = restated(name, "pdas", 3.0, scaled, np.float32)
        got = image(mi, name, scaled, "pdas", 3.0)
        used = keep & (B > 0)
        floor = float((np.abs(f32.astype(np.float64) - ref)[used] / B[used]).max())
        ratio = float((np.abs(got.astype(np.float64) - ref)[used] / B[used]).max())
        print(f"\n{name} x {s:.3e} pdas p=3: float32 floor {floor:.3e}, device {ratio:.3e} ({ratio / floor:.2f} x), {int(used.sum())} pixels")
        assert used.any() and ratio <= 4.0 * floor, (name, s, ratio, floor)


@pytest.mark.parametrize("nx,nz,K", FIR_SHAPES)
def test_rescaled_columns_scale_the_fir_bit_for_bit(mi, nx, nz, K):
    x, h = fir_input(nx, nz, K)
    ref = mi.axial_fir(x, h)
    for s in SCALES:
        s32 = np.float32(s)
        assert np.array_equal(bits(mi.axial_fir(x * s32, h)), bits(s32 * ref)), s


@pytest.mark.parametrize("n,Tn,K,D", RF2IQ_SHAPES)
def test_rescaled_traces_scale_rf2iq_bit_for_bit(mi, n, Tn, K, D):
    x, h = fir_input(n, Tn, K)
    kw = dict(t0=RF2IQ_T0, decimation=D, taps=h)
    ref = mi.rf2iq(x, RF2IQ_FD, RF2IQ_FS, **kw)
    for s in SCALES:
        s32 = np.float32(s)
        assert np.array_equal(bits(mi.rf2iq(x * s32, RF2IQ_FD, RF2IQ_FS, **kw)), bits((s32 * ref).astype(np.complex64))), s


# ---- E ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", range(1, 9))
def test_rf2iq_at_every_decimation(mi, D):
    """T = 256 D + r, r in {0, 1, D - 1}: Td = 256 fills one workgroup (r = 0) or starts a second one with one output whose window is
    partial (r >= 1); K in {0, 3, 40}; t0 in {0, -1.3 us}.  The rule is test_rf2iq's: 4 x the float32 floor."""
    cx = mi.default_context()
    fs, f_d, n = 20.0e6, 2.3e6, 2
    worst = (0.0, None)
    for r in sorted({0, 1, D - 1}):
        Tn = 256 * D + r
        for K in (0, 3, 40):
            rng = np.random.default_rng(D * 10000 + r * 100 + K)
            x = rng.standard_normal((n, Tn)).astype(np.float32)
            h = (rng.standard_normal(2 * K + 1) / np.sqrt(2 * K + 1)).astype(np.float32)
            for t0 in (0.0, -1.3e-6):
                got = mi.rf2iq(x, f_d, fs, t0=t0, decimation=D, taps=h)
                Td = -(-Tn // D)
                assert got.shape == (n, Td) and got.dtype == np.complex64 and Td == (256 if r == 0 else 257)
                ref, B = iu.rf2iq(x, fs, t0, f_d, D, h)
                f32, _ = iu.rf2iq(x, fs, t0, f_d, D, h, dtype=np.float32)
                used = B > 0
                floor = float((np.abs(f32 - ref)[used] / B[used]).max())
                ratio = float((np.abs(got.astype(np.complex128) - ref)[used] / B[used]).max())
                print(f"\nrf2iq D={D} T={Tn} K={K} t0={t0}: float32 floor {floor:.3e}, device {ratio:.3e} ({ratio / floor:.2f} x)")
                worst = max(worst, (ratio / floor, (r, K, t0)))
                assert used.all() and ratio <= 4.0 * floor, (D, r, K, t0, ratio, floor)
                dev = mi.rf2iq(mi.DeviceBuffer.from_host(cx, x), f_d, fs, t0=t0, decimation=D, taps=h)
                assert dev.shape == (n, Td) and np.array_equal(bits(dev.numpy()), bits(got))
    print(f"rf2iq D={D}: largest device / floor {worst[0]:.2f} at (r, K, t0) = {worst[1]}")


# ---- F ------------------------------------------------------------------------------------------------------------------------
def _d12_scene(mi, **integrator):
    """the scene of test_d12_nan_echoes_reach_the_display_as_in_the_f64_chain: the 0-degree plane wave meets a plate that faces the probe
    exactly, and every element's trace of that transmission holds NaN echoes from sample 800 (2 x 15 mm at 1500 m/s and 40 MHz) on.
    `integrator`: entries of the integrator's dict to replace (test_gpu_doppler_edges.py: the pulse model and the 0-degree angle alone)"""
    Tf = mi.ScalarTransform4f
    return mi.load_dict({
        "type": "scene",
        "integrator": {"type": "ultrasound_integrator", "max_depth": 4, "sampling_rate": 40e6, "frequency": 4e6, "sound_speed": 1500,
                       "attenuation": 0.1, "main_beam_angle": 20, "cutoff_angle": 35, "n_elements": 32, "pitch": 2e-4,
                       "time_samples": 4000, "angles": [-5.0, 0.0, 5.0], "paths_per_ray": 50, "seed": 9, **integrator},
        "sensor": {"type": "ultrasound_sensor", "to_world": Tf().look_at([0, 0, 0], [0, 0, 0.03], [0, 1, 0])},
        "p": {"type": "rectangle", "to_world": Tf().translate([0, 0, 0.015]) @ Tf().rotate([1, 0, 0], 180) @ Tf().scale([0.03, 0.03, 1]),
              "bsdf": {"type": "ultrasound_bsdf", "impedance": 7.8, "roughness": 0.9}}})


def _d12_buffers(mi, ui):
    chan = np.asarray(ui.channel_buf, np.float32).reshape(3, 32, 4000)
    assert np.isnan(chan[1]).any(axis=1).all() and not np.isnan(chan[[0, 2]]).any() and not np.isinf(chan).any()
    delays = np.asarray(ui.transmission_delays_buf, np.float32).reshape(3, 32)
    probe = mi.build_probe("linear", 32, ui.pitch, ui.frequency, 70)
    return chan, delays, probe


@pytest.mark.parametrize("which", ["pdas", "fdmas"])
def test_d12_nan_echoes_through_the_non_linear_chains(mi, which):
    """64 x 200 pixels at lambda / 16 (the step of test_us_render_with_the_new_beamformers, so that the bands fit), ending 0.3 mm above
    the plate and 0.2 - 1.7 mm off axis: a column reads sample 800 of the farthest element only from about 1 mm off axis on, so the
    scan holds clean columns and NaN columns.  The band-pass spreads a NaN over |n - j| <= K and the envelope over its column."""
    sc = _d12_scene(mi)
    ui = sc.integrator()
    step = (ui.sound_speed / ui.frequency) / 16
    bf = mi.PDelayAndSum(p=2.0) if which == "pdas" else mi.FilteredDelayMultiplyAndSum()
    display, env, (xs, zs) = mi.us_render(sc, beamformer=bf, x_range=(0.2e-3, 0.2e-3 + 62.5 * step), z_range=(0.0147 - 198.5 * step, 0.0147),
                                          step=step)
    assert env.shape == (64, 200) == (len(xs), len(zs)) and display.shape == (200, 64)
    chan, delays, probe = _d12_buffers(mi, ui)
    taps = bf.filter_taps(mi.GridScan(xs, zs), ui.sound_speed, probe)
    args = (delays, probe.geometry[0], xs, zs, ui.fs, ui.sound_speed)
    with np.errstate(invalid="ignore"):
        env_ref = obf.envelope(nu.fir(nu.beamform(which, chan, *args, p=2.0)[0], taps))
    nan_cols = np.isnan(env_ref).any(axis=1)
    sure, maybe = nu.bad_reads(np.isnan(chan), *args)
    keep = ~(~sure.any(axis=1) & maybe.any(axis=1))                 # a column whose status rests on pairs at a boundary alone is left out
    print(f"\nD12 {which}: {int(nan_cols.sum())} of {len(nan_cols)} columns NaN in the float64 chain, {int((~keep).sum())} left out, "
          f"K = {len(taps) // 2}")
    assert 1.0 - keep.mean() <= CAP and np.array_equal(nan_cols[keep], sure.any(axis=1)[keep])
    assert nan_cols[keep].any() and not nan_cols[keep].all()
    assert np.array_equal(np.isnan(env).any(axis=1)[keep], nan_cols[keep]) and np.array_equal(np.isnan(env).all(axis=1)[keep], nan_cols[keep])
    assert np.isfinite(env[keep & ~nan_cols]).all() and np.isnan(display).all()


@pytest.mark.parametrize("D", [1, 4])
def test_d12_nan_echoes_through_the_iq_chain(mi, D):
    """65 x 76 pixels at lambda / 4 around the plate: the low-pass of rf2iq spreads every NaN echo over |m D - j| <= K of its trace,
    the walk and the modulus keep it per pixel"""
    sc = _d12_scene(mi)
    ui = sc.integrator()
    display, env, (xs, zs) = mi.us_render(sc, iq=True, decimation=D, x_range=(-0.003, 0.003), z_range=(0.012, 0.019))
    chan, delays, probe = _d12_buffers(mi, ui)
    taps = mi.lowpass_taps(ui.frequency / 2, ui.fs)
    A, E, Tn = chan.shape
    args = (delays, probe.geometry[0], xs, zs, ui.fs / D, ui.sound_speed)
    with np.errstate(invalid="ignore"):
        iq = iu.rf2iq(chan.reshape(A * E, Tn), ui.fs, 0.0, ui.frequency, D, taps)[0].reshape(A, E, -1)
        env_ref = iu.modulus(iu.iq_beamform(iq, *args, ui.frequency)[0])
    assert np.array_equal(np.isnan(ui._render_plan.d_iq.numpy()), np.isnan(iq))          # k_rf2iq: NaN exactly at |m D - j| <= K
    nan = np.isnan(env_ref)
    sure, maybe = nu.bad_reads(np.isnan(iq), *args)
    keep = ~(~sure & maybe)
    print(f"\nD12 I/Q D={D}: {int(nan.sum())} of {nan.size} pixels NaN in the float64 chain, {int((~keep).sum())} left out, K = {len(taps) // 2}")
    assert env.shape == nan.shape and 1.0 - keep.mean() <= CAP and np.array_equal(nan[keep], sure[keep])
    assert nan[keep].any() and not nan[keep].all()
    assert np.array_equal(np.isnan(env)[keep], nan[keep]) and np.isfinite(env[keep & ~nan]).all() and np.isnan(display).all()


# ---- overlapping buffers, and an `out` of the wrong size --------------------------------------------------------------------------
def test_overlapping_buffers_are_refused(mi):
    """in and out inside ONE allocation of twice the needed size: nothing a call could write leaves it.  Disjoint halves are accepted;
    out = in + 4 bytes, in = out + 4 bytes and out = in are PBRT_E_INVALID in pbrt_axial_fir(_dev), pbrt_us_apply_pulse(_dev) and
    pbrt_envelope_dev; pbrt_log_compress_dev may take the same buffer."""
    cx = mi.default_context()
    lib = cx.lib
    nx, nz = 2, 40
    n = nx * nz
    host = np.zeros(2 * n, np.float32)
    d_buf = mi.DeviceBuffer.from_host(cx, host)
    h = np.ones(3, np.float32)
    d_h = mi.DeviceBuffer.from_host(cx, h)
    fs, fc, sigma = 50e6, 3e6, 5 / (4 * 3e6)
    calls = {
        "pbrt_axial_fir": (host.ctypes.data, lambda i, o: lib.pbrt_axial_fir(cx.handle, nx, nz, 1, h.ctypes.data, i, o)),
        "pbrt_axial_fir_dev": (d_buf.ptr, lambda i, o: lib.pbrt_axial_fir_dev(cx.handle, nx, nz, 1, d_h.ptr, i, o)),
        "pbrt_us_apply_pulse": (host.ctypes.data, lambda i, o: lib.pbrt_us_apply_pulse(cx.handle, nx, nz, fs, fc, sigma, i, o)),
        "pbrt_us_apply_pulse_dev": (d_buf.ptr, lambda i, o: lib.pbrt_us_apply_pulse_dev(cx.handle, nx, nz, fs, fc, sigma, i, o)),
        "pbrt_envelope_dev": (d_buf.ptr, lambda i, o: lib.pbrt_envelope_dev(cx.handle, nx, nz, i, o)),
    }
    for name, (base, call) in calls.items():
        assert call(base, base + 4 * n) == 0 and call(base + 4 * n, base) == 0, name
        for i, o in ((base, base + 4), (base + 4, base), (base, base), (base, base + 4 * (n - 1)), (base + 4 * (n - 1), base)):
            assert call(i, o) == E_INVALID, (name, i - base, o - base)
        assert b"invalid argument" in lib.pbrt_last_error(cx.handle)
    assert lib.pbrt_log_compress_dev(cx.handle, n, d_buf.ptr, 60.0, d_buf.ptr) == 0
    cx.synchronize()
    assert np.all(host == 0)


def test_axial_fir_checks_the_size_of_out(mi):
    cx = mi.default_context()
    x = mi.DeviceBuffer.from_host(cx, np.ones((3, 40), np.float32))
    h = np.ones(3, np.float32)
    for shape in ((3, 39), (3, 41), (2, 40), (1,)):
        with pytest.raises(ValueError, match="out must hold"):
            mi.axial_fir(x, h, out=mi.DeviceBuffer(cx, shape))
    out = mi.DeviceBuffer(cx, (3, 40))
    assert mi.axial_fir(x, h, out=out) is out and np.array_equal(out.numpy(), mi.axial_fir(np.ones((3, 40), np.float32), h))
