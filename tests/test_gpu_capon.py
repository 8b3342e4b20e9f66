"""Capon (minimum-variance) beamforming on the device: k_capon_beamform against the float64 restatement of
tests/capon_util.py on the walk cases, the bit-equalities of the call forms, what follows from the definition (L = 1 is I/Q
delay-and-sum, constant traces, exact zeros, non-finite samples), the refusals, the point scatterer, the classes and us_render.

The geometries are walk_cases.CASES, for the reasons that file states: N = 3 (L = 1), tiles with no element, N up to 39, a second block
of elements with N = 65 (L = 32), a third with N = 130 (the cap on L binds), and both convex cases.

The bound of the comparison, per case, input family, demodulation frequency and setting: the device's largest |got - f64| / B over the
pixels compared is at most 4 x floor.  B = sum_a sum_k |v_k| per pixel; the floor is the largest |restatement in np.float32 - restatement
in float64| / B over the same pixels, the larger of the two orders of every sum; the factor 4 is the project's (D19) for the kernel's
other order of operations -- the two float32 orders of the restatement differ from each other by up to 2.1 x the smaller floor.  Every
case prints its floor and the device's ratio before it asserts; DESIGN.md D23 records them."""
import ctypes as C

import numpy as np
import pytest

import capon_util as ku
import convex_util as cu
import das_util as du
import nlbf_util as nu
from conftest import scene_path
from walk_cases import C0, T, geometry

pytestmark = pytest.mark.gpu

NAMES = ("a1_e3_small_lin_f0_sum", "a6_e3_wide_lin_f1_mean", "a5_e64_lin_f1_sum", "a6_e65_near_f1_mean", "a5_e65_small_near_f0_sum",
         "a11_e130_small_near_f0_sum", "a5_e16_convex_lin_f1_sum", "a6_e16_convex_small_near_f0_mean")
SETTINGS = ((0.5, 0.01), (0.25, 0.1), (0.0, 0.01))
F_DS = (0.0, 3.0e6)
E_INVALID = -1


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(a.shape + (2,))


def image(mi, g, data, f_d, l_prop, delta_l, form="dev", tables=False):
    """the library's image through the Python layer: form 'dev', 'table' or 'host'; tables: the scan as np.meshgrid(x, z)"""
    gx, gz = np.meshgrid(g["x"], g["z"], indexing="ij") if tables else (g["x"], g["z"])
    kw = dict(g["kw"], l_prop=l_prop, delta_l=delta_l, tables=tables)
    if form != "host":
        data = mi.DeviceBuffer.from_host(mi.default_context(), np.ascontiguousarray(data))
        if form == "table":
            kw["table"] = (mi.scan_first_arrival if tables else mi.das_first_arrival)(g["tx"], g["elem"], gx, gz, C0)
    out = mi.capon_beamform(data, g["tx"], g["elem"], gx, gz, g["fs"], C0, f_d, **kw)
    return out if form == "host" else out.numpy()


# ---- the device against the float64 restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("f_d", F_DS)
@pytest.mark.parametrize("which", ["noise", "coherent"])
@pytest.mark.parametrize("name", NAMES)
def test_device_against_the_float64_restatement(mi, name, which, f_d):
    g = geometry(name)
    data = ku.case_data(name, which)
    assert g["left_out"].mean() <= 0.02
    keep = ~g["left_out"]
    unused = (g["n_a"].sum(axis=0) == 0) & keep
    for l_prop, delta_l in SETTINGS:
        ref, B = ku.restated(name, which, f_d, l_prop, delta_l)
        used = keep & (B > 0)
        floor = ku.floor_of(name, which, f_d, l_prop, delta_l, used)
        got = image(mi, g, data, f_d, l_prop, delta_l)
        ratio = float((np.abs(got.astype(np.complex128) - ref)[used] / B[used]).max())
        print(f"\n{name} {which} f_d={f_d:g} l_prop={l_prop} delta_l={delta_l}: float32 floor {floor:.2e}, device {ratio:.2e} "
              f"({ratio / floor:.2f} x), {int(used.sum())} pixels, {int(g['left_out'].sum())} left out, N up to {int(g['n_a'].max())}")
        assert used.any() and np.all(bits(got)[unused] == 0), (name, l_prop)          # a pixel that uses no element is exactly (+0, +0)
        assert ratio <= 4.0 * floor, (name, which, f_d, l_prop, delta_l, ratio, floor)
        if which == "noise" and f_d != 0.0:
            # the first-arrival table changes no bit, nor does staging from host memory, nor the tables of the separable scan
            want = bits(got)
            assert np.array_equal(bits(image(mi, g, data, f_d, l_prop, delta_l, "table")), want), (name, l_prop, "table")
            assert np.array_equal(bits(image(mi, g, data, f_d, l_prop, delta_l, "host")), want), (name, l_prop, "host")
            assert np.array_equal(bits(image(mi, g, data, f_d, l_prop, delta_l, "dev", tables=True)), want), (name, l_prop, "tables")
            assert np.array_equal(bits(image(mi, g, data, f_d, l_prop, delta_l, "table", tables=True)), want), (name, l_prop, "table, tables")


def test_zero_aperture_tiles_are_exactly_zero(mi):
    name = "a6_e3_wide_lin_f1_mean"
    g = geometry(name)
    none = g["n_a"].sum(axis=0) == 0
    assert none[:8].all() and none[16:].all() and not none[8:16].all()       # the outer x tiles see no element, the middle one does
    for form in ("dev", "table"):
        got = image(mi, g, ku.case_data(name, "noise"), 3.0e6, 0.5, 0.01, form)
        assert np.all(bits(got)[none & ~g["left_out"]] == 0) and np.all(bits(got)[:8] == 0) and np.all(bits(got)[16:] == 0)
        assert np.any(got[8:16] != 0)


# ---- L = 1 is I/Q delay-and-sum ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_one_element_subarrays_are_iq_delay_and_sum(mi, name):
    g = geometry(name)
    data = ku.case_data(name, "noise")
    args = (g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0)
    tol_of = cu.das_tolerance if g["elem"].ndim == 2 else du.tolerance
    tol, n_terms = tol_of(np.abs(data), *args, **g["kw"])
    keep = ~g["left_out"]
    das = mi.iq_beamform(data, *args, 3.0e6, **g["kw"])
    for delta_l in (0.01, 10.0):
        one = image(mi, g, data, 3.0e6, 0.0, delta_l)
        err = np.maximum(np.abs(one.real.astype(np.float64) - das.real), np.abs(one.imag.astype(np.float64) - das.imag))
        print(f"\n{name} delta_l={delta_l}: largest error / tolerance {np.max(err[keep] / np.maximum(tol[keep], 1e-300)):.3f}")
        assert np.any(das[keep] != 0) and np.all(err[keep] <= tol[keep])
        assert np.all(bits(one)[(n_terms == 0) & keep] == 0)
    if name == "a1_e3_small_lin_f0_sum":      # N = 3: every setting is L = 1
        assert np.array_equal(bits(image(mi, g, data, 3.0e6, 0.5, 0.01)), bits(image(mi, g, data, 3.0e6, 0.0, 0.01)))


# ---- constant traces ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a5_e64_lin_f1_sum", "a6_e65_near_f1_mean", "a5_e65_small_near_f0_sum", "a11_e130_small_near_f0_sum",
                                  "a5_e16_convex_lin_f1_sum"])
def test_constant_traces_give_n_times_the_sample(mi, name):
    """traces == v without a carrier: y_a = N_a v, the image v sum_a N_a (/ A), per transmission to (N_a + 16) 2^-24 L / delta_l relative"""
    g = geometry(name)
    v = complex(np.complex64(0.75 + 0.3j))
    n_a, keep = g["n_a"], ~g["left_out"]
    A = g["A"]
    data = np.full((A, g["E"], T), v, np.complex64)
    scale = 1.0 / A if g["kw"]["compound"] == "mean" else 1.0
    want = v * n_a.sum(axis=0) * scale
    for l_prop, delta_l in SETTINGS:
        L = np.vectorize(lambda n: ku.lm(int(n), l_prop)[0])(n_a)
        bound = ((n_a + 16.0) * 2.0 ** -24 * L / delta_l * abs(v) * n_a).sum(axis=0) * scale
        got = image(mi, g, data, 0.0, l_prop, delta_l).astype(np.complex128)
        err = np.abs(got - want)
        print(f"\n{name} l_prop={l_prop} delta_l={delta_l}: largest error / bound {np.max(err[keep] / np.maximum(bound[keep], 1e-300)):.4f}")
        assert np.any(want != 0) and np.all(err[keep] <= bound[keep]), (name, l_prop, delta_l)


# ---- the scale of the data ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a5_e64_lin_f1_sum", "a5_e65_small_near_f0_sum"])
def test_a_power_of_two_on_the_data_is_a_power_of_two_on_the_image(mi, name):
    """y_a is homogeneous in the samples, and the kernel brings the v_k of a pixel to order 1 by a power of two before it squares them
    (include/pbrt_hip.h): data times 2^k give the image times 2^k bit for bit, also where the squares of the samples leave the range of
    float32 -- 2^-70 (squares near 1e-42, subnormal) and 2^70 (squares near 1e42, beyond the largest float)"""
    g = geometry(name)
    data = ku.case_data(name, "noise")
    for l_prop, delta_l in SETTINGS[:2]:
        one = image(mi, g, data, 3.0e6, l_prop, delta_l)
        for k in (-70, -20, 30, 70):
            got = image(mi, g, (data * np.float32(2.0 ** k)).astype(np.complex64), 3.0e6, l_prop, delta_l)
            assert np.isfinite(got).all() and np.array_equal(bits(got), bits(one * np.float32(2.0 ** k))), (name, l_prop, k)


# ---- non-finite samples ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "plus_inf"])
@pytest.mark.parametrize("name", ["a5_e64_lin_f1_sum", "a5_e65_small_near_f0_sum", "a5_e16_convex_lin_f1_sum"])
def test_a_bad_sample_stays_in_the_pixels_that_read_it(mi, name, value):
    g = geometry(name)
    clean = ku.case_data(name, "noise")
    where, _ = nu.bad_sites(g, T, C0, 3, 17)
    kept = ~(g["left_out"] | nu.near_bad(g, T, C0, where))
    assert 1.0 - kept.mean() <= 0.02
    data = np.array(clean, copy=True)
    flags = np.zeros(data.shape, bool)
    for a, e, t in where:
        data[a, e, t] = complex(value, float(clean[a, e, t].imag))
        flags[a, e, t] = True
    sure, maybe = nu.bad_reads(flags, g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, f_number=g["kw"]["f_number"],
                               interpolation=g["kw"]["interpolation"])
    for l_prop, delta_l in SETTINGS:
        ref = image(mi, g, clean, 3.0e6, l_prop, delta_l)
        got = image(mi, g, data, 3.0e6, l_prop, delta_l)
        assert np.isfinite(ref).all()
        hit, free = kept & sure, kept & ~sure & ~maybe
        assert hit.any() and free.any()
        assert np.all(~np.isfinite(got.real[hit]) | ~np.isfinite(got.imag[hit])), (name, value, l_prop)
        assert np.array_equal(bits(got)[free], bits(ref)[free]), (name, value, l_prop)
        assert np.array_equal(bits(image(mi, g, data, 3.0e6, l_prop, delta_l, "table")), bits(got))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def capon_block(capi, g, f_d=3.0e6, l_prop=0.5, delta_l=0.01, tables=0):
    par = capi.CaponParams()
    d, kw = par.scan.das, g["kw"]
    d.n_angles, d.n_elements, d.time_samples = g["A"], g["E"], T
    d.fs, d.sound_speed, d.t0, d.f_number = g["fs"], C0, 0.0, kw["f_number"]
    d.interpolation = {"nearest": capi.DAS_NEAREST, "linear": capi.DAS_LINEAR}[kw["interpolation"]]
    d.compound_mean = {"sum": 0, "mean": 1}[kw["compound"]]
    d.nx, d.nz = len(g["x"]), len(g["z"])
    par.scan.method, par.scan.p, par.scan.demod_freq, par.scan.probe = capi.SCAN_IQ, 2.0, f_d, int(g["elem"].ndim == 2)
    par.tables, par.l_prop, par.delta_l = tables, l_prop, delta_l
    return par


def raw_call(mi, par, g, data, form="dev", edit=None):
    """pbrt_capon_beamform[_dev | _table_dev] through ctypes on a block -> (rc, out, the context's error text); out starts as 7"""
    cx = mi.default_context()
    if edit is not None:
        edit(par)
    out = np.full((len(g["x"]), len(g["z"])), 7.0, np.complex64)
    host = [np.ascontiguousarray(a) for a in (data, g["tx"], g["elem"], g["x"], g["z"])]
    if form == "host":
        rc = cx.lib.pbrt_capon_beamform(cx.handle, C.byref(par), *(a.ctypes.data for a in host), out.ctypes.data)
    else:
        bufs = [mi.DeviceBuffer.from_host(cx, a) for a in host]
        d_out = mi.DeviceBuffer.from_host(cx, out)
        if form == "table":
            bufs[1] = mi.das_first_arrival(bufs[1], bufs[2], bufs[3], bufs[4], C0)
        name = "pbrt_capon_beamform_table_dev" if form == "table" else "pbrt_capon_beamform_dev"
        rc = getattr(cx.lib, name)(cx.handle, C.byref(par), *(b.ptr for b in bufs), d_out.ptr)
        out = d_out.numpy()
    msg = cx.lib.pbrt_last_error(cx.handle)
    return rc, out, (msg.decode() if msg else "")


def test_refusals_on_the_device_library(mi, capi):
    name = "a5_e64_lin_f1_sum"
    g, data = geometry(name), ku.case_data(name, "noise")
    rc, out, msg = raw_call(mi, capon_block(capi, g), g, data)
    assert rc == 0 and np.any(out != 7.0), msg
    assert np.array_equal(bits(out), bits(image(mi, g, data, 3.0e6, 0.5, 0.01)))
    nan, inf = float("nan"), float("inf")
    rules = [(lambda p, m=m: setattr(p.scan, "method", m), "method") for m in (capi.SCAN_DAS, capi.BF_PDAS, capi.BF_FDMAS, 4)]
    rules += [(lambda p: setattr(p, "tables", 2), "tables")]
    rules += [(lambda p, v=v: setattr(p, "l_prop", v), "l_prop") for v in (-0.25, 0.75, nan, inf)]
    rules += [(lambda p, v=v: setattr(p, "delta_l", v), "delta_l") for v in (0.0, -0.01, 2e3, nan, inf)]
    rules += [(lambda p: setattr(p.scan.das, "n_elements", 257), "n_elements <= CAPON_MAX_E"),
              (lambda p: setattr(p.scan, "probe", 2), "probe"), (lambda p: setattr(p.scan, "demod_freq", -1.0), "demod_freq"),
              (lambda p: setattr(p.scan, "demod_freq", nan), "demod_freq"), (lambda p: setattr(p.scan.das, "n_angles", 0), "n_angles"),
              (lambda p: setattr(p.scan.das, "n_elements", 0), "n_elements"), (lambda p: setattr(p.scan.das, "time_samples", 1), "time_samples"),
              (lambda p: setattr(p.scan.das, "fs", 0.0), "fs"), (lambda p: setattr(p.scan.das, "sound_speed", 0.0), "sound_speed"),
              (lambda p: setattr(p.scan.das, "interpolation", 2), "interpolation"), (lambda p: setattr(p.scan.das, "f_number", -1.0), "f_number"),
              (lambda p: setattr(p.scan.das, "nx", 0), "nx")]
    for edit, word in rules:
        for form in ("dev", "table", "host"):
            rc, out, msg = raw_call(mi, capon_block(capi, g), g, data, form, edit)
            assert rc == E_INVALID and np.all(out == 7.0), (word, form, rc)
            assert msg.startswith("invalid argument: ") and word in msg, (word, form, msg)
    for lp, dl in ((0.0, 1e3), (0.5, 1e-6), (0.25, 1.0)):
        assert raw_call(mi, capon_block(capi, g, l_prop=lp, delta_l=dl), g, data)[0] == 0
    # the Python calls say so before the library is asked
    args = (data, g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, 3.0e6)
    for kw in (dict(l_prop=0.75), dict(l_prop=-0.1), dict(l_prop=nan), dict(delta_l=0.0), dict(delta_l=2e3), dict(delta_l=None)):
        with pytest.raises(ValueError):
            mi.capon_beamform(*args, **kw)
    with pytest.raises(ValueError):
        mi.capon_beamform(np.zeros((1, 257, 8), np.complex64), np.zeros((1, 257)), np.zeros(257), g["x"], g["z"], g["fs"], C0, 3.0e6)
    # the class: always I/Q, no receive window, RF data refused as the I/Q DelayAndSum refuses them
    with pytest.raises(NotImplementedError):
        mi.Capon().set_is_iq(False)
    with pytest.raises(NotImplementedError):
        mi.Capon(is_iq=False)
    with pytest.raises(NotImplementedError):
        mi.Capon().update_setup("is_iq", False)
    probe = mi.build_probe("linear", g["E"], 1.0e-4, 3.0e6, 70)
    info = {"sampling_freq": g["fs"], "t0": 0, "delays": g["tx"], "sound_speed": C0}
    scan = mi.GridScan(g["x"], g["z"])
    with pytest.raises(ValueError, match="boxcar"):
        mi.Capon(rx_apodization="hann").automatic_setup(info, probe).beamform(data, scan)
    with pytest.raises(ValueError, match="the data are real"):
        mi.Capon().automatic_setup(info, probe).beamform(data.real.copy(), scan)
    mi.default_context().synchronize()


# ---- the point scatterer, through the library ---------------------------------------------------------------------------------------
def test_capon_narrows_the_point_scatterer_on_the_device(mi):
    def das(s, fn):
        return mi.iq_beamform(s["iq"], s["tx"], s["ex"], s["x"], s["z"], s["fs"], s["c"], s["f0"], f_number=fn)

    def capon(s, fn):
        return mi.capon_beamform(s["iq"], s["tx"], s["ex"], s["x"], s["z"], s["fs"], s["c"], s["f0"], l_prop=0.5, delta_l=0.01, f_number=fn)

    ku.assert_capon_narrows_the_scatterer(das, capon)


# ---- the classes -------------------------------------------------------------------------------------------------------------------
def test_the_class_hands_the_settings_on(mi):
    name = "a5_e64_lin_f1_sum"
    g, iq = geometry(name), ku.case_data(name, "noise")
    probe = mi.build_probe("linear", g["E"], float(g["elem"][1] - g["elem"][0]), 3.0e6, 70)
    probe.geometry[0] = g["elem"]                      # the case's own positions, bit for bit
    info = {"sampling_freq": g["fs"], "t0": 0, "delays": g["tx"], "sound_speed": C0}
    scan = mi.GridScan(g["x"], g["z"])
    su = dict(f_number=1.0, interpolation="linear", compound="sum")
    args = (g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, 3.0e6)
    bf = mi.Capon(l_prop=0.25, delta_l=0.1, **su).automatic_setup(info, probe)
    assert bf.is_iq and bf.setups["l_prop"] == 0.25 and bf.setups["delta_l"] == 0.1 and "Capon" in str(bf)
    want = mi.capon_beamform(iq, *args, l_prop=0.25, delta_l=0.1, **su)
    assert want.dtype == np.complex64 and np.array_equal(bits(bf.beamform(iq, scan)), bits(want))
    on_dev = bf.beamform(mi.DeviceBuffer.from_host(mi.default_context(), iq), scan)
    assert isinstance(on_dev, mi.DeviceBuffer) and np.array_equal(bits(on_dev.numpy()), bits(want))
    env = bf.compute_envelope(want)
    assert np.array_equal(env, mi.iq_envelope(want))
    bf.update_setup("delta_l", 0.01)
    bf.update_setup("l_prop", 0.5)
    other = bf.beamform(iq, scan)
    assert not np.array_equal(other, want) and np.array_equal(bits(other), bits(mi.capon_beamform(iq, *args, **su)))
    polar = mi.PolarScan(np.asarray(g["z"], np.float64)[0] + np.arange(16) * 0.187e-3, np.linspace(-0.3, 0.3, 9))
    px, pz = polar.pixels()
    on_polar = bf.beamform(iq, polar)
    assert on_polar.shape == polar.shape and np.isfinite(on_polar).all() and np.any(on_polar != 0)
    assert np.array_equal(bits(on_polar), bits(mi.capon_beamform(iq, g["tx"], g["elem"], px, pz, g["fs"], C0, 3.0e6, tables=True, **su)))
    from importlib import import_module
    assert import_module(mi.__name__ + ".ultraspy.beamformers.capon").Capon is mi.Capon


# ---- us_render ---------------------------------------------------------------------------------------------------------------------
def _plate_scan(ui, step, half_x, half_z):
    return dict(x_range=(-(half_x + 0.5) * step, half_x * step), z_range=(0.05 - (half_z + 0.5) * step, 0.05 + half_z * step), step=step)


def test_us_render_with_capon(mi):
    """the plate phantom (tests/scenes/us_plate.xml) with beamformer=Capon(): is_iq selects the I/Q chain by itself -- rf2iq, Capon,
    modulus, log compression -- on a 25 x 65 scan at lambda / 2.  One path per ray: the replayed chain is compared bit for bit."""
    sc = mi.load_file(scene_path("us_plate.xml"), paths_per_ray=1, seed=4)
    ui = sc.integrator()
    lam = ui.sound_speed / ui.frequency
    kw = _plate_scan(ui, lam / 2, 12, 32)
    bf = mi.Capon()
    imgs, flags = [], []
    for _ in range(3):
        tm = {}
        disp, env, (xs, zs) = mi.us_render(sc, beamformer=bf, timing=tm, **kw)
        imgs.append((disp, env))
        flags.append(tm["replayed"])
    assert len(xs) <= 64 and len(zs) <= 200 and disp.shape == (len(zs), len(xs)) and env.shape == (len(xs), len(zs))
    assert flags == [False, False, True]
    plan = ui._render_plan
    mag = np.abs(plan.d_iq.numpy())
    print(f"\nus_render Capon: |I/Q| from {mag[mag > 0].min():.3e} to {mag.max():.3e} ({int((mag == 0).sum())} of {mag.size} zero), "
          f"{int((~np.isfinite(env)).sum())} of {env.size} pixels non-finite")
    assert np.array_equal(imgs[2][0], imgs[1][0]) and np.array_equal(imgs[2][1], imgs[1][1]) and env.max() > 0 and np.isfinite(env).all()
    # the host classes on the channel buffer the device chain used: the same bits, step by step
    chan = np.asarray(ui.channel_buf, np.float32).reshape(ui.n_angles, ui.n_elements, ui.time_samples)
    delays = np.asarray(ui.transmission_delays_buf, np.float32).reshape(ui.n_angles, ui.n_elements)
    probe = mi.build_probe("linear", ui.n_elements, ui.pitch, ui.frequency, 70)
    iq = mi.rf2iq(chan, ui.frequency, ui.fs, decimation=1)
    host_bf = mi.Capon().automatic_setup({"sampling_freq": ui.fs, "t0": 0, "delays": delays, "sound_speed": ui.sound_speed}, probe)
    scan = mi.GridScan(xs, zs)
    img = host_bf.beamform(iq, scan)
    assert np.array_equal(plan.d_iq.numpy(), iq) and np.array_equal(bits(plan.d_bf_iq.numpy()), bits(img)) and np.any(img != 0)
    assert np.array_equal(host_bf.compute_envelope(img), env)
    # the image is not delay-and-sum's
    das = mi.DelayAndSum(is_iq=True).automatic_setup(host_bf.acquisition_info, probe).beamform(iq, scan)
    assert not np.array_equal(das, img)
    # a changed delta_l is a new recording and another image
    bf.update_setup("delta_l", 1.0)
    tm = {}
    _, env_loaded, _ = mi.us_render(sc, beamformer=bf, timing=tm, **kw)
    assert not tm["replayed"] and not np.array_equal(env_loaded, env)
    host_bf.update_setup("delta_l", 1.0)
    assert np.array_equal(bits(host_bf.beamform(iq, scan)), bits(ui._render_plan.d_bf_iq.numpy()))
    # on_device, and the chain through the host-pointer forms on an acquisition of its own (its channel words differ by the order of
    # their float32 atomic adds: finite, and the same shape)
    d_img, d_env, _ = mi.us_render(sc, beamformer=bf, on_device=True, **kw)
    sc.device().ctx.synchronize()
    assert np.array_equal(d_env.numpy(), env_loaded) and d_img.numpy().T.shape == disp.shape
    d_host, b_host, _ = mi.us_render(sc, beamformer=bf, device_resident=False, **kw)
    assert d_host.shape == disp.shape and np.isfinite(b_host).all() and b_host.max() > 0


def test_us_render_with_capon_convex_and_polar(mi):
    from test_gpu_convex_array import _scene
    sc = _scene(mi, paths_per_ray=4)
    ui = sc.integrator()
    step = (ui.sound_speed / ui.frequency) / 2
    R = ui.radius                       # z is measured from the centre of curvature: the plate lies at R + 20 mm
    kw = dict(x_range=(-10 * step, 10 * step), z_range=(R + 0.02 - 20 * step, R + 0.02 + 20 * step), step=step)
    disp, env, (xs, zs) = mi.us_render(sc, beamformer=mi.Capon(), **kw)
    assert np.isfinite(env).all() and env.max() > 0 and disp.shape == (len(zs), len(xs))
    sc = mi.load_file(scene_path("us_plate.xml"), paths_per_ray=1, seed=4)
    ui = sc.integrator()
    lam = ui.sound_speed / ui.frequency
    disp, env, (xs, zs) = mi.us_render(sc, beamformer=mi.Capon(), scan="polar", **_plate_scan(ui, lam / 2, 12, 32))
    assert np.isfinite(env).all() and env.max() > 0 and disp.shape == (len(zs), len(xs)) and env.shape == (len(xs), len(zs))
