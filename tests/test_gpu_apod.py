"""Receive apodisation on the device: k_apod_beamform against the float64 restatement of tests/apod_util.py for every
method, probe kind, scan kind and call form; boxcar against the calls that exist; the refusals; the classes and us_render.

The shapes are the five f-number cases of walk_cases.CASES, for the reasons that file states (a6_e3_wide_lin_f1_mean is the one whose
outer tiles see no element); the f-number-0 cases serve boxcar and the refusals.

The bound of the comparison, per case, window, method and input family: |device - f64| / B <= 4 x floor + 4 * 2^-24.  B is the
per-pixel sum of the UNWEIGHTED magnitudes (apod_util.beamform), the floor the largest |restatement in np.float32 - restatement in
float64| / B over the pixels compared, the factor 4 the project's for the kernel's other summation order and ocml's powf (D19, D20),
and 4 * 2^-24 the bound of a weight (include/pbrt_hip.h): the device's cospif and the restatement's cosine may differ by that much on
every sample of a pixel.  Every case prints its floor and the device's ratio before it asserts; DESIGN.md D22 records them."""
import ctypes as C

import numpy as np
import pytest

import apod_util as au
import nlbf_util as nu
from conftest import scene_path
from walk_cases import C0, CASES, T, geometry

pytestmark = pytest.mark.gpu

F_CASES = ("a5_e64_lin_f1_sum", "a6_e65_near_f1_mean", "a6_e3_wide_lin_f1_mean", "a5_e16_convex_lin_f1_sum", "a11_e130_small_lin_f1_mean")
WINDOWS = (("hann", 0.5), ("hamming", 0.5), ("tukey", 0.25))
RF_METHODS = (("das", 2.0), ("pdas", 2.0), ("pdas", 3.0), ("fdmas", 2.0))
ALL_METHODS = RF_METHODS + (("iq", 2.0),)
F_D = 3.0e6
E_INVALID = -1


def family(name, which):
    """test_gpu_nlbf.py's two RF families -- (i) every trace of one sign, |v| in [0.25, 1]; (ii) zero-mean RF -- and complex normal I/Q"""
    g = geometry(name)
    rng = np.random.default_rng(sum(map(ord, name)) * 7 + len(which))
    shape = (g["A"], g["E"], T)
    if which == "one_sign":
        sign = rng.choice([-1.0, 1.0], size=(g["A"], g["E"], 1))
        return (sign * rng.uniform(0.25, 1.0, shape)).astype(np.float32)
    if which == "iq":
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    return rng.standard_normal(shape).astype(np.float32)


def image(mi, g, data, method, p, window="boxcar", alpha=0.5, form="dev", tables=False):
    """the library's image through the Python layer: form 'dev', 'table' or 'host'; tables: the scan as np.meshgrid(x, z)"""
    kw = dict(g["kw"], rx_apodization=window, rx_apodization_alpha=alpha)
    gx, gz = np.meshgrid(g["x"], g["z"], indexing="ij") if tables else (g["x"], g["z"])
    if form != "host":
        cx = mi.default_context()
        data = mi.DeviceBuffer.from_host(cx, data)
        if form == "table":
            first = mi.scan_first_arrival if tables else mi.das_first_arrival
            kw["table"] = first(g["tx"], g["elem"], gx, gz, C0)
    args = (data, g["tx"], g["elem"], gx, gz, g["fs"], C0)
    if tables:
        out = mi.scan_beamform(*args, method=method, p=p, demod_freq=F_D if method == "iq" else None, **kw)
    elif method == "das":
        out = mi.das_beamform(*args, **kw)
    elif method == "iq":
        out = mi.iq_beamform(*args, F_D, **kw)
    else:
        out = mi.nonlinear_beamform(*args, method=method, p=p, **kw)
    return out if form == "host" else out.numpy()


def apod_block(capi, g, method, p, window, alpha, tables=0):
    par = capi.ApodParams()
    d, kw = par.scan.das, g["kw"]
    d.n_angles, d.n_elements, d.time_samples = g["A"], g["E"], T
    d.fs, d.sound_speed, d.t0, d.f_number = g["fs"], C0, 0.0, kw["f_number"]
    d.interpolation = {"nearest": capi.DAS_NEAREST, "linear": capi.DAS_LINEAR}[kw["interpolation"]]
    d.compound_mean = {"sum": 0, "mean": 1}[kw["compound"]]
    d.nx, d.nz = len(g["x"]), len(g["z"])
    par.scan.method = {"das": capi.SCAN_DAS, "pdas": capi.BF_PDAS, "fdmas": capi.BF_FDMAS, "iq": capi.SCAN_IQ}[method]
    par.scan.p, par.scan.demod_freq, par.scan.probe = p, F_D, int(g["elem"].ndim == 2)
    par.tables, par.window, par.alpha = tables, window, alpha
    return par


def raw_call(mi, par, g, data, form="dev", edit=None):
    """pbrt_apod_beamform[_dev | _table_dev] through ctypes on a block -> (rc, out, the context's error text); out starts as 7"""
    cx = mi.default_context()
    if edit is not None:
        edit(par)
    dtype = data.dtype
    out = np.full((len(g["x"]), len(g["z"])), 7.0, dtype)
    gx, gz = (np.meshgrid(g["x"], g["z"], indexing="ij") if par.tables == 1 else (g["x"], g["z"]))
    host = [np.ascontiguousarray(a) for a in (data, g["tx"], g["elem"], gx.astype(np.float32), gz.astype(np.float32))]
    if form == "host":
        rc = cx.lib.pbrt_apod_beamform(cx.handle, C.byref(par), *(a.ctypes.data for a in host), out.ctypes.data)
    else:
        bufs = [mi.DeviceBuffer.from_host(cx, a) for a in host]
        d_out = mi.DeviceBuffer.from_host(cx, out)
        if form == "table":
            first = mi.scan_first_arrival if par.tables == 1 else mi.das_first_arrival
            bufs[1] = first(bufs[1], bufs[2], bufs[3], bufs[4], C0)
        name = "pbrt_apod_beamform_table_dev" if form == "table" else "pbrt_apod_beamform_dev"
        rc = getattr(cx.lib, name)(cx.handle, C.byref(par), *(b.ptr for b in bufs), d_out.ptr)
        out = d_out.numpy()
    msg = cx.lib.pbrt_last_error(cx.handle)
    return rc, out, (msg.decode() if msg else "")


def restated(g, data, method, p, window, alpha, dtype=np.float64):
    return au.beamform(method, data, g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, window, alpha, p=p, f_d=F_D, dtype=dtype, **g["kw"])


# ---- 6. the device against the float64 restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["one_sign", "zero_mean", "iq"])
@pytest.mark.parametrize("name", F_CASES)
def test_device_against_the_float64_restatement(mi, name, which):
    g = geometry(name)
    data = family(name, which)
    assert g["left_out"].mean() <= 0.02
    keep = ~g["left_out"]
    unused = (g["n_a"].sum(axis=0) == 0) & keep
    for window, alpha in WINDOWS:
        for method, p in ((("iq", 2.0),) if which == "iq" else RF_METHODS):
            ref, B = restated(g, data, method, p, window, alpha)
            f32, _ = restated(g, data, method, p, window, alpha, np.float32)
            got = image(mi, g, data, method, p, window, alpha)
            used = keep & (B > 0)
            floor = float((np.abs(f32.astype(ref.dtype) - ref)[used] / B[used]).max())
            ratio = float((np.abs(got.astype(ref.dtype) - ref)[used] / B[used]).max())
            print(f"\n{name} {which} {window} {method} p={p}: float32 floor {floor / 2 ** -24:.2f} x 2^-24, device {ratio / 2 ** -24:.2f} x 2^-24, "
                  f"{int(used.sum())} pixels, {int(g['left_out'].sum())} left out")
            assert np.all(got[unused] == 0.0), (name, window, method)              # a pixel that uses no element is exactly 0
            assert ratio <= 4.0 * floor + au.WEIGHT_BOUND, (name, which, window, method, p, ratio, floor)
            if which != "zero_mean":
                # the first-arrival table changes no bit, nor does staging from host memory, nor the tables of the separable scan
                assert np.array_equal(image(mi, g, data, method, p, window, alpha, "table"), got), (name, window, method, p)
                assert np.array_equal(image(mi, g, data, method, p, window, alpha, "host"), got), (name, window, method, p)
                assert np.array_equal(image(mi, g, data, method, p, window, alpha, "dev", tables=True), got), (name, window, method, p)
                assert np.array_equal(image(mi, g, data, method, p, window, alpha, "table", tables=True), got), (name, window, method, p)


# ---- 7. boxcar is today's ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_boxcar_is_the_existing_call_bit_for_bit(mi, capi, name):
    g = geometry(name)
    for method, p in ALL_METHODS:
        data = family(name, "iq" if method == "iq" else "zero_mean")
        args = (mi.DeviceBuffer.from_host(mi.default_context(), data), g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0)
        if method == "das":
            today = mi.das_beamform(*args, **g["kw"]).numpy()
        elif method == "iq":
            today = mi.iq_beamform(*args, F_D, **g["kw"]).numpy()
        else:
            today = mi.nonlinear_beamform(*args, method=method, p=p, **g["kw"]).numpy()
        assert np.any(today != 0)
        assert np.array_equal(image(mi, g, data, method, p, "boxcar", 0.5), today), (name, method, p)
        assert np.array_equal(image(mi, g, data, method, p, "boxcar", 7.0, "host"), today), (name, method, p)   # (alpha: Tukey's only)
        for form in ("dev", "table", "host"):
            for tables in (0, 1):
                rc, out, msg = raw_call(mi, apod_block(capi, g, method, p, capi.PBRT_APOD_BOXCAR, -1.0, tables), g, data, form)
                assert rc == 0, msg
                assert np.array_equal(out, today), (name, method, p, form, tables)


# ---- 8. Tukey(1) against Hann ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a5_e64_lin_f1_sum", "a5_e16_convex_lin_f1_sum"])
def test_tukey_1_is_hann_and_the_windows_differ(mi, name):
    g = geometry(name)
    for method, p in ALL_METHODS:
        data = family(name, "iq" if method == "iq" else "zero_mean")
        hann = image(mi, g, data, method, p, "hann", 0.3)
        assert np.array_equal(image(mi, g, data, method, p, "tukey", 1.0), hann), (name, method)
        tukey, boxcar = image(mi, g, data, method, p, "tukey", 0.25), image(mi, g, data, method, p)
        hamming = image(mi, g, data, method, p, "hamming")
        for a, b in ((hann, boxcar), (tukey, boxcar), (tukey, hann), (hamming, hann), (hamming, boxcar)):
            assert not np.array_equal(a, b), (name, method)


# ---- 9. constant traces ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [0.75, -0.75])
@pytest.mark.parametrize("name", ["a5_e64_lin_f1_sum", "a5_e16_convex_lin_f1_sum"])
def test_constant_traces_give_the_sum_of_the_weights(mi, name, v):
    """traces == v: delay-and-sum gives v sum_a sum_{e in U(a)} w_e, to (max_a N_a + 20) 2^-24 |v| sum_a N_a"""
    g = geometry(name)
    assert g["kw"]["compound"] == "sum"
    n_a, keep = g["n_a"], ~g["left_out"]
    data = np.full((g["A"], g["E"], T), v, np.float32)
    used = [ok for _, ok in nu.delayed(data, g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, f_number=g["kw"]["f_number"],
                                       interpolation=g["kw"]["interpolation"])]
    assert np.array_equal(np.stack([u.sum(axis=0) for u in used]), n_a)
    bound = (n_a.max(axis=0) + 20.0) * 2.0 ** -24 * abs(v) * n_a.sum(axis=0)
    for window, alpha in WINDOWS:
        w, _ = au.weights(g["elem"], g["x"], g["z"], g["kw"]["f_number"], window, alpha)
        want = v * sum((u * w).sum(axis=0) for u in used)
        got = image(mi, g, data, "das", 2.0, window, alpha).astype(np.float64)
        err = np.abs(got - want)[keep]
        print(f"\n{name} v={v} {window}: largest error / bound {np.max(err / np.maximum(bound[keep], 1e-300)):.3f}")
        assert np.all(err <= bound[keep]) and np.any(want != 0), (name, window)


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device_library(mi, capi):
    name = "a5_e64_lin_f1_sum"
    g, data = geometry(name), family(name, "zero_mean")

    def base():
        return apod_block(capi, g, "das", 2.0, capi.PBRT_APOD_HANN, 0.5)

    rc, out, msg = raw_call(mi, base(), g, data)
    assert rc == 0 and np.any(out != 7.0), msg

    def tukey(alpha):
        def edit(p):
            p.window, p.alpha = capi.PBRT_APOD_TUKEY, alpha
        return edit

    rules = [(lambda p: setattr(p, "window", 4), "window"), (lambda p: setattr(p, "window", 0xFFFFFFFF), "window"),
             (lambda p: setattr(p.scan.das, "f_number", 0.0), "f_number"), (lambda p: setattr(p, "tables", 2), "tables"),
             (lambda p: setattr(p.scan, "method", 4), "method"), (lambda p: setattr(p.scan, "probe", 2), "probe"),
             (lambda p: (setattr(p.scan, "method", capi.BF_PDAS), setattr(p.scan, "p", 0.5)), "p >= 1.0f"),
             (lambda p: (setattr(p.scan, "method", capi.BF_PDAS), setattr(p.scan, "p", float("nan"))), "isfinite(p)"),
             (lambda p: (setattr(p.scan, "method", capi.SCAN_IQ), setattr(p.scan, "demod_freq", -1.0)), "demod_freq"),
             (lambda p: setattr(p.scan.das, "n_angles", 0), "n_angles"), (lambda p: setattr(p.scan.das, "time_samples", 1), "time_samples"),
             (lambda p: setattr(p.scan.das, "fs", 0.0), "fs"), (lambda p: setattr(p.scan.das, "interpolation", 2), "interpolation"),
             (lambda p: setattr(p.scan.das, "nx", 0), "nx")]
    rules += [(tukey(a), "alpha") for a in (0.0, -0.5, 1.5, float("nan"), float("inf"))]
    for edit, word in rules:
        for form in ("dev", "table", "host"):
            rc, out, msg = raw_call(mi, base(), g, data, form, edit)
            assert rc == E_INVALID and np.all(out == 7.0), (word, form, rc)
            assert msg.startswith("invalid argument: ") and word in msg, (word, form, msg)
    for alpha in (1.0, 0.5, 1e-3):
        assert raw_call(mi, base(), g, data, "dev", tukey(alpha))[0] == 0
    # a window on a scan without an f-number: refused; boxcar on it: taken
    g0 = geometry("a1_e3_small_lin_f0_sum")
    d0 = family("a1_e3_small_lin_f0_sum", "zero_mean")
    rc, out, msg = raw_call(mi, apod_block(capi, g0, "das", 2.0, capi.PBRT_APOD_HAMMING, 0.5), g0, d0)
    assert rc == E_INVALID and np.all(out == 7.0) and "f_number" in msg
    assert raw_call(mi, apod_block(capi, g0, "das", 2.0, capi.PBRT_APOD_BOXCAR, 0.5), g0, d0)[0] == 0
    # the Python calls say so before the library is asked
    dev = mi.DeviceBuffer.from_host(mi.default_context(), data)
    args = (dev, g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0)
    for kw in (dict(rx_apodization="kaiser"), dict(rx_apodization="tukey", rx_apodization_alpha=0.0),
               dict(rx_apodization="tukey", rx_apodization_alpha=1.5), dict(rx_apodization="hann", f_number=0.0),
               dict(rx_apodization="hamming", f_number=None)):
        with pytest.raises(ValueError):
            mi.das_beamform(*args, **kw)
        with pytest.raises(ValueError):
            mi.nonlinear_beamform(*args, **kw)
    mi.default_context().synchronize()


# ---- 11. the zero-aperture tiles -------------------------------------------------------------------------------------------------------
def test_zero_aperture_tiles_are_exactly_zero(mi):
    name = "a6_e3_wide_lin_f1_mean"
    g = geometry(name)
    none = g["n_a"].sum(axis=0) == 0
    assert none[:8].all() and none[16:].all() and not none[8:16].all()       # the outer x tiles see no element, the middle one does
    for window, alpha in WINDOWS:
        for method, p in ALL_METHODS:
            data = family(name, "iq" if method == "iq" else "zero_mean")
            for form in ("dev", "table"):
                got = image(mi, g, data, method, p, window, alpha, form)
                parts = (got.real, got.imag) if method == "iq" else (got,)
                for part in parts:
                    assert np.all(part[none & ~g["left_out"]] == 0.0) and not np.signbit(part[:8]).any() and not np.signbit(part[16:]).any()
                assert np.any(got[8:16] != 0.0)


# ---- 12. the classes -------------------------------------------------------------------------------------------------------------------
def test_the_classes_hand_the_window_on(mi):
    name = "a5_e64_lin_f1_sum"
    g = geometry(name)
    data, iq = family(name, "zero_mean"), family(name, "iq")
    pitch = float(g["elem"][1] - g["elem"][0])
    probe = mi.build_probe("linear", g["E"], pitch, F_D, 70)
    probe.geometry[0] = g["elem"]                      # the case's own positions, bit for bit
    info = {"sampling_freq": g["fs"], "t0": 0, "delays": g["tx"], "sound_speed": C0}
    scan = mi.GridScan(g["x"], g["z"])
    su = dict(f_number=1.0, interpolation="linear", compound="sum")
    kw = dict(rx_apodization="hann", **su)
    args = (g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0)
    bf = mi.DelayAndSum(**kw).automatic_setup(info, probe)
    hann = mi.das_beamform(data, *args, **kw)
    assert np.array_equal(bf.beamform(data, scan), hann)
    on_dev = bf.beamform(mi.DeviceBuffer.from_host(mi.default_context(), data), scan)
    assert isinstance(on_dev, mi.DeviceBuffer) and np.array_equal(on_dev.numpy(), hann)
    biq = mi.DelayAndSum(is_iq=True, **kw).automatic_setup(info, probe)
    assert np.array_equal(biq.beamform(iq, scan), mi.iq_beamform(iq, *args, F_D, **kw))
    pd = mi.PDelayAndSum(p=3.0, band=None, **kw).automatic_setup(info, probe)
    assert np.array_equal(pd.beamform(data, scan), mi.nonlinear_beamform(data, *args, method="pdas", p=3.0, **kw))
    fd = mi.FilteredDelayMultiplyAndSum(band=None, **kw).automatic_setup(info, probe)
    assert np.array_equal(fd.beamform(data, scan), mi.nonlinear_beamform(data, *args, method="fdmas", **kw))
    polar = mi.PolarScan(np.asarray(g["z"], np.float64)[0] + np.arange(16) * 0.187e-3, np.linspace(-0.3, 0.3, 9))
    px, pz = polar.pixels()
    assert np.array_equal(bf.beamform(data, polar), mi.scan_beamform(data, g["tx"], g["elem"], px, pz, g["fs"], C0, method="das", **kw))
    # update_setup then changes the image
    bf.update_setup("rx_apodization", "tukey")
    bf.update_setup("rx_apodization_alpha", 0.25)
    tukey = bf.beamform(data, scan)
    assert not np.array_equal(tukey, hann)
    assert np.array_equal(tukey, mi.das_beamform(data, *args, rx_apodization="tukey", rx_apodization_alpha=0.25, **su))
    bf.update_setup("rx_apodization", "boxcar")
    assert np.array_equal(bf.beamform(data, scan), mi.das_beamform(data, *args, **su))
    bf.update_setup("rx_apodization", "kaiser")
    with pytest.raises(ValueError):
        bf.beamform(data, scan)


# ---- 13. us_render ---------------------------------------------------------------------------------------------------------------------
def test_us_render_with_a_window(mi):
    """test_gpu_nlbf.py's end-to-end scene and sizes (the plate phantom, a 64 x 200 scan at lambda / 16, one path per ray: the replayed
    chain is compared bit for bit with the call before it) with beamformer=DelayAndSum(rx_apodization="hann")"""
    sc = mi.load_file(scene_path("us_plate.xml"), paths_per_ray=1, seed=4)
    ui = sc.integrator()
    step = (ui.sound_speed / ui.frequency) / 16
    kw = dict(x_range=(-31.5 * step, 31.0 * step), z_range=(0.05 - 99.5 * step, 0.05 + 99.0 * step), step=step)
    bf = mi.DelayAndSum(rx_apodization="hann")
    imgs, flags = [], []
    for _ in range(3):
        tm = {}
        disp, env, (xs, zs) = mi.us_render(sc, beamformer=bf, timing=tm, **kw)
        imgs.append((disp, env))
        flags.append(tm["replayed"])
    assert len(xs) <= 64 and len(zs) <= 200 and disp.shape == (len(zs), len(xs)) and env.shape == (len(xs), len(zs))
    assert flags == [False, False, True]
    assert all(np.array_equal(imgs[k][0], imgs[0][0]) and np.array_equal(imgs[k][1], imgs[0][1]) for k in (1, 2)) and env.max() > 0
    rf_dev = ui._render_plan.d_bf.numpy()
    # the host chain's beamformer on the channel buffer the device chain used: the same bits
    chan = np.asarray(ui.channel_buf, np.float32).reshape(ui.n_angles, ui.n_elements, ui.time_samples)
    delays = np.asarray(ui.transmission_delays_buf, np.float32).reshape(ui.n_angles, ui.n_elements)
    probe = mi.build_probe("linear", ui.n_elements, ui.pitch, ui.frequency, 70)
    info = {"sampling_freq": ui.fs, "t0": 0, "delays": delays, "sound_speed": ui.sound_speed}
    host_bf = mi.DelayAndSum(rx_apodization="hann").automatic_setup(info, probe)
    scan = mi.GridScan(xs, zs)
    assert np.array_equal(host_bf.beamform(chan, scan), rf_dev) and np.any(rf_dev != 0)
    assert np.array_equal(host_bf.compute_envelope(rf_dev), env)
    # another window is another recording: the fourth call is queued the plain way and gives another image
    bf.update_setup("rx_apodization", "hamming")
    tm = {}
    _, env_hamming, _ = mi.us_render(sc, beamformer=bf, timing=tm, **kw)
    assert not tm["replayed"] and not np.array_equal(env_hamming, env)
    host_bf.update_setup("rx_apodization", "hamming")
    assert np.array_equal(host_bf.beamform(chan, scan), ui._render_plan.d_bf.numpy())
    # the boxcar image of the same seed differs from both
    tm = {}
    _, env_boxcar, _ = mi.us_render(sc, beamformer=mi.DelayAndSum(), timing=tm, **kw)
    assert not tm["replayed"] and not np.array_equal(env_boxcar, env) and not np.array_equal(env_boxcar, env_hamming)


# ---- 14. the physics on the device -----------------------------------------------------------------------------------------------------
def test_the_windows_trade_width_for_side_lobes_on_the_device(mi):
    from test_apod_restatement import assert_the_windows_trade_width_for_side_lobes, scatterer_figures

    def beamform(s, name, alpha):
        return mi.das_beamform(s["data"], s["tx"], s["ex"], s["x"], s["z"], s["fs"], s["c"], f_number=1.0, interpolation="linear",
                               rx_apodization=name, rx_apodization_alpha=alpha)
    assert_the_windows_trade_width_for_side_lobes(scatterer_figures(beamform))
