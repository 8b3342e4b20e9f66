"""p-DAS and F-DMAS on the device: k_nl_beamform against the float64 restatement of tests/nlbf_util.py, the axial FIR
against np.convolve, the refusals, and us_render end to end with the new beamformer classes.

The shapes are the smallest at which the kernel can still go wrong: 1 / 5 / 6 / 11 transmissions (a second trip of five angles with one
angle in it, a third one), 3 / 64 / 65 / 130 elements (fewer elements than the four waves of a workgroup; a second block of 64 with one
element in it, a third with two), scans of 9 x 13, 9 x 17 and 24 x 16 pixels (partial 8 x 8 tiles), traces of 160 samples.

The tolerance of the comparison is not a constant: per case, method and input family it is FOUR TIMES the float32 floor -- the
largest |restatement in np.float32 - restatement in float64| / B over the pixels compared, B the size of what the pixel adds up
(nlbf_util.beamform).  The factor covers the kernel's other summation order and ocml's powf against NumPy's.  Every case prints its
floor and the device's largest ratio before it asserts; DESIGN.md D19 records them."""
import ctypes as C

import numpy as np
import pytest

import convex_util as cu
import das_util as du
import nlbf_util as nu
from conftest import scene_path
from walk_cases import C0, CASES, FS, T, geometry

pytestmark = pytest.mark.gpu

METHODS = (("pdas", 1.0), ("pdas", 1.5), ("pdas", 2.0), ("pdas", 3.0), ("fdmas", 2.0))


def family(name, which):
    """(i) every trace of one sign and bounded away from zero, |v| in [0.25, 1], the sign varies between traces; (ii) zero-mean RF"""
    g = geometry(name)
    rng = np.random.default_rng(sum(map(ord, name)) * 7 + len(which))
    if which == "one_sign":
        sign = rng.choice([-1.0, 1.0], size=(g["A"], g["E"], 1))
        return (sign * rng.uniform(0.25, 1.0, (g["A"], g["E"], T))).astype(np.float32)
    return rng.standard_normal((g["A"], g["E"], T)).astype(np.float32)


def device_image(mi, g, data, method, p, form="dev"):
    """the library's image: form 'dev' (pbrt_bf_beamform_dev), 'table' (_table_dev) or 'host' (pbrt_bf_beamform)"""
    args = (g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0)
    if form == "host":
        return mi.nonlinear_beamform(data, *args, method=method, p=p, **g["kw"])
    cx = mi.default_context()
    d = mi.DeviceBuffer.from_host(cx, data)
    table = mi.das_first_arrival(g["tx"], g["elem"], g["x"], g["z"], C0) if form == "table" else None
    return mi.nonlinear_beamform(d, *args, method=method, p=p, table=table, **g["kw"]).numpy()


def test_the_grids_leave_out_at_most_two_per_cent():
    for name in CASES:
        g = geometry(name)
        assert g["left_out"].mean() <= 0.02, (name, g["left_out"].mean())
        assert g["n_a"].max() >= min(g["E"], 3), name


@pytest.mark.parametrize("which", ["one_sign", "zero_mean"])
@pytest.mark.parametrize("name", list(CASES))
def test_device_against_the_float64_restatement(mi, name, which):
    g = geometry(name)
    data = family(name, which)
    keep = ~g["left_out"]
    unused = (g["n_a"].sum(axis=0) == 0) & keep
    args = (data, g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0)
    for method, p in METHODS:
        ref, B = nu.beamform(method, *args, p=p, **g["kw"])
        f32, _ = nu.beamform(method, *args, p=p, dtype=np.float32, **g["kw"])
        got = device_image(mi, g, data, method, p)
        used = keep & (B > 0)
        floor = float((np.abs(f32.astype(np.float64) - ref)[used] / B[used]).max())
        ratio = float((np.abs(got.astype(np.float64) - ref)[used] / B[used]).max())
        print(f"\n{name} {which} {method} p={p}: float32 floor {floor:.3e}, device {ratio:.3e} ({ratio / floor:.2f} x), "
              f"{int(used.sum())} pixels, {int(g['left_out'].sum())} left out")
        assert np.all(got[unused] == 0.0), (name, method)           # a pixel that uses no element is exactly 0
        assert ratio <= 4.0 * floor, (name, which, method, p, ratio, floor)
        if which == "one_sign":
            # the first-arrival table changes no bit, nor does staging the arguments from host memory
            assert np.array_equal(device_image(mi, g, data, method, p, "table"), got), (name, method, p)
            assert np.array_equal(device_image(mi, g, data, method, p, "host"), got), (name, method, p)


def test_zero_aperture_tiles_are_exactly_zero(mi):
    g = geometry("a6_e3_wide_lin_f1_mean")
    none = g["n_a"].sum(axis=0) == 0
    assert none[:8].all() and none[16:].all() and not none[8:16].all()       # the outer x tiles see no element, the middle one does
    data = family("a6_e3_wide_lin_f1_mean", "zero_mean")
    for method, p in METHODS:
        for form in ("dev", "table"):
            got = device_image(mi, g, data, method, p, form)
            assert np.all(got[none & ~g["left_out"]] == 0.0) and not np.signbit(got[:8]).any() and np.any(got[8:16] != 0.0)


@pytest.mark.parametrize("v", [0.75, -0.75])
@pytest.mark.parametrize("name", ["a5_e64_lin_f1_sum", "a6_e65_near_f1_mean", "a1_e3_small_lin_f0_sum", "a5_e16_convex_lin_f1_sum"])
def test_constant_traces_give_the_closed_forms(mi, name, v):
    """traces == v: p-DAS gives sgn(v) |v| sum_a N_a^p, F-DMAS |v| sum_a N_a (N_a - 1) / 2 for either sign, to (N_a + 16) 2^-24 relative"""
    g = geometry(name)
    n_a, keep = g["n_a"], ~g["left_out"]
    data = np.full((g["A"], g["E"], T), v, np.float32)
    scale = 1.0 / g["A"] if g["kw"]["compound"] == "mean" else 1.0
    rel = (n_a.max(axis=0) + 16.0) * du.U32
    for method, p in METHODS:
        got = device_image(mi, g, data, method, p).astype(np.float64)
        if method == "fdmas":
            want = abs(v) * (n_a * (n_a - 1) / 2).sum(axis=0) * scale
        else:
            want = np.sign(v) * abs(v) * (n_a ** p).sum(axis=0) * scale
        err = np.abs(got - want)[keep]
        print(f"\n{name} v={v} {method} p={p}: largest error / (tolerance) {np.max(err / np.maximum((rel * np.abs(want))[keep], 1e-300)):.3f}")
        assert np.all(err <= (rel * np.abs(want))[keep]), (name, method, p)


@pytest.mark.parametrize("name", ["a5_e64_lin_f1_sum", "a6_e65_near_f1_mean", "a6_e16_convex_small_near_f0_mean"])
def test_p_1_is_delay_and_sum(mi, name):
    g = geometry(name)
    data = family(name, "zero_mean")
    args = (g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0)
    cx = mi.default_context()
    das = mi.das_beamform(mi.DeviceBuffer.from_host(cx, data), *args, **g["kw"]).numpy()
    got = device_image(mi, g, data, "pdas", 1.0)
    tol_of = cu.das_tolerance if g["elem"].ndim == 2 else du.tolerance
    tol, n_terms = tol_of(data, *args, **g["kw"])
    keep = ~g["left_out"]
    assert np.any(das[keep] != 0)
    assert np.all(np.abs(got.astype(np.float64) - das)[keep] <= tol[keep])
    assert np.all(got[(n_terms == 0) & keep] == 0.0)


@pytest.mark.parametrize("nx,nz,K", [(3, 5, 8), (7, 300, 40), (2, 257, 1024)])
def test_axial_fir(mi, nx, nz, K):
    rng = np.random.default_rng(nx * 1000 + nz + K)
    x = rng.standard_normal((nx, nz)).astype(np.float32)
    h = (rng.standard_normal(2 * K + 1) / np.sqrt(2 * K + 1)).astype(np.float32)
    got = mi.axial_fir(x, h)
    assert got.shape == (nx, nz) and got.dtype == np.float32
    ref = nu.fir(x, h)
    if nz >= 2 * K + 1:        # np.convolve's 'same' keeps the longer operand's length: the column's, where the column is the longer
        assert np.array_equal(ref, np.stack([np.convolve(r.astype(np.float64), h.astype(np.float64), "same") for r in x]))
    bound = (2 * K + 17) * du.U32 * nu.fir(np.abs(x), np.abs(h))
    assert np.all(np.abs(got - ref) <= bound)
    cx = mi.default_context()
    dev = mi.axial_fir(mi.DeviceBuffer.from_host(cx, x), h).numpy()
    assert np.array_equal(dev, got)
    # an impulse returns the taps bit for bit
    imp = np.zeros((nx, nz), np.float32)
    m = nz // 2
    imp[nx - 1, m] = 1.0
    out = mi.axial_fir(imp, h)
    n = np.arange(nz)
    inside = np.abs(n - m) <= K
    assert np.array_equal(out[nx - 1][inside], h[K + (n - m)[inside]]) and np.all(out[nx - 1][~inside] == 0) and np.all(out[:nx - 1] == 0)


def _bf_call(mi, capi, method, p, probe=0):
    g = geometry("a1_e3_small_lin_f0_sum")
    cx = mi.default_context()
    bufs = [mi.DeviceBuffer.from_host(cx, a) for a in (family("a1_e3_small_lin_f0_sum", "one_sign"), g["tx"], g["elem"], g["x"], g["z"])]
    out = mi.DeviceBuffer(cx, (len(g["x"]), len(g["z"])))
    bp = capi.BfParams()
    d = bp.das
    d.n_angles, d.n_elements, d.time_samples, d.fs, d.sound_speed, d.interpolation = g["A"], g["E"], T, FS, C0, capi.DAS_LINEAR
    d.nx, d.nz = len(g["x"]), len(g["z"])
    bp.method, bp.p, bp.probe = method, p, probe
    return cx.lib.pbrt_bf_beamform_dev(cx.handle, C.byref(bp), *(b.ptr for b in bufs), out.ptr)


def test_refusals(mi, capi):
    E_INVALID = -1
    assert _bf_call(mi, capi, capi.BF_PDAS, 2.0) == 0 and _bf_call(mi, capi, capi.BF_FDMAS, 2.0) == 0
    assert _bf_call(mi, capi, capi.BF_PDAS, 1.0) == 0 and _bf_call(mi, capi, capi.BF_PDAS, 8.0) == 0
    for p in (0.5, 9.0, float("nan"), float("inf")):
        assert _bf_call(mi, capi, capi.BF_PDAS, p) == E_INVALID, p
    for method in (0, 3):
        assert _bf_call(mi, capi, method, 2.0) == E_INVALID, method
    assert _bf_call(mi, capi, capi.BF_PDAS, 2.0, probe=2) == E_INVALID
    mi.default_context().synchronize()
    x = np.ones((2, 40), np.float32)
    with pytest.raises(RuntimeError, match="rc=-1"):
        mi.axial_fir(x, np.ones(2 * 1025 + 1, np.float32))                      # K = 1025
    cx = mi.default_context()
    one = np.ones(3, np.float32)
    assert cx.lib.pbrt_axial_fir(cx.handle, 2, 0, 1, one.ctypes.data, x.ctypes.data, np.empty_like(x).ctypes.data) == E_INVALID   # nz = 0
    with pytest.raises(RuntimeError, match="rc=-1"):
        mi.nonlinear_beamform(np.ones((1, 3, T), np.float32), np.zeros((1, 3)), np.zeros(3), [0.0], [1e-3], FS, C0, method="pdas", p=0.5)


def test_the_default_band_is_refused_on_the_lambda_4_grid(mi):
    """the reference's grid (step = lambda / 4) puts the axial Nyquist frequency at the carrier: us_render says so before it acquires
    anything, and names the step that would fit"""
    sc = mi.load_file(scene_path("us_plate.xml"), paths_per_ray=1, seed=1)
    for bf in (mi.PDelayAndSum(), mi.FilteredDelayMultiplyAndSum()):
        for resident in (True, False):
            with pytest.raises(ValueError, match=r"step below .* m would fit"):
                mi.us_render(sc, beamformer=bf, device_resident=resident, x_range=(-0.001, 0.001), z_range=(0.049, 0.051))


def test_the_non_linear_beamformers_narrow_a_point_scatterer_on_the_device(mi):
    """the inequality of test_nlbf_restatement.py through the library: classes, kernels and the FIR"""
    from test_nlbf_restatement import scatterer_widths
    bfm = mi.beamform

    def beamform(method, d):
        if method == "das":
            return mi.das_beamform(d["data"], d["tx"], d["ex"], d["x"], d["z"], d["fs"], d["c"], f_number=0.0)
        return mi.nonlinear_beamform(d["data"], d["tx"], d["ex"], d["x"], d["z"], d["fs"], d["c"], method=method, p=2.0, f_number=0.0)

    w = scatterer_widths(beamform, mi.axial_fir, bfm)
    print(w)
    assert np.isfinite(w["das"]) and w["pdas"] < w["das"] and w["fdmas"] < w["das"]
    # the classes give the free functions' images (host arrays in, a host array out), the band set explicitly
    d = nu.point_scatterer()
    probe = mi.build_probe("linear", len(d["ex"]), float(d["ex"][1] - d["ex"][0]), d["f0"], 70)
    scan = mi.GridScan(d["x"], d["z"])
    info = {"sampling_freq": d["fs"], "t0": 0, "delays": d["tx"], "sound_speed": d["c"]}
    bf = mi.FilteredDelayMultiplyAndSum(f_number=0.0).automatic_setup(info, probe)
    assert np.allclose(probe.geometry[0], d["ex"], rtol=1e-6, atol=0)
    h = bfm.bandpass_taps(2 * d["f0"] * 0.65, 2 * d["f0"] * 1.35, bfm.axial_rate(d["z"], d["c"]))
    raw = mi.nonlinear_beamform(d["data"], d["tx"], probe.geometry[0], d["x"], d["z"], d["fs"], d["c"], method="fdmas", f_number=0.0)
    assert np.array_equal(bf.beamform(d["data"], scan), mi.axial_fir(raw, h))
    bf.update_setup("band", None)
    assert np.array_equal(bf.beamform(d["data"], scan), raw)
    cx = mi.default_context()
    bf.update_setup("band", "default")
    on_dev = bf.beamform(mi.DeviceBuffer.from_host(cx, d["data"]), scan)
    assert isinstance(on_dev, mi.DeviceBuffer) and np.array_equal(on_dev.numpy(), mi.axial_fir(raw, h))


@pytest.mark.parametrize("which", ["fdmas", "pdas"])
def test_us_render_with_the_new_beamformers(mi, which):
    """the plate phantom of the finite-difference loop (tests/scenes/us_plate.xml) on a 64 x 200 scan at lambda / 16 around the plate.
    One path per ray: a channel word then receives a few echoes at the most, and the acquisition's float32 atomic adds give the same
    word in any order of two -- the replayed chain is compared bit for bit with the call before it."""
    make = (lambda **kw: mi.FilteredDelayMultiplyAndSum(**kw)) if which == "fdmas" else (lambda **kw: mi.PDelayAndSum(p=2.0, **kw))
    sc = mi.load_file(scene_path("us_plate.xml"), paths_per_ray=1, seed=4)
    ui = sc.integrator()
    lam = ui.sound_speed / ui.frequency
    step = lam / 16
    kw = dict(x_range=(-31.5 * step, 31.0 * step), z_range=(0.05 - 99.5 * step, 0.05 + 99.0 * step), step=step)
    bf = make()
    imgs, flags = [], []
    for _ in range(3):
        tm = {}
        disp, env, (xs, zs) = mi.us_render(sc, beamformer=bf, timing=tm, **kw)
        imgs.append((disp, env))
        flags.append(tm["replayed"])
    assert len(xs) <= 64 and len(zs) <= 200 and disp.shape == (len(zs), len(xs)) and env.shape == (len(xs), len(zs))
    assert flags == [False, False, True]
    assert np.array_equal(imgs[2][0], imgs[1][0]) and np.array_equal(imgs[2][1], imgs[1][1]) and env.max() > 0
    plan = ui._render_plan
    rf_dev = plan.d_bf.numpy()                                  # the band-passed RF image of the device-resident chain
    # device_resident=False: its own acquisition through the host-pointer forms -- compared as RF images, on the scale B of the first
    # tolerance: the host chain's beamformer run on the channel buffer the device chain used gives the same bits, and the restatement
    # in float32 / float64 sets the floor for that buffer
    chan = np.asarray(ui.channel_buf, np.float32).reshape(ui.n_angles, ui.n_elements, ui.time_samples)
    delays = np.asarray(ui.transmission_delays_buf, np.float32).reshape(ui.n_angles, ui.n_elements)
    probe = mi.build_probe("linear", ui.n_elements, ui.pitch, ui.frequency, 70)
    host_bf = make().automatic_setup({"sampling_freq": ui.fs, "t0": 0, "delays": delays, "sound_speed": ui.sound_speed}, probe)
    scan = mi.GridScan(xs, zs)
    assert np.array_equal(host_bf.beamform(chan, scan), rf_dev)
    taps = host_bf.filter_taps(scan, ui.sound_speed)
    args = (chan, delays, probe.geometry[0], xs, zs, ui.fs, ui.sound_speed)
    ref, B = nu.beamform(which, *args, p=2.0)
    f32, _ = nu.beamform(which, *args, p=2.0, dtype=np.float32)
    left_out, _ = nu.margins(delays, probe.geometry[0], xs, zs, ui.time_samples, ui.fs, ui.sound_speed)
    raw = mi.nonlinear_beamform(*args, method=which, p=2.0)
    used = ~left_out & (B > 0)
    assert used.any() and np.abs(ref).max() > 0
    floor = float((np.abs(f32 - ref)[used] / B[used]).max())
    ratio = float((np.abs(raw - ref)[used] / B[used]).max())
    print(f"\nus_render {which}: float32 floor {floor:.3e}, device {ratio:.3e}, {int(left_out.sum())} of {left_out.size} pixels left out")
    assert ratio <= 4.0 * floor
    # ... and pushed through the FIR: |fir(raw) - fir(ref)| <= sum |h| 4 floor B + the FIR's own (2K + 17) u sum |h| |raw|
    K = len(taps) // 2
    keep_cols = ~left_out.any(axis=1)
    bound = nu.fir(4.0 * floor * B, np.abs(taps)) + (2 * K + 17) * du.U32 * nu.fir(np.abs(raw), np.abs(taps))
    assert keep_cols.any() and np.all(np.abs(rf_dev - nu.fir(ref, taps))[keep_cols] <= bound[keep_cols])
    # device_resident=False runs an acquisition of its own: its channel words differ by the order of their float32 atomic adds (2e-5 of
    # the largest, tests/test_gpu_beamform.py), and a signed root turns a difference d of a sample into at most sqrt(d): 4.5e-3, doubled
    d_host, b_host, _ = mi.us_render(sc, beamformer=make(), device_resident=False, **kw)
    assert d_host.shape == disp.shape and np.allclose(b_host, imgs[1][1], rtol=0, atol=1e-2 * env.max())
    # another p is another recording: the next call queues the plain way, and (p-DAS) the image changes
    if which == "pdas":
        bf.update_setup("p", 3.0)
        tm = {}
        _, env3, _ = mi.us_render(sc, beamformer=bf, timing=tm, **kw)
        assert not tm["replayed"] and not np.array_equal(env3, imgs[1][1])
        bf.update_setup("p", 2.0)
    else:
        bf.update_setup("f_number", 1.5)
        tm = {}
        mi.us_render(sc, beamformer=bf, timing=tm, **kw)
        assert not tm["replayed"]
        bf.update_setup("f_number", 1.0)
    # on_device: buffers, still being written; they match after synchronize()
    for _ in range(3):
        tm = {}
        d_img, d_env, _ = mi.us_render(sc, beamformer=bf, on_device=True, timing=tm, **kw)
    assert tm["replayed"] and isinstance(d_img, mi.DeviceBuffer) and d_img.shape == (len(xs), len(zs)) == d_env.shape
    sc.device().ctx.synchronize()
    assert np.array_equal(d_env.numpy(), imgs[1][1]) and np.array_equal(d_img.numpy().T, imgs[1][0])


def test_us_render_convex_and_gaussian_take_the_new_beamformers(mi):
    """the convex probe (element table -> probe = 1) and the Gaussian pulse model through us_render with F-DMAS and p-DAS"""
    from test_gpu_convex_array import _scene
    sc = _scene(mi, paths_per_ray=4)
    ui = sc.integrator()
    step = (ui.sound_speed / ui.frequency) / 16
    R = ui.radius                       # z is measured from the centre of curvature: the plate lies at R + 20 mm
    kw = dict(x_range=(-20 * step, 20 * step), z_range=(R + 0.02 - 60 * step, R + 0.02 + 60 * step), step=step)
    for bf in (mi.FilteredDelayMultiplyAndSum(), mi.PDelayAndSum(p=1.5)):
        disp, env, (xs, zs) = mi.us_render(sc, beamformer=bf, **kw)
        assert np.isfinite(env).all() and env.max() > 0 and disp.shape == (len(zs), len(xs))
        chan = np.asarray(ui.channel_buf, np.float32).reshape(ui.n_angles, ui.n_elements, ui.time_samples)
        delays = np.asarray(ui.transmission_delays_buf, np.float32).reshape(ui.n_angles, ui.n_elements)
        probe = mi.build_probe("convex", ui.n_elements, ui.pitch, ui.frequency, 70, radius=ui.radius, opening_angle=ui.opening_angle)
        host = type(bf)(**({"p": 1.5} if isinstance(bf, mi.PDelayAndSum) else {}))
        host.automatic_setup({"sampling_freq": ui.fs, "t0": 0, "delays": delays, "sound_speed": ui.sound_speed}, probe)
        assert np.array_equal(host.compute_envelope(host.beamform(chan, mi.GridScan(xs, zs))), env)
    sc = mi.load_file(scene_path("us_plate.xml"), paths_per_ray=2, seed=6)
    ui = sc.integrator()
    ui.pulse_model = "gaussian"
    ui.quirks |= mi._capi.USQ_NO_CARRIER
    step = (ui.sound_speed / ui.frequency) / 16
    kw = dict(x_range=(-16 * step, 16 * step), z_range=(0.05 - 60 * step, 0.05 + 60 * step), step=step)
    env = mi.us_render(sc, beamformer=mi.FilteredDelayMultiplyAndSum(), **kw)[1]
    assert np.isfinite(env).all() and env.max() > 0
