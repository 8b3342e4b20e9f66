"""Sector scans on the device: the walk on pixel tables (pbrt_scan_beamform and its _dev / _table_dev forms,
pbrt_scan_first_arrival_dev), k_scan_convert, and us_render(scan="polar") end to end.

1. On the tables of a separable scan the pixel-table calls give the bits of the calls on the axes: every case of tests/walk_cases.py, every
   method, the host, _dev and _table_dev forms, and the first-arrival table.
2. On a sector the device is held to the float64 restatements of the beamformers, evaluated pixel by pixel (scan_util.per_pixel), with
   the project's bounds: das_util.tolerance / convex_util.das_tolerance for delay-and-sum, four times the float32 floor on the scale B
   for p-DAS, F-DMAS and I/Q.  The cases read (nx, nz) as (n_theta, n_rho): 9 x 13, 9 x 17 and 24 x 16 (partial tiles), 1 / 5 / 6 / 11
   transmissions and 3 / 64 / 65 / 130 elements.
3. The scan conversion against scan_util.scan_convert: four times its float32 floor on the scale max |corner| (C_SC 2^-24 where the floor
   is zero), the inside mask, constants, fill = NaN, one NaN sample, host against _dev, refusals.
4. us_render(scan="polar"): the three paths give one display image, which is the chain of the public pieces.

Every comparison prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import imgform_util as imu
import scan_util as su
from conftest import scene_path
from walk_cases import C0, CASES, T, geometry

pytestmark = pytest.mark.gpu

METHODS = (("das", 2.0), ("pdas", 2.0), ("pdas", 3.0), ("fdmas", 2.0), ("iq", 2.0))
E_INVALID = -1


def _on_axes(mi, g, d_data, method, p):
    """today's call on the axes x, z, data in HBM -> a host array"""
    args = (g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0)
    if method == "das":
        return mi.das_beamform(d_data, *args, **g["kw"]).numpy()
    if method == "iq":
        return mi.iq_beamform(d_data, *args, su.F_D, **g["kw"]).numpy()
    return mi.nonlinear_beamform(d_data, *args, method=method, p=p, **g["kw"]).numpy()


def _on_tables(mi, g, data, px, pz, method, p, form):
    """scan_beamform on pixel tables: form 'host' (pbrt_scan_beamform), 'dev' (_dev) or 'table' (_table_dev)"""
    kw = dict(g["kw"], method=method, p=p, demod_freq=su.F_D if method == "iq" else None)
    args = (g["tx"], g["elem"], px, pz, g["fs"], C0)
    if form == "host":
        return mi.scan_beamform(data, *args, **kw)
    cx = mi.default_context()
    table = mi.scan_first_arrival(g["tx"], g["elem"], px, pz, C0) if form == "table" else None
    out = mi.scan_beamform(mi.DeviceBuffer.from_host(cx, data), *args, table=table, **kw)
    assert isinstance(out, mi.DeviceBuffer) and out.shape == px.shape and out.dtype == (np.complex64 if method == "iq" else np.float32)
    return out.numpy()


# ---- 1. the same bits as the axes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_pixel_tables_of_a_separable_scan_give_the_bits_of_the_axes(mi, name):
    g = geometry(name)
    px, pz = np.meshgrid(g["x"], g["z"], indexing="ij")
    assert px.dtype == np.float32 and px.shape == (len(g["x"]), len(g["z"]))
    cx = mi.default_context()
    rf, iq = su.rf_data(name), su.iq_data(name)
    for method, p in METHODS:
        data = iq if method == "iq" else rf
        want = _on_axes(mi, g, mi.DeviceBuffer.from_host(cx, data), method, p)
        assert np.any(want != 0)
        for form in ("host", "dev", "table"):
            assert np.array_equal(_on_tables(mi, g, data, px, pz, method, p, form), want), (name, method, p, form)
    want = mi.das_first_arrival(g["tx"], g["elem"], g["x"], g["z"], C0).numpy()
    got = mi.scan_first_arrival(g["tx"], g["elem"], px, pz, C0)
    assert got.shape == (g["A"],) + px.shape and got.dtype == np.float64 and np.array_equal(got.numpy(), want)


# ---- 2. a sector against float64 ---------------------------------------------------------------------------------------------------
def test_the_sectors_leave_out_at_most_two_per_cent():
    for name in CASES:
        g = su.sector(name)
        assert g["left_out"].mean() <= 0.02, (name, g["left_out"].mean())
        assert np.all(g["n_a"].sum(axis=0) > 0), name          # no pixel of these sectors uses no element


@pytest.mark.parametrize("name", list(CASES))
def test_a_sector_against_the_float64_restatement(mi, name):
    g = su.sector(name)
    px, pz, keep = g["px"], g["pz"], ~g["left_out"]
    rf, iq = su.rf_data(name), su.iq_data(name)
    ref, tol, n_terms = su.das_reference(g, rf)
    got = _on_tables(mi, g, rf, px, pz, "das", 2.0, "host")
    err = np.abs(got.astype(np.float64) - ref)
    print(f"\n{name} das: largest error / tolerance {float((err[keep] / tol[keep]).max()):.3f}, {int(keep.sum())} pixels, "
          f"{int(g['left_out'].sum())} left out")
    assert np.any(got[keep] != 0) and np.all(n_terms[keep] > 0)
    assert np.all(err[keep] <= tol[keep]), name
    for form in ("dev", "table"):
        assert np.array_equal(_on_tables(mi, g, rf, px, pz, "das", 2.0, form), got), (name, form)
    for method, p in METHODS[1:]:
        if method == "iq":
            ref, B, f32 = su.iq_reference(g, iq)
            data = iq
        else:
            ref, B, f32 = su.nl_reference(g, rf, method, p)
            data = rf
        got = _on_tables(mi, g, data, px, pz, method, p, "host")
        used = keep & (B > 0)
        floor = float((np.abs(f32 - ref)[used] / B[used]).max())
        ratio = float((np.abs(got.astype(f32.dtype) - ref)[used] / B[used]).max())
        print(f"{name} {method} p={p}: float32 floor {floor:.3e}, device {ratio:.3e} ({ratio / floor:.2f} x), {int(used.sum())} pixels")
        assert used.sum() == keep.sum() and ratio <= 4.0 * floor, (name, method, p, ratio, floor)
        for form in ("dev", "table"):
            assert np.array_equal(_on_tables(mi, g, data, px, pz, method, p, form), got), (name, method, form)


def test_tiles_of_a_sector_that_see_no_element_are_exactly_zero(mi):
    """three elements under f# = 1 and a sector from -10 to 60 degrees: beyond atan(1 / 2) no element receives a pixel -- the restatement's
    N_a is 0 in both tiles of the last eight rays and nowhere zero in a whole tile of the first sixteen"""
    name = "a6_e3_wide_lin_f1_mean"
    g = su.sector(name, (-10.0, 60.0))
    none = g["n_a"].sum(axis=0) == 0
    assert none.shape == (24, 16) and not g["left_out"].any()
    assert none[16:, :8].all() and none[16:, 8:].all()
    assert not any(none[i:i + 8, j:j + 8].all() for i in (0, 8) for j in (0, 8)) and not none[:8].any()
    rf, iq = su.rf_data(name), su.iq_data(name)
    for method, p in METHODS:
        for form in ("host", "dev", "table"):
            got = _on_tables(mi, g, iq if method == "iq" else rf, g["px"], g["pz"], method, p, form)
            assert np.all(got[none] == 0), (method, form)
            assert not np.signbit(got[none].real).any() and not np.signbit(got[none].imag).any()
            assert np.all(got[:8] != 0), (method, form)


def _scan_call(mi, capi, method, p=2.0, f_d=0.0, probe=0, iq_data=False):
    name = "a1_e3_small_lin_f0_sum"
    g = geometry(name)
    px, pz = np.meshgrid(g["x"], g["z"], indexing="ij")
    cx = mi.default_context()
    data = su.iq_data(name) if iq_data else su.rf_data(name)
    bufs = [mi.DeviceBuffer.from_host(cx, a) for a in (data, g["tx"], g["elem"], px, pz)]
    out = mi.DeviceBuffer(cx, px.shape, np.complex64)
    out.upload(np.full(px.shape, 7.0, np.complex64))
    sp = capi.ScanParams()
    d = sp.das
    d.n_angles, d.n_elements, d.time_samples, d.fs, d.sound_speed, d.interpolation = g["A"], g["E"], T, g["fs"], C0, capi.DAS_LINEAR
    d.nx, d.nz = px.shape
    sp.method, sp.p, sp.demod_freq, sp.probe = method, p, f_d, probe
    rc = cx.lib.pbrt_scan_beamform_dev(cx.handle, C.byref(sp), *(b.ptr for b in bufs), out.ptr)
    return rc, out.numpy()


def test_scan_beamform_refusals(mi, capi):
    """the checks of the calls the family sits beside, with their error code, and nothing is launched: the output keeps its bytes"""
    for method, kw in ((capi.SCAN_DAS, {}), (capi.BF_PDAS, dict(p=1.0)), (capi.BF_PDAS, dict(p=8.0)), (capi.BF_FDMAS, dict(p=99.0)),
                       (capi.SCAN_IQ, dict(f_d=0.0, iq_data=True)), (capi.SCAN_DAS, dict(p=99.0, f_d=float("nan")))):
        assert _scan_call(mi, capi, method, **kw)[0] == 0, (method, kw)
    for method, kw in ((4, {}), (99, {}), (capi.BF_PDAS, dict(p=0.5)), (capi.BF_PDAS, dict(p=9.0)), (capi.BF_PDAS, dict(p=float("nan"))),
                       (capi.SCAN_IQ, dict(f_d=-1.0)), (capi.SCAN_IQ, dict(f_d=float("inf"))), (capi.SCAN_DAS, dict(probe=2))):
        rc, out = _scan_call(mi, capi, method, **kw)
        assert rc == E_INVALID and np.all(out == 7.0), (method, kw)
    g = geometry("a1_e3_small_lin_f0_sum")
    with pytest.raises(ValueError, match="one shape"):
        mi.scan_beamform(su.rf_data("a1_e3_small_lin_f0_sum"), g["tx"], g["elem"], np.zeros((3, 4)), np.zeros((4, 3)), g["fs"], C0)
    with pytest.raises(ValueError, match="method"):
        mi.scan_beamform(su.rf_data("a1_e3_small_lin_f0_sum"), g["tx"], g["elem"], np.zeros((3, 4)), np.zeros((3, 4)), g["fs"], C0, method="x")


# ---- 3. scan conversion ------------------------------------------------------------------------------------------------------------
ORIGIN = (0.3e-3, -2.0e-3)          # off the output grid: its z starts at 0.5 mm
SOURCES = {"9x13": (9, 13), "24x16": (24, 16)}
GRIDS = {"7x5": (7, 5), "40x33": (40, 33)}


def _polar(mi, shape):
    nt, nr = shape
    return mi.PolarScan(3.0e-3 + np.arange(nr) * (9.0e-3 / (nr - 1)), np.linspace(-0.5, 0.6, nt), origin=ORIGIN)


def _grid(shape):
    nx, nz = shape
    return (np.linspace(-6.1e-3, 7.3e-3, nx).astype(np.float32), np.linspace(0.5e-3, 11.2e-3, nz).astype(np.float32))


def _axes_of(scan):
    th, rho = scan.thetas, scan.rhos
    return th[0], (th[-1] - th[0]) / (len(th) - 1), rho[0], (rho[-1] - rho[0]) / (len(rho) - 1), scan.origin


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("source", list(SOURCES))
def test_scan_convert_against_the_float64_restatement(mi, source, grid):
    scan, (x, z) = _polar(mi, SOURCES[source]), _grid(GRIDS[grid])
    rng = np.random.default_rng(SOURCES[source][0] * 100 + GRIDS[grid][0])
    src = rng.standard_normal(scan.shape).astype(np.float32)
    ref, bound, floor = su.scan_convert_bound(src, *_axes_of(scan), x, z)
    keep = ~ref["edge"]
    assert ref["edge"].mean() <= 0.02 and ref["inside"].any() and (~ref["inside"]).any()
    got = mi.scan_convert(src, scan, x, z, fill=-3.0)
    assert got.shape == (len(x), len(z)) and got.dtype == np.float32
    inside = ref["inside"]
    assert np.array_equal((got != -3.0)[keep], inside[keep])                       # (noise never interpolates to the fill exactly)
    sel = keep & inside
    err = np.abs(got.astype(np.float64) - ref["out"])
    print(f"\nscan_convert {source} -> {grid}: float32 floor {floor:.3e}, device {float((err[sel] / ref['scale'][sel]).max()):.3e}, "
          f"{int(sel.sum())} pixels inside, {int(ref['edge'].sum())} left out")
    assert floor > 0 and np.all(err[sel] <= bound[sel])
    assert np.all(got[keep & ~inside] == -3.0)
    cx = mi.default_context()
    dev = mi.scan_convert(mi.DeviceBuffer.from_host(cx, src), scan, x, z, fill=-3.0)
    assert isinstance(dev, mi.DeviceBuffer) and dev.shape == got.shape and np.array_equal(dev.numpy(), got)
    # a constant source gives exactly the constant and exactly the fill, NaN as a fill included
    const = mi.scan_convert(np.full(scan.shape, 1.75, np.float32), scan, x, z, fill=0.0)
    assert np.all(const[sel] == 1.75) and np.all(const[keep & ~inside] == 0.0) and not np.signbit(const[keep & ~inside]).any()
    nan_fill = mi.scan_convert(src, scan, x, z, fill=float("nan"))
    assert np.array_equal(np.isnan(nan_fill)[keep], ~inside[keep]) and np.array_equal(nan_fill[sel], got[sel])
    # one NaN sample: NaN at exactly the pixels whose four corners include it
    k = int(np.flatnonzero(sel.ravel())[sel.sum() // 2])            # a sample that a kept pixel reads: the upper corner of its cell
    ti, tj = int(ref["i"].ravel()[k]) + 1, int(ref["j"].ravel()[k]) + 1
    bad = src.copy()
    bad[ti, tj] = np.nan
    hit = su.reads(ref, ti, tj)
    got_bad = mi.scan_convert(bad, scan, x, z, fill=-3.0)
    assert hit[keep].any() and not hit[keep].all()
    assert np.array_equal(np.isnan(got_bad)[keep], hit[keep]) and np.array_equal(got_bad[keep & ~hit], got[keep & ~hit])


def test_scan_convert_refusals(mi, capi):
    cx = mi.default_context()
    src, (x, z) = np.ones((4, 5), np.float32), _grid((7, 5))
    out = np.full((7, 5), 7.0, np.float32)

    def call(**kw):
        sc = capi.ScanConvertParams()
        sc.n_theta, sc.n_rho, sc.nx, sc.nz = 4, 5, 7, 5
        sc.theta0, sc.dtheta, sc.rho0, sc.drho, sc.ox, sc.oz, sc.fill = -0.5, 0.3, 3e-3, 2e-3, 0.0, 0.0, 0.0
        for k, v in kw.items():
            setattr(sc, k, v)
        out[:] = 7.0
        return cx.lib.pbrt_scan_convert(cx.handle, C.byref(sc), src.ctypes.data, x.ctypes.data, z.ctypes.data, out.ctypes.data)

    assert call() == 0 and not np.all(out == 7.0)
    assert call(fill=float("nan")) == 0
    for kw in (dict(n_theta=1), dict(n_rho=1), dict(n_theta=0), dict(dtheta=0.0), dict(drho=0.0), dict(theta0=float("nan")),
               dict(dtheta=float("inf")), dict(rho0=float("nan")), dict(drho=float("nan")), dict(ox=float("inf")), dict(oz=float("nan"))):
        assert call(**kw) == E_INVALID and np.all(out == 7.0), kw
    with pytest.raises(ValueError, match="scan's shape"):
        mi.scan_convert(np.ones((5, 4), np.float32), mi.PolarScan(np.arange(1, 6) * 1e-3, np.linspace(-0.1, 0.1, 4)), x, z)


# ---- 4. us_render(scan="polar") ----------------------------------------------------------------------------------------------------
def _three_paths(mi, sc, **kw):
    """queued, queued and recorded, replayed, and device_resident=False -> the replayed (display, envelope, axes)"""
    imgs, flags = [], []
    for _ in range(3):
        tm = {}
        imgs.append(mi.us_render(sc, scan="polar", timing=tm, **kw))
        flags.append(tm["replayed"])
    assert flags == [False, False, True]
    host = mi.us_render(sc, scan="polar", device_resident=False, **kw)
    for k, other in (("queued", imgs[0]), ("recorded", imgs[1]), ("host", host)):
        d = np.abs(other[0].astype(np.float64) - imgs[2][0])
        print(f"\nus_render polar, {k} against replayed: largest difference of the display image {float(d.max()):.3e}")
    assert np.array_equal(imgs[0][0], imgs[2][0]) and np.array_equal(imgs[1][0], imgs[2][0]) and np.array_equal(imgs[1][1], imgs[2][1])
    assert np.array_equal(host[0], imgs[2][0])
    return imgs[2]


def _pieces(mi, ui, probe, scan, xs, zs, kind, dr=60.0):
    """the chain from the public pieces on the fetched channel buffer -> (envelope on the sector, converted envelope [nx, nz])"""
    chan = np.asarray(ui.channel_buf, np.float32).reshape(ui.n_angles, ui.n_elements, ui.time_samples)
    delays = np.asarray(ui.transmission_delays_buf, np.float32).reshape(ui.n_angles, ui.n_elements)
    px, pz = scan.pixels()
    args = (delays, probe.das_elements, px, pz, ui.fs, ui.sound_speed)
    if kind == "iq":
        env = mi.iq_envelope(mi.scan_beamform(mi.rf2iq(chan, ui.frequency, ui.fs), *args, method="iq", demod_freq=ui.frequency))
    elif kind == "fdmas":
        bf = mi.FilteredDelayMultiplyAndSum().automatic_setup({"sound_speed": ui.sound_speed}, probe)
        env = mi.envelope(mi.axial_fir(mi.scan_beamform(chan, *args, method="fdmas"), bf.filter_taps(scan, ui.sound_speed)))
    else:
        env = mi.envelope(mi.scan_beamform(chan, *args))
    return env, mi.scan_convert(env, scan, xs, zs, fill=0.0)


def _check_polar(mi, sc, probe, kind, theta_range, kw, **extra):
    ui = sc.integrator()
    disp, bmode, (xs, zs) = _three_paths(mi, sc, theta_range=theta_range, **extra, **kw)
    step = kw["step"]
    if theta_range is None:
        half = np.radians(ui.opening_angle) / 2
        theta_range = (-half, half)
    n_theta = mi.polar_n_theta(zs[-1], theta_range, step)
    scan = mi.PolarScan(zs, np.linspace(theta_range[0], theta_range[1], n_theta))
    plan = ui._render_plan
    assert plan.d_bf.shape == scan.shape == plan.d_table.shape[1:] and plan.d_img.shape == (len(xs), len(zs))
    assert disp.shape == (len(zs), len(xs)) and bmode.shape == (len(xs), len(zs)) and bmode.max() > 0 and np.isfinite(bmode).all()
    env_sec, env = _pieces(mi, ui, probe, scan, xs, zs, kind)
    assert np.array_equal(plan.d_env_sec.numpy(), env_sec) and np.array_equal(bmode, env)
    bound, ref = imu.log_bound(env, 60.0)
    worst = imu.worst_ratio(disp.T, ref, bound)
    print(f"us_render polar {kind}: sector {scan.shape}, grid {(len(xs), len(zs))}, display against the pieces {worst:.3f} of the log bound")
    assert worst <= 1.0
    u, v = su.polar_coordinates(*_axes_of(scan), xs.astype(np.float32), zs.astype(np.float32))
    outside = (u < -su.EDGE_UV) | (u > n_theta - 1 + su.EDGE_UV) | (v < -su.EDGE_UV) | (v > len(zs) - 1 + su.EDGE_UV)
    assert np.all(disp.T[outside] == 0.0) and np.all(bmode[outside] == 0.0)
    return disp, outside


def _plate(mi, seed=4):
    sc = mi.load_file(scene_path("us_plate.xml"), paths_per_ray=1, seed=seed)
    ui = sc.integrator()
    return sc, ui, mi.build_probe("linear", ui.n_elements, ui.pitch, ui.frequency, 70)


def test_us_render_polar_linear_das(mi):
    sc, ui, probe = _plate(mi)
    step = (ui.sound_speed / ui.frequency) / 4
    kw = dict(x_range=(-12.5 * step, 12 * step), z_range=(0.05 - 32.5 * step, 0.05 + 32 * step), step=step)
    grid = mi.us_render(sc, **kw)
    again = mi.us_render(sc, scan="grid", **kw)
    assert np.array_equal(grid[0], again[0]) and np.array_equal(grid[1], again[1])
    disp, outside = _check_polar(mi, sc, probe, "das", (-0.015, 0.019), kw)
    assert outside.any() and not outside.all() and disp.shape == grid[0].shape
    # the default sector of a linear array: the x-range seen from the deepest z
    d2, _, (xs, zs) = mi.us_render(sc, scan="polar", **kw)
    tr = (np.arctan(kw["x_range"][0] / kw["z_range"][1]), np.arctan(kw["x_range"][1] / kw["z_range"][1]))
    assert np.array_equal(d2, mi.us_render(sc, scan="polar", theta_range=tr, **kw)[0]) and not np.array_equal(d2, disp)
    # the grid afterwards: the plan key separates the scans
    after = mi.us_render(sc, **kw)
    assert np.array_equal(after[0], grid[0]) and np.array_equal(after[1], grid[1])
    with pytest.raises(ValueError, match="theta_range belongs"):
        mi.us_render(sc, theta_range=(-0.1, 0.1), **kw)


def test_us_render_polar_fdmas(mi):
    sc, ui, probe = _plate(mi)
    step = (ui.sound_speed / ui.frequency) / 16
    kw = dict(x_range=(-31.5 * step, 31.0 * step), z_range=(0.05 - 99.5 * step, 0.05 + 99.0 * step), step=step)
    _, outside = _check_polar(mi, sc, probe, "fdmas", (-8.0e-3, 9.0e-3), kw, beamformer=mi.FilteredDelayMultiplyAndSum())
    assert outside.any()


def test_us_render_polar_iq(mi):
    sc, ui, probe = _plate(mi)
    step = (ui.sound_speed / ui.frequency) / 4
    kw = dict(x_range=(-12.5 * step, 12 * step), z_range=(0.05 - 32.5 * step, 0.05 + 32 * step), step=step)
    _, outside = _check_polar(mi, sc, probe, "iq", (-0.015, 0.019), kw, iq=True)
    assert outside.any()


def test_us_render_polar_convex(mi):
    """the curved array: the default sector is its opening angle, around the centre of curvature"""
    from test_gpu_convex_array import _scene
    sc = _scene(mi, paths_per_ray=1)
    ui = sc.integrator()
    probe = mi.build_probe("convex", ui.n_elements, ui.pitch, ui.frequency, 70, radius=ui.radius, opening_angle=ui.opening_angle)
    step = (ui.sound_speed / ui.frequency) / 2
    R = ui.radius
    kw = dict(x_range=(-330 * step, 330 * step), z_range=(R + 0.02 - 20 * step, R + 0.02 + 20 * step), step=step)
    _, outside = _check_polar(mi, sc, probe, "das", None, kw)
    assert outside.any() and not outside.all()
