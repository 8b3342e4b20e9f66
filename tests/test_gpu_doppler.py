"""Colour and power Doppler on the device (include/pbrt_hip.h) against its restatement tests/doppler_util.py.
The rule is the project's for every beamformer: |device - float64| / B <= 4 x the float32 floor, the floor being the largest
|float32 restatement - float64| / B of the same case, B the sum of the absolute values of everything added up; the velocity, an angle,
is held to (nyquist / pi) (4 floor B_R1 / |R1| + 8 2^-24 pi) on the pixels with |R1| >= 1e-3 B_R1 (atan2f's six ulp and the product),
and at most 10 % of an image may be left out.  Then the exact statements, the three forms, every rule through the C-ABI, the Python
layer's ValueErrors and doppler_render end to end on the moving plate of D24.  Shapes are the smallest at which the kernels can go
wrong: 13 x 37 (no multiple of a tile, a wave or a workgroup; two workgroups of the autocorrelation, four tiles of the maps), 1 x 1,
70 x 5 (nine rows of tiles), 5 x 9 under a 15 x 15 window (larger than the image), 1 x 65, 65 x 1 and 9 x 33 under windows 15 long.
Every instance of k_doppler_autocorr (no filter, degrees 0 .. 3) runs at N = degree + 2 and above.  Non-finite and rescaled data and
doppler_render beyond one configuration: tests/test_gpu_doppler_edges.py."""
import ctypes as C
import math

import numpy as np
import pytest

import doppler_util as du

pytestmark = pytest.mark.gpu

E_INVALID = -1
NONE = 0xFFFFFFFF
NYQ = 0.3


def _q(mi, N, d):
    return None if d is None else mi.wall_basis(N, d)


def _held(name, dev, f64, f32, B):
    floor, ratio = du.floor_of(f32, f64, B), du.ratio_of(dev, f64, B)
    print(f"{name}: floor {floor:.3e}, device {ratio:.3e}, quotient {ratio / floor if floor else float('nan'):.2f}")
    assert ratio <= 4.0 * floor, (name, ratio, floor)
    return floor


ACF_CASES = [(N, d, (13, 37)) for N in (2, 3, 8, 17, 64) for d in (None, 0, 1, 3) if d is None or d + 1 < N] + [(8, 3, (70, 5)), (17, None, (70, 5))]
# degree 2 (k_doppler_autocorr<3>), and the tightest ensemble N = degree + 2 of degrees 2 and 3 (those of 0 and 1 are above)
ACF_CASES += [(N, 2, (13, 37)) for N in (4, 8, 17, 64)] + [(5, 3, (13, 37))]


@pytest.mark.parametrize("N,d,shape", ACF_CASES)
def test_autocorrelation_against_the_restatement(mi, N, d, shape):
    """random complex frames plus a clutter polynomial (of the filter's degree; degree 0 without a filter) 1e3 times stronger"""
    x = du.ensemble(np.random.default_rng(1000 * N + 10 * (d or 0) + shape[0]), N, shape, d=d or 0)
    q = _q(mi, N, d)
    f64, B = du.autocorr(x, q)
    f32, _ = du.autocorr(x, q, dtype=np.float32)
    got = mi.doppler_autocorr(x, "none" if d is None else "poly", d or 0)
    assert got.shape == (3,) + shape and got.dtype == np.float32
    for plane, name in enumerate(("Re R1", "Im R1", "R0")):
        _held(f"N = {N}, degree {d}, {shape}, {name}", got[plane], f64[plane], f32[plane], B[plane])


def test_autocorrelation_of_a_1_x_1_image(mi):
    """One pixel, one thread of one workgroup.  The floor of a single pixel is ONE sample of a rounding error, and the quotient of two
    such samples has no bound (the first run of this case on random data gave 0.87, 0.13 and 5.53 on the three planes of one pixel,
    beside at most 2.54 over the 481 pixels of every other case), so this case takes data on which every operation of the header is
    exact in float32: integer-valued random samples in [-8, 8] plus a clutter constant 1e3 times stronger, N = 4 under degree 0, where
    q = 1/2 exactly.  Then u = x - x_0 is an integer, c = sum u / 2, y = u - c / 2 is a multiple of 1/4 below 32, the products are multiples of 1/16 below 2^10 and
    R0 = r0 / 4: device, float32 and float64 restatement agree bit for bit, and the rule holds as 0 <= 4 x 0."""
    rng = np.random.default_rng(41)
    noise = rng.integers(-8, 9, size=(4, 1, 1)) + 1j * rng.integers(-8, 9, size=(4, 1, 1))
    x = (noise + 1e3 * (3 - 5j)).astype(np.complex64)
    q = mi.wall_basis(4, 0)
    assert np.array_equal(q, np.full((1, 4), 0.5, np.float32))
    f64, B = du.autocorr(x, q)
    f32, _ = du.autocorr(x, q, dtype=np.float32)
    got = mi.doppler_autocorr(x, "mean")
    assert got.shape == (3, 1, 1) and np.array_equal(f32, f64) and f64[2, 0, 0] > 0
    for plane, name in enumerate(("Re R1", "Im R1", "R0")):
        _held(f"N = 4, degree 0, (1, 1), {name}", got[plane], f64[plane], f32[plane], B[plane])
    assert np.array_equal(got.astype(np.float64), f64)
    vel, amp = mi.doppler_maps(got, NYQ, "hamming", (15, 15))      # a window larger than the one pixel: its centre weights only
    wc = float(du.weights("hamming", 15)[7])
    m64 = du.maps(got, NYQ, "hamming", (15, 15))
    assert vel.shape == (1, 1) and abs(float(amp[0, 0]) - math.sqrt(f64[2, 0, 0]) * wc) <= 4 * du.F32_EPS * float(amp[0, 0])
    assert abs(float(vel[0, 0]) - float(m64["velocity"][0, 0])) <= NYQ / math.pi * 8 * du.F32_EPS * math.pi


@pytest.mark.parametrize("window", ["boxcar", "hamming"])
@pytest.mark.parametrize("shape,kernel", [((13, 37), (1, 1)), ((13, 37), (3, 5)), ((13, 37), (15, 15)), ((5, 9), (15, 15)), ((70, 5), (5, 3))]
                         + [(s, k) for s in ((1, 65), (65, 1), (9, 33)) for k in ((15, 1), (1, 15), (15, 15))])
def test_maps_against_the_restatement(mi, window, shape, kernel):
    """the acf of a pure-tone ensemble plus 10 % noise (float64 restatement, rounded to float32) through pbrt_doppler_maps.  The thin
    images: 1 x 65 (every halo row outside the image, three z-tiles of one row), 65 x 1 (every halo column outside, nine x-tiles of
    one column) and 9 x 33 (one pixel past a tile each way)."""
    acf = du.autocorr(du.tone(np.random.default_rng(7), 8, shape))[0].astype(np.float32)
    m64, m32 = du.maps(acf, NYQ, window, kernel), du.maps(acf, NYQ, window, kernel, dtype=np.float32)
    vel, amp = mi.doppler_maps(acf, NYQ, window, kernel)
    assert vel.shape == shape and amp.shape == shape and vel.dtype == np.float32
    tag = f"{shape}, {window} {kernel}"
    floor = max(du.floor_of(m32["planes"][p], m64["planes"][p], m64["B"][p]) for p in range(3))
    _held(f"{tag}, amplitude", amp, m64["amplitude"], m32["amplitude"], m64["B_amp"])
    bound, kept = du.velocity_bound(m64, NYQ, floor)
    left_out = int((~kept).sum())
    err = np.abs(vel.astype(np.float64) - m64["velocity"])
    print(f"{tag}, velocity: floor of the planes {floor:.3e}, left out {left_out} of {kept.size}, worst error / bound {float((err[kept] / bound[kept]).max()):.3f}")
    assert left_out <= 0.1 * kept.size
    assert np.all(err[kept] <= bound[kept])
    if kernel == (1, 1):   # the identity: the amplitude is the root of the plane itself, correctly rounded
        assert np.array_equal(amp, np.sqrt(acf[2]))


@pytest.mark.parametrize("N", [2, 3, 8, 17, 64])
def test_identical_frames_under_mean_removal_are_exactly_zero(mi, N):
    """N identical frames under degree 0: acf, velocity and amplitude exactly 0 -- the filter works on x_n - x_0, which is exactly 0
    here, and everything after it is sums of products with 0."""
    rng = np.random.default_rng(N)
    frame = (rng.normal(size=(13, 37)) + 1j * rng.normal(size=(13, 37))).astype(np.complex64)
    x = np.repeat(frame[None], N, axis=0)
    acf = mi.doppler_autocorr(x, "mean")
    assert not acf.any()
    if N > 4:
        assert not mi.doppler_autocorr(x, "poly", 3).any()
    for kernel in ((1, 1), (3, 5)):
        vel, amp = mi.doppler_maps(acf, NYQ, "hamming", kernel)
        assert not vel.any() and not amp.any() and not np.signbit(vel).any()
    assert not mi.get_color_doppler_map(x, NYQ, "mean").any() and not mi.get_power_doppler_map(x, "mean").any()


def test_a_1_x_1_kernel_reads_the_pixel_s_own_acf_only(mi):
    """velocity and amplitude of a pixel are functions of its own three values: a second call on the transposed image gives the
    transposed maps, bit for bit"""
    acf = du.autocorr(du.tone(np.random.default_rng(9), 8, (13, 37)))[0].astype(np.float32)
    vel, amp = mi.doppler_maps(acf, NYQ, "hamming", (1, 1))
    vel_t, amp_t = mi.doppler_maps(np.ascontiguousarray(acf.transpose(0, 2, 1)), NYQ, "boxcar", (1, 1))
    assert np.array_equal(vel_t.T, vel) and np.array_equal(amp_t.T, amp)


def test_the_host_form_and_the_dev_form_are_bit_equal(mi):
    cx = mi.default_context()
    x = du.ensemble(np.random.default_rng(5), 8, (13, 37), d=1)
    d_x = mi.DeviceBuffer.from_host(cx, x)
    for wall, degree in (("none", 0), ("mean", 0), ("poly", 3), ("poly", 1), ("poly", 2)):      # (every instance of the kernel)
        host = mi.doppler_autocorr(x, wall, degree)
        d_acf = mi.doppler_autocorr(d_x, wall, degree)
        assert isinstance(d_acf, mi.DeviceBuffer) and d_acf.shape == (3, 13, 37) and np.array_equal(d_acf.numpy(), host)
        for window, kernel in (("hamming", (3, 5)), ("boxcar", (15, 15)), ("boxcar", (1, 1))):
            hv, ha = mi.doppler_maps(host, NYQ, window, kernel)
            dv, da = mi.doppler_maps(d_acf, NYQ, window, kernel)
            assert np.array_equal(dv.numpy(), hv) and np.array_equal(da.numpy(), ha)
    assert np.array_equal(mi.get_color_doppler_map(d_x, NYQ, "mean", kernel=(3, 3)).numpy(), mi.get_color_doppler_map(x, NYQ, "mean", kernel=(3, 3)))
    disp = mi.get_power_doppler_map(x, "mean", kernel=(3, 3), dynamic_range=40.0)
    assert np.array_equal(mi.get_power_doppler_map(d_x, "mean", kernel=(3, 3), dynamic_range=40.0).numpy(), disp)
    assert disp.min() >= 0.0 and disp.max() == 1.0
    assert np.array_equal(disp, mi.log_compress(mi.get_power_doppler_map(x, "mean", kernel=(3, 3)), 40.0))
    # a view is the memory of its parent, and never frees it
    v = d_x.view(3 * 13 * 37, (13, 37))
    assert np.array_equal(v.numpy(), x[3]) and v.parent is d_x
    v.close()
    assert np.array_equal(d_x.view(0, (13, 37)).numpy(), x[0])
    for off, shape in ((8 * 13 * 37, (1,)), (-1, (1,)), (7 * 13 * 37 + 1, (13, 37))):
        with pytest.raises(ValueError):
            d_x.view(off, shape)


def _packet_case(mi):
    rng = np.random.default_rng(11)
    N, A, E, T = 3, 2, 16, 96
    fs, c, f = 10e6, 1500.0, 2.5e6
    probe = mi.build_probe("linear", E, 3e-4, f)
    data = (rng.normal(size=(N, A, E, T)) + 1j * rng.normal(size=(N, A, E, T))).astype(np.complex64)
    tx = (probe.geometry[0][None, :].astype(np.float64) * np.sin(np.deg2rad([-5.0, 5.0]))[:, None] / c).astype(np.float32)
    info = {"sampling_freq": fs, "t0": 0, "delays": tx, "sound_speed": c}
    scan = mi.GridScan(np.linspace(-2e-3, 2e-3, 5), np.linspace(1e-3, 6e-3, 7))
    return data, info, probe, scan


@pytest.mark.parametrize("name", ["DelayAndSum", "Capon"])
def test_beamform_packet_equals_single_beamform_calls(mi, name):
    data, info, probe, scan = _packet_case(mi)
    bf = getattr(mi, name)(is_iq=True).automatic_setup(info, probe)
    want = np.stack([bf.beamform(f, scan) for f in data])
    got = bf.beamform_packet(data, scan)
    assert got.shape == (3, 5, 7) and got.dtype == np.complex64 and np.array_equal(got, want)
    cx = mi.default_context()
    d_frames = [mi.DeviceBuffer.from_host(cx, f) for f in data]
    on_dev = bf.beamform_packet(d_frames, scan)
    assert isinstance(on_dev, mi.DeviceBuffer) and on_dev.shape == (3, 5, 7) and np.array_equal(on_dev.numpy(), want)
    assert bf.acquisition_info["delays"] is info["delays"] and bf.probe_dev is None and scan.d_x is None   # nothing of the call stays behind
    out = mi.DeviceBuffer(cx, (3, 5, 7), np.complex64)
    assert bf.beamform_packet(d_frames, scan, out=out) is out and np.array_equal(out.numpy(), want)
    assert np.array_equal(bf.beamform(data, scan), want[0])      # beamform() reads frame 0 of four-dimensional data, as before
    with pytest.raises(ValueError):
        bf.beamform_packet(d_frames, scan, out=mi.DeviceBuffer(cx, (2, 5, 7), np.complex64))
    with pytest.raises(ValueError):
        bf.beamform_packet(data[0], scan)
    with pytest.raises(ValueError):
        bf.beamform_packet([], scan)
    with pytest.raises(ValueError):
        bf.beamform_packet(data.real.copy(), scan)
    with pytest.raises(ValueError):
        mi.DelayAndSum(is_iq=False).automatic_setup(info, probe).beamform_packet(data, scan)
    with pytest.raises(RuntimeError):
        mi.DelayAndSum(is_iq=True).beamform_packet(data, scan)


# ---- every rule of doppler_request.h through the C-ABI, in both forms ---------------------------------------------------------------
class Form:
    """one form of the entry points: the "_dev" suffix or none, and disjoint buffers of its kind (4096 floats each)"""

    def __init__(self, mi, ctx, dev):
        self.ctx, self.lib, self.dev = ctx, ctx.lib, dev
        fill = np.linspace(0.5, 1.5, 4096, dtype=np.float32)
        self.keep = {k: (mi.DeviceBuffer.from_host(ctx, fill) if dev else fill.copy()) for k in ("frames", "q", "acf", "vel", "amp")}

    def p(self, name, offset=0):
        if name is None:
            return None
        b = self.keep[name]
        return (int(b.ptr) if self.dev else b.ctypes.data) + offset

    def call(self, name, *args, handle=True):
        return getattr(self.lib, name + ("_dev" if self.dev else ""))(self.ctx.handle if handle else None, *args)


@pytest.fixture(scope="module")
def forms(mi):
    ctx = mi.Context()
    yield {"host": Form(mi, ctx, False), "dev": Form(mi, ctx, True)}
    ctx.close()


def _block(capi, **edits):
    p = capi.DopplerParams(n_frames=8, nx=3, nz=5, wall_degree=1, kx=3, kz=5, window=1, nyquist_velocity=0.3)
    for k, v in edits.items():
        setattr(p, k, v)
    return p


def _acf(L, capi, frames="frames", q="q", acf="acf", null_params=False, handle=True, off=0, **edits):
    p = _block(capi, **edits)
    return L.call("pbrt_doppler_autocorr", None if null_params else C.byref(p), L.p(frames), L.p(q), L.p(acf, off), handle=handle)


def _maps(L, capi, acf="acf", vel="vel", amp="amp", null_params=False, handle=True, off=0, **edits):
    p = _block(capi, **edits)
    return L.call("pbrt_doppler_maps", None if null_params else C.byref(p), L.p(acf), L.p(vel, off), L.p(amp), handle=handle)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_every_rule_through_the_c_abi(forms, capi, form):
    L = forms[form]
    assert _acf(L, capi) == 0 and _maps(L, capi) == 0
    assert _acf(L, capi, handle=False) == E_INVALID and _maps(L, capi, handle=False) == E_INVALID
    assert _acf(L, capi, null_params=True) == E_INVALID and _maps(L, capi, null_params=True) == E_INVALID
    # the autocorrelation
    assert _acf(L, capi, frames=None) == E_INVALID and _acf(L, capi, acf=None) == E_INVALID
    for n in (0, 1, 65):
        assert _acf(L, capi, n_frames=n, wall_degree=NONE) == E_INVALID
    assert _acf(L, capi, n_frames=2, wall_degree=NONE) == 0 and _acf(L, capi, n_frames=64, wall_degree=NONE) == 0
    assert _acf(L, capi, wall_degree=4) == E_INVALID and _acf(L, capi, wall_degree=3) == 0
    assert _acf(L, capi, n_frames=4, wall_degree=3) == E_INVALID and _acf(L, capi, n_frames=5, wall_degree=3) == 0
    assert _acf(L, capi, n_frames=2, wall_degree=1) == E_INVALID and _acf(L, capi, n_frames=2, wall_degree=0) == 0
    assert _acf(L, capi, q=None) == E_INVALID and _acf(L, capi, q=None, wall_degree=NONE) == 0
    assert _acf(L, capi, nx=0x10000, nz=0x10000, n_frames=4) == E_INVALID
    assert _acf(L, capi, nx=0x4000000, nz=1, n_frames=64) == E_INVALID
    assert _acf(L, capi, acf="frames") == E_INVALID and _acf(L, capi, acf="frames", off=8 * 15 * 8 - 4) == E_INVALID
    assert _acf(L, capi, acf="q") == E_INVALID and _acf(L, capi, acf="q", wall_degree=NONE) == 0
    assert _acf(L, capi, nx=0) == 0 and _acf(L, capi, nz=0, frames="acf") == 0                 # an empty call touches nothing
    assert _acf(L, capi, kx=2, kz=0, window=9, nyquist_velocity=float("nan")) == 0               # (the other step's fields)
    # the maps
    assert _maps(L, capi, acf=None) == E_INVALID and _maps(L, capi, vel=None) == E_INVALID and _maps(L, capi, amp=None) == E_INVALID
    for k in (0, 2, 16, 17):
        assert _maps(L, capi, kx=k) == E_INVALID and _maps(L, capi, kz=k) == E_INVALID
    assert _maps(L, capi, kx=1, kz=15) == 0 and _maps(L, capi, kx=15, kz=1) == 0
    assert _maps(L, capi, window=2) == E_INVALID and _maps(L, capi, window=0) == 0
    for v in (0.0, -1.0, float("nan"), float("inf")):
        assert _maps(L, capi, nyquist_velocity=v) == E_INVALID
    assert _maps(L, capi, nx=0x10000, nz=0x10000) == E_INVALID
    assert _maps(L, capi, vel="acf") == E_INVALID and _maps(L, capi, vel="acf", off=12 * 15 - 4) == E_INVALID
    assert _maps(L, capi, amp="acf") == E_INVALID and _maps(L, capi, amp="vel") == E_INVALID
    assert _maps(L, capi, nx=0) == 0 and _maps(L, capi, nz=0, vel="acf") == 0
    assert _maps(L, capi, n_frames=0, wall_degree=77) == 0


def test_the_dev_forms_are_recordable_and_the_host_forms_are_not(mi, capi):
    """queued on the context's stream like their neighbours: inside a recording the _dev forms are recorded and replayed with the
    same bits, the host forms are refused by the context"""
    cx = mi.Context()
    x = du.ensemble(np.random.default_rng(3), 8, (13, 37), d=1)
    want_acf = mi.doppler_autocorr(x, "poly", 1)
    want_vel, want_amp = mi.doppler_maps(want_acf, NYQ, "hamming", (3, 5))
    d_x, d_q = mi.DeviceBuffer.from_host(cx, x), mi.DeviceBuffer.from_host(cx, mi.wall_basis(8, 1))
    d_acf, d_vel, d_amp = mi.DeviceBuffer(cx, (3, 13, 37)), mi.DeviceBuffer(cx, (13, 37)), mi.DeviceBuffer(cx, (13, 37))
    p = capi.DopplerParams(n_frames=8, nx=13, nz=37, wall_degree=1, kx=3, kz=5, window=1, nyquist_velocity=NYQ)
    h_q = mi.wall_basis(8, 1)
    host, h_vel, h_amp = np.zeros(3 * 13 * 37, np.float32), np.zeros(13 * 37, np.float32), np.zeros(13 * 37, np.float32)
    with cx.record() as rec:
        assert cx.lib.pbrt_doppler_autocorr_dev(cx.handle, C.byref(p), d_x.ptr, d_q.ptr, d_acf.ptr) == 0
        assert cx.lib.pbrt_doppler_maps_dev(cx.handle, C.byref(p), d_acf.ptr, d_vel.ptr, d_amp.ptr) == 0
        assert cx.lib.pbrt_doppler_autocorr(cx.handle, C.byref(p), x.ctypes.data, h_q.ctypes.data, host.ctypes.data) == E_INVALID
        assert cx.lib.pbrt_last_error(cx.handle).decode().endswith("pbrt_doppler_autocorr cannot run")
        assert cx.lib.pbrt_doppler_maps(cx.handle, C.byref(p), host.ctypes.data, h_vel.ctypes.data, h_amp.ctypes.data) == E_INVALID
        assert cx.lib.pbrt_last_error(cx.handle).decode().endswith("pbrt_doppler_maps cannot run")
    rec.graph.launch()
    assert np.array_equal(d_acf.numpy(), want_acf) and np.array_equal(d_vel.numpy(), want_vel) and np.array_equal(d_amp.numpy(), want_amp)
    rec.graph.close()
    cx.close()


def test_the_value_errors_of_the_python_layer(mi):
    cx = mi.default_context()
    x = np.zeros((4, 3, 5), np.complex64)
    d_real = mi.DeviceBuffer.from_host(cx, np.zeros((4, 3, 5), np.float32))
    d_x = mi.DeviceBuffer.from_host(cx, x)
    with pytest.raises(ValueError):
        mi.doppler_autocorr(d_real)
    with pytest.raises(ValueError):
        mi.doppler_autocorr(d_x, out=mi.DeviceBuffer(cx, (2, 3, 5)))
    with pytest.raises(ValueError):
        mi.doppler_autocorr(d_x, "poly", 3)
    d_acf = mi.doppler_autocorr(d_x)
    with pytest.raises(ValueError):
        mi.doppler_maps(d_acf, NYQ, out=(mi.DeviceBuffer(cx, (3, 5)), mi.DeviceBuffer(cx, (3, 4))))
    with pytest.raises(ValueError):
        mi.doppler_maps(d_x, NYQ)
    with pytest.raises(ValueError):
        mi.doppler_maps(d_acf, NYQ, kernel=(2, 3))
    with pytest.raises(ValueError, match="absolute time"):
        mi.doppler_render(du.plate_scenes(mi, du.LAM / 16, "impulse")[:2], 4000.0)
    with pytest.raises(ValueError, match="two scenes"):
        mi.doppler_render(du.plate_scenes(mi, du.LAM / 16)[:1], 4000.0)


# ---- end to end: the moving plate of DESIGN D24 ---------------------------------------------------------------------------------------
PRF = 4000.0
# 5 x 19 pixels at the default step lambda / 2: x = -lambda .. lambda, z = the 19 depths of DESIGN D24 (18.5 mm in steps of lambda / 2)
RENDER = dict(x_range=(-du.LAM, 0.75 * du.LAM), z_range=(float(du.PLATE_Z[0]), float(du.PLATE_Z[-1]) - du.LAM / 4), step=None, dynamic_range=40.0)


@pytest.fixture(scope="module")
def rendered(mi):
    """doppler_render on the eight plate scenes, dz = +-lambda / 16, wall filter none and mean: the images and the frames it made"""
    out = {}
    for sign in (+1, -1):
        scenes = du.plate_scenes(mi, sign * du.LAM / 16)
        for wall in ("none", "mean"):
            bufs = {}
            vel, disp, (xs, zs) = mi.doppler_render(scenes, PRF, wall_filter=wall, kernel=(1, 1), buffers=bufs, **RENDER)
            out[(sign, wall)] = dict(vel=vel, disp=disp, xs=xs, zs=zs, frames=bufs["frames"].numpy(), acf=bufs["acf"].numpy(),
                                     amp=bufs["amplitude"].numpy(), scenes=scenes)
    return out


def _render_grid():
    """the grid doppler_render makes of RENDER by us_render's rule np.arange(lo, hi + step, step), step = lambda / 2"""
    step = du.LAM / 2
    return (np.arange(RENDER["x_range"][0], RENDER["x_range"][1] + step, step), np.arange(RENDER["z_range"][0], RENDER["z_range"][1] + step, step))


@pytest.mark.parametrize("sign", [+1, -1])
@pytest.mark.parametrize("wall", ["none", "mean"])
def test_doppler_render_on_the_moving_plate(mi, rendered, sign, wall):
    r = rendered[(sign, wall)]
    xs, zs = _render_grid()
    nx, nz = len(xs), len(zs)
    assert np.array_equal(r["xs"], xs) and np.array_equal(r["zs"], zs) and (nx, nz) == (5, 19)
    assert r["vel"].shape == (nz, nx) and r["disp"].shape == (nz, nx) and r["frames"].shape == (8, nx, nz)
    nyq = mi.nyquist_velocity(du.PLATE["c"], PRF, du.PLATE["f"])
    # the two steps on the frames it beamformed, by the two rules above
    q = None if wall == "none" else mi.wall_basis(8, 0)
    f64, B = du.autocorr(r["frames"], q)
    f32, _ = du.autocorr(r["frames"], q, dtype=np.float32)
    floor = 0.0
    for plane, name in enumerate(("Re R1", "Im R1", "R0")):
        floor = max(floor, _held(f"plate {sign:+d}, wall {wall}, {name}", r["acf"][plane], f64[plane], f32[plane], B[plane]))
    m64, m32 = du.maps(r["acf"], nyq), du.maps(r["acf"], nyq, dtype=np.float32)
    _held(f"plate {sign:+d}, wall {wall}, amplitude", r["amp"], m64["amplitude"], m32["amplitude"], m64["B_amp"])
    bound, kept = du.velocity_bound(m64, nyq, 0.0)      # (a 1 x 1 kernel: the planes are the device's own, bit for bit)
    err = np.abs(r["vel"].T.astype(np.float64) - m64["velocity"])
    assert (~kept).sum() <= 0.1 * kept.size and np.all(err[kept] <= bound[kept])
    assert np.array_equal(r["disp"].T, mi.log_compress(r["amp"], RENDER["dynamic_range"]))
    # the physics, by the CPU test's assertion: the sign, and 10 % of the closed form
    keep = r["acf"][2] >= 0.1 * r["acf"][2].max()
    med = float(np.median(np.arctan2(r["acf"][1], r["acf"][0])[keep])) / math.pi
    expected = -4.0 * sign / 16.0
    print(f"doppler_render, dz = {sign:+d} lambda/16, wall {wall}: median arg R1 / pi = {med:+.4f} on {int(keep.sum())} of {keep.size} pixels "
          f"(expected {expected:+.4f}); median velocity {float(np.median(r['vel'].T[keep])):+.4f} m/s of {-sign * du.LAM / 16 * PRF:+.4f}")
    assert keep.sum() >= 4 and med * expected > 0 and abs(med - expected) <= 0.1 * abs(expected)
    assert np.sign(np.median(r["vel"].T[keep])) == -sign


def test_doppler_render_on_device_returns_the_same_bits(mi, rendered):
    """on_device=True hands back the buffers on_device=False copies: DeviceBuffers [nx, nz] whose bits are the chain's on the frames of
    that call.  Held on the frames of the SAME call, through the host forms: two acquisitions of one scene are not equal bit for bit
    (their float32 atomics add in another order, tests/test_gpu_beamform.py), so a second call is no reference for bits."""
    r = rendered[(+1, "mean")]
    bufs = {}
    d_vel, d_disp, (xs, zs) = mi.doppler_render(r["scenes"], PRF, wall_filter="mean", kernel=(1, 1), on_device=True, buffers=bufs, **RENDER)
    assert isinstance(d_vel, mi.DeviceBuffer) and isinstance(d_disp, mi.DeviceBuffer) and d_vel.shape == d_disp.shape == (len(xs), len(zs))
    nyq = mi.nyquist_velocity(du.PLATE["c"], PRF, du.PLATE["f"])
    vel, amp = mi.doppler_maps(mi.doppler_autocorr(bufs["frames"].numpy(), "mean"), nyq, "hamming", (1, 1))
    assert np.array_equal(d_vel.numpy(), vel) and np.array_equal(d_disp.numpy(), mi.log_compress(amp, RENDER["dynamic_range"]))
    assert np.array_equal(bufs["amplitude"].numpy(), amp)
    # and the copies of on_device=False are these buffers' transposes: a second call on the same scenes agrees to the acquisition's
    # tolerance, not to the bit
    assert r["vel"].shape == d_vel.shape[::-1] and np.sign(np.median(d_vel.numpy())) == np.sign(np.median(r["vel"]))
