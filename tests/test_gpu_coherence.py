"""Spatial-coherence beamforming on the device: k_coherence_beamform -- SLSC and the coherence factor -- against the
float64 restatement of tests/coherence_util.py on the walk cases, the bit-equalities of the call forms, the exact statements that follow
from the definition, the scale of the data, the kernel at the ends of a trace, non-finite samples and geometry, the point scatterer, the
refusals, the classes and us_render.

The geometries are the eight walk cases of test_gpu_capon.py: N = 3, tiles with no element, a second and a third block of 64 elements,
N = 130 (the cap of 64 lags binds at lag_prop 1), both convex cases, both interpolations and both compounds.

The bound of the comparison, per case, input family, demodulation frequency and setting: the device's largest |got - f64| / B over the
pixels compared is at most 4 x floor.  B = sum_a M_a (SLSC) or sum_a sum_k |v_k| (CF) per pixel; the floor is the largest |restatement in
np.float32 - restatement in float64| / B over the same pixels, the larger of the two orders of every sum; the factor 4 is the project's
(D19, D23).  Every case prints its floor and the device's ratio before it asserts; profiles/coherence.md records them."""
import ctypes as C

import numpy as np
import pytest

import capon_util as ku
import coherence_util as cu
import nlbf_util as nu
from conftest import scene_path
from walk_cases import C0, T, geometry

pytestmark = pytest.mark.gpu

NAMES = ("a1_e3_small_lin_f0_sum", "a6_e3_wide_lin_f1_mean", "a5_e64_lin_f1_sum", "a6_e65_near_f1_mean", "a5_e65_small_near_f0_sum",
         "a11_e130_small_near_f0_sum", "a5_e16_convex_lin_f1_sum", "a6_e16_convex_small_near_f0_mean")
LINE_NAMES = tuple(n for n in NAMES if "convex" not in n)
SLSC_SETTINGS = (("slsc", 0.3, 1), ("slsc", 1.0, 4), ("slsc", 0.1, 0))
CF_SETTINGS = (("cf", 0.0), ("cf", 1.0), ("cf", 0.5), ("cf", 2.0))
SETTINGS = SLSC_SETTINGS + CF_SETTINGS
F_DS = (0.0, 3.0e6)
E_INVALID = -1


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(a.shape + (2,)) if a.dtype == np.complex64 else a.view(np.uint32)


def image(mi, g, data, f_d, setting, form="dev", tables=False, t0=0.0, tx=None, edit_table=None):
    """the library's image through the Python layer: form 'dev', 'table' or 'host'; tables: the scan as np.meshgrid(x, z);
    edit_table: a function of the first-arrival table [A, nx, nz] (float64, on the host) that changes it in place"""
    gx, gz = np.meshgrid(g["x"], g["z"], indexing="ij") if tables else (g["x"], g["z"])
    tx = g["tx"] if tx is None else tx
    kw = dict(g["kw"], tables=tables, t0=t0, **cu.settings_kw(setting))
    if form != "host":
        cx = mi.default_context()
        data = mi.DeviceBuffer.from_host(cx, np.ascontiguousarray(data))
        if form == "table":
            table = (mi.scan_first_arrival if tables else mi.das_first_arrival)(tx, g["elem"], gx, gz, C0)
            if edit_table is not None:
                host = table.numpy()
                edit_table(host)
                table = mi.DeviceBuffer.from_host(cx, host)
            kw["table"] = table
    out = mi.coherence_beamform(data, tx, g["elem"], gx, gz, g["fs"], C0, f_d, **kw)
    out = out if form == "host" else out.numpy()
    assert out.dtype == (np.float32 if setting[0] == "slsc" else np.complex64)
    return out


def compare(got, ref, B, used):
    return float((np.abs(got.astype(ref.dtype) - ref)[used] / B[used]).max())


# ---- 1. the device against the float64 restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "_".join(str(v) for v in s))
@pytest.mark.parametrize("f_d", F_DS)
@pytest.mark.parametrize("which", ["noise", "coherent"])
@pytest.mark.parametrize("name", NAMES)
def test_device_against_the_float64_restatement(mi, name, which, f_d, setting):
    g = geometry(name)
    data = ku.case_data(name, which)
    ref, B, edge, _ = cu.restated(name, which, f_d, setting)
    left_out = g["left_out"] | edge
    assert left_out.mean() <= 0.02
    keep = ~left_out
    unused = (g["n_a"].sum(axis=0) == 0) & keep
    used = keep & (B > 0)
    floor = cu.floor_of(name, which, f_d, setting, used)
    got = image(mi, g, data, f_d, setting)
    ratio = compare(got, ref, B, used)
    print(f"\n{name} {which} f_d={f_d:g} {setting}: float32 floor {floor:.2e}, device {ratio:.2e} ({ratio / floor:.2f} x), "
          f"{int(used.sum())} pixels, {int(left_out.sum())} left out, N up to {int(g['n_a'].max())}")
    assert used.any() and np.all(bits(got)[unused] == 0), (name, setting)          # a pixel that uses no element is exactly +0 / (+0, +0)
    assert np.all(bits(got)[keep & (B == 0)] == 0), (name, setting)                # (SLSC: nor does one element alone have a lag)
    assert ratio <= 4.0 * floor, (name, which, f_d, setting, ratio, floor)
    if which == "noise" and f_d != 0.0:
        # the first-arrival table changes no bit, nor does staging from host memory, nor the tables of the separable scan
        want = bits(got)
        assert np.array_equal(bits(image(mi, g, data, f_d, setting, "table")), want), (name, setting, "table")
        assert np.array_equal(bits(image(mi, g, data, f_d, setting, "host")), want), (name, setting, "host")
        assert np.array_equal(bits(image(mi, g, data, f_d, setting, "dev", tables=True)), want), (name, setting, "tables")
        assert np.array_equal(bits(image(mi, g, data, f_d, setting, "table", tables=True)), want), (name, setting, "table, tables")


# ---- 2. exact statements, without a carrier and with H = 0 ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_equal_samples_are_fully_coherent_bit_for_bit(mi, name):
    """all samples (1, 0): every unit row is (1, 0), every C is 1, the sum over N - m pairs divided by N - m is 1 and SLSC is
    sum_a M(N_a); the coherence factor is N^2 / (N N) = 1 at any gamma and the image is I/Q delay-and-sum's sum_a N_a -- in float32
    without a rounding, so bit for bit (mean: one float32 division by A)"""
    g = geometry(name)
    ones = np.ones((g["A"], g["E"], T), np.complex64)
    keep = ~g["left_out"]
    mean = g["kw"]["compound"] == "mean"
    for lag_prop in (0.3, 1.0, 0.1):
        want = np.vectorize(lambda n: cu.lags(n, lag_prop))(g["n_a"]).sum(axis=0).astype(np.float32)
        want = want / np.float32(g["A"]) if mean else want
        got = image(mi, g, ones, 0.0, ("slsc", lag_prop, 0))
        assert np.any(want[keep] > 0) or g["E"] == 3
        assert np.array_equal(bits(got)[keep], bits(want)[keep]), (name, lag_prop)
    das = mi.iq_beamform(ones, g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, 0.0, **g["kw"])
    count = g["n_a"].sum(axis=0).astype(np.float32)
    assert np.array_equal(das.real[keep], count[keep] / np.float32(g["A"]) if mean else count[keep]) and np.all(das.imag == 0)
    for setting in CF_SETTINGS:
        got = image(mi, g, ones, 0.0, setting)
        assert np.array_equal(bits(got), bits(das)), (name, setting)


@pytest.mark.parametrize("name", LINE_NAMES)
def test_alternating_traces(mi, name):
    """traces (-1)^e on a line, where the ranks are consecutive elements: C(i, i + m) = (-1)^m exactly, their sum over N - m pairs
    divided by N - m is (-1)^m exactly, y_a is -1 or 0 and the clamp leaves +0 at EVERY pixel.  CF at gamma = 1: S_a is 0 or +-1, Q_a =
    N, y_a = S_a / N^2 -- against the restatement within (4 + A) 2^-24 sum_a 1 / N_a^2: per transmission one division and two products,
    each rounded once relative to |y_a| <= 1 / N_a^2, and A - 1 roundings of partial sums no larger than sum_a |y_a|."""
    g = geometry(name)
    data = np.broadcast_to(((-1.0) ** np.arange(g["E"]))[None, :, None], (g["A"], g["E"], T)).astype(np.complex64)
    for lag_prop in (0.3, 1.0):
        got = image(mi, g, data, 0.0, ("slsc", lag_prop, 0))
        assert np.all(bits(got) == 0), (name, lag_prop)
    keep = ~g["left_out"]
    ref, _, _, _ = cu.coherence(data, g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, 0.0, kind="cf", gamma=1.0, **g["kw"])
    got = image(mi, g, data, 0.0, ("cf", 1.0)).astype(np.complex128)
    scale = 1.0 / g["A"] if g["kw"]["compound"] == "mean" else 1.0
    bound = (4 + g["A"]) * 2.0 ** -24 * (np.where(g["n_a"] > 0, 1.0 / np.maximum(g["n_a"], 1) ** 2, 0.0)).sum(axis=0) * scale
    err = np.abs(got - ref)
    print(f"\n{name}: largest error / bound {np.max(err[keep] / np.maximum(bound[keep], 1e-300)):.3f}")
    assert np.any(ref[keep] != 0) and np.all(err[keep] <= bound[keep])


def test_zero_aperture_tiles_are_exactly_zero(mi):
    name = "a6_e3_wide_lin_f1_mean"
    g = geometry(name)
    none = g["n_a"].sum(axis=0) == 0
    assert none[:8].all() and none[16:].all() and not none[8:16].all()       # the outer x tiles see no element, the middle one does
    for setting in (("slsc", 1.0, 2), ("cf", 1.0)):
        for form in ("dev", "table"):
            got = image(mi, g, ku.case_data(name, "noise"), 3.0e6, setting, form)
            assert np.all(bits(got)[none & ~g["left_out"]] == 0) and np.all(bits(got)[:8] == 0) and np.all(bits(got)[16:] == 0)
            assert np.any(got[8:16] != 0)


# ---- 3. the scale of the data -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a5_e64_lin_f1_sum", "a5_e65_small_near_f0_sum"])
def test_a_power_of_two_on_the_data(mi, name):
    """SLSC is homogeneous of degree 0 and every row is brought to order 1 by a power of two before it is squared: data times 2^+-70
    (squares beyond the largest float, or subnormal) keep the image's bits.  CF is homogeneous of degree 1 and the aperture is
    rescaled likewise: the image times that power of two, bit for bit."""
    g = geometry(name)
    data = ku.case_data(name, "noise")
    for setting in (("slsc", 0.3, 1), ("slsc", 1.0, 4), ("cf", 1.0), ("cf", 0.5)):
        one = image(mi, g, data, 3.0e6, setting)
        assert np.any(one != 0)
        for k in (-70, 70):
            got = image(mi, g, (data * np.float32(2.0 ** k)).astype(np.complex64), 3.0e6, setting)
            want = one if setting[0] == "slsc" else one * np.float32(2.0 ** k)
            assert np.isfinite(got).all() and np.array_equal(bits(got), bits(want)), (name, setting, k)


# ---- 4. the kernel at the ends of a trace -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t0_samples", [24.0, -56.0], ids=["before_sample_0", "past_the_last_sample"])
def test_the_kernel_at_the_ends_of_a_trace(mi, t0_samples):
    name = "a5_e64_lin_f1_sum"
    g = dict(geometry(name))
    t0 = float(np.float32(t0_samples / g["fs"]))
    g["left_out"], g["n_a"] = nu.margins(g["tx"], g["elem"], g["x"], g["z"], T, g["fs"], C0, t0=t0, f_number=g["kw"]["f_number"],
                                         interpolation=g["kw"]["interpolation"])
    data = ku.case_data(name, "noise")
    setting = ("slsc", 0.3, 4)
    args = (data, g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, 3.0e6)
    ref, B, edge, (before, past) = cu.coherence(*args, t0=t0, **cu.settings_kw(setting), **g["kw"])
    assert (before if t0 > 0 else past) > 0 and (past if t0 > 0 else before) == 0
    used = ~(g["left_out"] | edge) & (B > 0)
    floor = max(compare(cu.coherence(*args, t0=t0, dtype=np.float32, order=o, **cu.settings_kw(setting), **g["kw"])[0], ref, B, used)
                for o in (0, 1))
    got = image(mi, g, data, 3.0e6, setting, t0=t0)
    ratio = compare(got, ref, B, used)
    print(f"\n{name} t0 = {t0_samples:g} samples: {before} pairs with a kernel sample before the trace, {past} past it; float32 floor "
          f"{floor:.2e}, device {ratio:.2e} ({ratio / floor:.2f} x), {int(used.sum())} pixels")
    assert used.mean() > 0.5 and ratio <= 4.0 * floor
    assert np.array_equal(bits(image(mi, g, data, 3.0e6, setting, "table", t0=t0)), bits(got))


# ---- 5. non-finite samples ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "plus_inf"])
@pytest.mark.parametrize("name", ["a5_e64_lin_f1_sum", "a5_e16_convex_lin_f1_sum"])
def test_a_bad_sample_goes_where_the_arithmetic_carries_it(mi, name, value):
    g = geometry(name)
    clean = ku.case_data(name, "noise")
    where, _ = nu.bad_sites(g, T, C0, 3, 17)
    data = np.array(clean, copy=True)
    for a, e, t in where:
        data[a, e, t] = complex(value, float(clean[a, e, t].imag))
    args = (g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, 3.0e6)
    for setting in (("slsc", 0.3, 1), ("cf", 1.0)):
        H = setting[2] if setting[0] == "slsc" else 0
        ref_clean, _, edge, _ = cu.restated(name, "noise", 3.0e6, setting)
        ref_bad = cu.coherence(data, *args, **cu.settings_kw(setting), **g["kw"])[0]
        kept = ~(g["left_out"] | edge | cu.near_bad(g, where, H))
        assert 1.0 - kept.mean() <= 0.03
        got_clean, got = image(mi, g, clean, 3.0e6, setting), image(mi, g, data, 3.0e6, setting)
        assert np.isfinite(got_clean).all()
        changed = nu.classes(ref_bad) != nu.classes(ref_clean)
        assert changed[kept].any()
        assert np.array_equal(nu.classes(got)[kept], nu.classes(ref_bad)[kept]), (name, value, setting)
        same = kept & np.isfinite(ref_bad) & (ref_bad == ref_clean)
        assert same.any() and np.array_equal(bits(got)[same], bits(got_clean)[same]), (name, value, setting)
        assert np.array_equal(bits(image(mi, g, data, 3.0e6, setting, "table")), bits(got))


# ---- 6. non-finite geometry (D25) ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", [("slsc", 0.3, 1), ("cf", 1.0)], ids=["slsc", "cf"])
def test_a_transmission_without_a_first_arrival_adds_nothing(mi, setting):
    name, a_bad = "a5_e64_lin_f1_sum", 2
    g = geometry(name)
    assert g["kw"]["compound"] == "sum" and g["kw"]["interpolation"] == "linear"
    data = ku.case_data(name, "noise")
    others = [a for a in range(g["A"]) if a != a_bad]
    without = image(mi, g, data[others], 3.0e6, setting, tx=g["tx"][others])
    assert np.any(without != 0) and not np.array_equal(without, image(mi, g, data, 3.0e6, setting))
    tx = g["tx"].copy()
    tx[a_bad] = np.nan                                                       # no element gives a first arrival: 1e300, N = 0
    assert np.array_equal(bits(image(mi, g, data, 3.0e6, setting, tx=tx)), bits(without))
    tx = g["tx"].copy()
    tx[a_bad, 7] = -np.inf                                                   # the first arrival is -inf: no position lies in the trace
    assert np.array_equal(bits(image(mi, g, data, 3.0e6, setting, tx=tx)), bits(without))

    def plus_inf(table):
        table[a_bad] = np.inf

    assert np.array_equal(bits(image(mi, g, data, 3.0e6, setting, "table", edit_table=plus_inf)), bits(without))
    # a NaN table entry under linear interpolation: the trace is indexed by the receive part alone with a NaN weight -- a NaN pixel,
    # and no other pixel changes by a bit
    ix, iz = 11, 9
    assert g["n_a"][a_bad, ix, iz] >= 2 and not g["left_out"][ix, iz]

    def one_nan(table):
        table[a_bad, ix, iz] = np.nan

    whole = image(mi, g, data, 3.0e6, setting, "table")
    got = image(mi, g, data, 3.0e6, setting, "table", edit_table=one_nan)
    assert np.all(np.isnan(got[ix, iz]))
    mask = np.ones(got.shape, bool)
    mask[ix, iz] = False
    assert np.array_equal(bits(got)[mask], bits(whole)[mask])


# ---- 7. the point scatterer, through the library -------------------------------------------------------------------------------------
def test_the_point_scatterer_on_the_device(mi):
    for A in (1, 3):
        s = ku.baseband_scatterer(A)
        args = (s["iq"], s["tx"], s["ex"], s["x"], s["z"], s["fs"], s["c"], s["f0"])
        for fn in (0.0, 1.0):
            das = np.abs(mi.iq_beamform(*args, f_number=fn))[:, 1]
            for lag_prop, H in ((0.3, 0), (0.3, 2), (1.0, 1)):
                img = mi.coherence_beamform(*args, kind="slsc", lag_prop=lag_prop, half_kernel=H, f_number=fn)
                B = cu.coherence(*args, kind="slsc", lag_prop=lag_prop, half_kernel=H, f_number=fn)[1]
                k = int(np.argmax(img[:, 1]))
                print(f"\nA={A} f#={fn} lag_prop={lag_prop} H={H}: SLSC at the scatterer / sum_a M = {img[k, 1] / B[k, 1]:.4f}")
                assert k == len(s["x"]) // 2 and img[k, 1] >= 0.99 * B[k, 1], (A, fn, lag_prop, H)
            for gamma, most in ((1.0, 0.75), (2.0, 0.6)):
                cf = np.abs(mi.coherence_beamform(*args, kind="cf", gamma=gamma, f_number=fn))[:, 1]
                ratio, peak = ku.width(cf) / ku.width(das), float(cf.max() / das.max())
                print(f"\nA={A} f#={fn} gamma={gamma}: -6 dB width over delay-and-sum's {ratio:.3f}, peak ratio {peak:.4f}")
                assert ratio < most and abs(peak - 1.0) <= 0.01, (A, fn, gamma, ratio, peak)


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------
def coherence_block(capi, g, kind, f_d=3.0e6, tables=0):
    par = capi.CoherenceParams()
    d, kw = par.scan.das, g["kw"]
    d.n_angles, d.n_elements, d.time_samples = g["A"], g["E"], T
    d.fs, d.sound_speed, d.t0, d.f_number = g["fs"], C0, 0.0, kw["f_number"]
    d.interpolation = {"nearest": capi.DAS_NEAREST, "linear": capi.DAS_LINEAR}[kw["interpolation"]]
    d.compound_mean = {"sum": 0, "mean": 1}[kw["compound"]]
    d.nx, d.nz = len(g["x"]), len(g["z"])
    par.scan.method, par.scan.p, par.scan.demod_freq, par.scan.probe = capi.SCAN_IQ, 2.0, f_d, int(g["elem"].ndim == 2)
    par.tables, par.kind, par.half_kernel, par.lag_prop, par.gamma = tables, kind, (1 if kind == capi.COH_SLSC else 0), 0.3, 1.0
    return par


def raw_call(mi, par, g, data, form="dev", edit=None):
    """pbrt_coherence_beamform[_dev | _table_dev] through ctypes on a block -> (rc, out, the context's error text); out is a buffer of
    nx * nz pairs that starts as 7 in every float"""
    cx = mi.default_context()
    if edit is not None:
        edit(par)
    out = np.full((len(g["x"]), len(g["z"])), 7.0 + 7.0j, np.complex64)
    host = [np.ascontiguousarray(a) for a in (data, g["tx"], g["elem"], g["x"], g["z"])]
    if form == "host":
        rc = cx.lib.pbrt_coherence_beamform(cx.handle, C.byref(par), *(a.ctypes.data for a in host), out.ctypes.data)
    else:
        bufs = [mi.DeviceBuffer.from_host(cx, a) for a in host]
        d_out = mi.DeviceBuffer.from_host(cx, out)
        if form == "table":
            bufs[1] = mi.das_first_arrival(bufs[1], bufs[2], bufs[3], bufs[4], C0)
        name = "pbrt_coherence_beamform_table_dev" if form == "table" else "pbrt_coherence_beamform_dev"
        rc = getattr(cx.lib, name)(cx.handle, C.byref(par), *(b.ptr for b in bufs), d_out.ptr)
        out = d_out.numpy()
    msg = cx.lib.pbrt_last_error(cx.handle)
    return rc, out, (msg.decode() if msg else "")


def test_refusals_on_the_device_library(mi, capi):
    name = "a5_e64_lin_f1_sum"
    g, data = geometry(name), ku.case_data(name, "noise")
    seven = np.complex64(7.0 + 7.0j)
    n = len(g["x"]) * len(g["z"])
    for form in ("dev", "table", "host"):
        rc, out, msg = raw_call(mi, coherence_block(capi, g, capi.COH_SLSC), g, data, form)
        flat = out.view(np.float32).ravel()                                  # an SLSC image is nx * nz floats: the rest stays as it was
        assert rc == 0 and np.all(flat[n:] == 7.0), msg
        assert np.array_equal(bits(flat[:n].reshape(out.shape)), bits(image(mi, g, data, 3.0e6, ("slsc", 0.3, 1))))
        rc, out, msg = raw_call(mi, coherence_block(capi, g, capi.COH_CF), g, data, form)
        assert rc == 0 and np.array_equal(bits(out), bits(image(mi, g, data, 3.0e6, ("cf", 1.0)))), msg
    nan, inf = float("nan"), float("inf")
    S, F = capi.COH_SLSC, capi.COH_CF
    both = [(lambda p, m=m: setattr(p.scan, "method", m), "method") for m in (capi.SCAN_DAS, capi.BF_PDAS, capi.BF_FDMAS, 4)]
    both += [(lambda p: setattr(p, "tables", 2), "tables")]
    both += [(lambda p, k=k: setattr(p, "kind", k), "kind") for k in (0, 3, 0xFFFFFFFF)]
    both += [(lambda p: setattr(p.scan.das, "n_elements", 257), "n_elements <= COH_MAX_E"),
             (lambda p: setattr(p.scan, "probe", 2), "probe"), (lambda p: setattr(p.scan, "demod_freq", -1.0), "demod_freq"),
             (lambda p: setattr(p.scan, "demod_freq", nan), "demod_freq"), (lambda p: setattr(p.scan.das, "n_angles", 0), "n_angles"),
             (lambda p: setattr(p.scan.das, "n_elements", 0), "n_elements"), (lambda p: setattr(p.scan.das, "time_samples", 1), "time_samples"),
             (lambda p: setattr(p.scan.das, "fs", 0.0), "fs"), (lambda p: setattr(p.scan.das, "sound_speed", 0.0), "sound_speed"),
             (lambda p: setattr(p.scan.das, "interpolation", 2), "interpolation"), (lambda p: setattr(p.scan.das, "f_number", -1.0), "f_number"),
             (lambda p: setattr(p.scan.das, "nx", 0), "nx")]
    rules = [(k, e, w) for k in (S, F) for e, w in both]
    rules += [(S, lambda p, v=v: setattr(p, "lag_prop", v), "lag_prop") for v in (0.0, -0.3, 1.5, nan, inf)]
    rules += [(S, lambda p, v=v: setattr(p, "half_kernel", v), "half_kernel") for v in (5, 0xFFFFFFFF)]
    rules += [(F, lambda p, v=v: setattr(p, "gamma", v), "gamma") for v in (-0.5, 4.5, nan, inf)]
    rules += [(F, lambda p, v=v: setattr(p, "half_kernel", v), "half_kernel") for v in (1, 4)]
    for kind, edit, word in rules:
        for form in ("dev", "host") if word not in ("kind", "lag_prop", "gamma", "half_kernel", "tables") else ("dev", "table", "host"):
            rc, out, msg = raw_call(mi, coherence_block(capi, g, kind), g, data, form, edit)
            assert rc == E_INVALID and np.all(out == seven), (kind, word, form, rc)
            assert msg.startswith("invalid argument: ") and word in msg, (kind, word, form, msg)
    rc, out, _ = raw_call(mi, capi.CoherenceParams(), g, data)               # a zeroed block
    assert rc == E_INVALID and np.all(out == seven)
    # the other kind's fields are not read; the ends of the ranges are taken
    for kind, edit in ((S, lambda p: setattr(p, "gamma", nan)), (F, lambda p: setattr(p, "lag_prop", nan)),
                       (S, lambda p: setattr(p, "lag_prop", 1.0)), (S, lambda p: setattr(p, "half_kernel", 4)),
                       (S, lambda p: setattr(p, "half_kernel", 0)), (F, lambda p: setattr(p, "gamma", 4.0)),
                       (F, lambda p: setattr(p, "gamma", 0.0))):
        assert raw_call(mi, coherence_block(capi, g, kind), g, data, "dev", edit)[0] == 0
    mi.default_context().synchronize()


def test_the_limits_of_the_request_run(mi):
    """256 elements, H = 4, 64 lags: the largest dynamic LDS a launch can ask for (72 KB per workgroup) on a scan of one tile"""
    rng = np.random.default_rng(9)
    E, A, nT = 256, 2, 224
    elem = ((np.arange(E) - (E - 1) / 2) * 1.0e-4).astype(np.float32)
    tx = np.zeros((A, E), np.float32)
    x, z = (np.arange(5) * 0.3e-3).astype(np.float32), (2.0e-3 + np.arange(6) * 0.2e-3).astype(np.float32)
    data = (rng.standard_normal((A, E, nT)) + 1j * rng.standard_normal((A, E, nT))).astype(np.complex64)
    kw = dict(f_number=0.0, interpolation="linear", compound="sum")
    got = mi.coherence_beamform(data, tx, elem, x, z, 20.0e6, C0, 3.0e6, kind="slsc", lag_prop=1.0, half_kernel=4, **kw)
    ref, B, edge, _ = cu.coherence(data, tx, elem, x, z, 20.0e6, C0, 3.0e6, kind="slsc", lag_prop=1.0, half_kernel=4, **kw)
    left_out, n_a = nu.margins(tx, elem, x, z, nT, 20.0e6, C0, f_number=0.0, interpolation="linear")
    used = ~(left_out | edge) & (B > 0)
    floor = max(compare(cu.coherence(data, tx, elem, x, z, 20.0e6, C0, 3.0e6, kind="slsc", lag_prop=1.0, half_kernel=4, dtype=np.float32,
                                     order=o, **kw)[0], ref, B, used) for o in (0, 1))
    ratio = compare(got, ref, B, used)
    print(f"\nE = 256, H = 4: N up to {int(n_a.max())}, float32 floor {floor:.2e}, device {ratio:.2e} ({ratio / floor:.2f} x)")
    assert n_a.max() > 128 and used.mean() > 0.9 and ratio <= 4.0 * floor


# ---- 9. the classes and the chains --------------------------------------------------------------------------------------------------
def test_the_classes_hand_the_settings_on(mi):
    name = "a5_e64_lin_f1_sum"
    g, iq = geometry(name), ku.case_data(name, "noise")
    probe = mi.build_probe("linear", g["E"], float(g["elem"][1] - g["elem"][0]), 3.0e6, 70)
    probe.geometry[0] = g["elem"]                      # the case's own positions, bit for bit
    info = {"sampling_freq": g["fs"], "t0": 0, "delays": g["tx"], "sound_speed": C0}
    scan = mi.GridScan(g["x"], g["z"])
    su = dict(f_number=1.0, interpolation="linear", compound="sum")
    args = (g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, 3.0e6)
    polar = mi.PolarScan(np.asarray(g["z"], np.float64)[0] + np.arange(16) * 0.187e-3, np.linspace(-0.3, 0.3, 9))
    px, pz = polar.pixels()
    cases = ((mi.ShortLagSpatialCoherence, dict(lag_prop=0.5, half_kernel=2), dict(kind="slsc", lag_prop=0.5, half_kernel=2),
              ("lag_prop", 0.3), np.float32),
             (mi.CoherenceFactor, dict(gamma=2.0), dict(kind="cf", gamma=2.0), ("gamma", 1.0), np.complex64))
    for cls, setups, kw, (key, other_value), dtype in cases:
        bf = cls(**setups, **su).automatic_setup(info, probe)
        assert bf.is_iq and all(bf.setups[k] == v for k, v in setups.items()) and cls.__name__ in str(bf)
        want = mi.coherence_beamform(iq, *args, **kw, **su)
        assert want.dtype == dtype and np.array_equal(bits(bf.beamform(iq, scan)), bits(want)) and np.any(want != 0)
        on_dev = bf.beamform(mi.DeviceBuffer.from_host(mi.default_context(), iq), scan)
        assert isinstance(on_dev, mi.DeviceBuffer) and on_dev.dtype == dtype and np.array_equal(bits(on_dev.numpy()), bits(want))
        env = bf.compute_envelope(want)
        assert env is want if dtype == np.float32 else np.array_equal(env, mi.iq_envelope(want))
        bf.update_setup(key, other_value)
        other = bf.beamform(iq, scan)
        assert not np.array_equal(other, want) and np.array_equal(bits(other), bits(mi.coherence_beamform(iq, *args, **dict(kw, **{key: other_value}), **su)))
        on_polar = bf.beamform(iq, polar)
        assert on_polar.shape == polar.shape and np.isfinite(on_polar).all() and np.any(on_polar != 0)
        assert np.array_equal(bits(on_polar), bits(mi.coherence_beamform(iq, g["tx"], g["elem"], px, pz, g["fs"], C0, 3.0e6, tables=True,
                                                                           **dict(kw, **{key: other_value}), **su)))
    cf = mi.CoherenceFactor(**su).automatic_setup(info, probe)
    packet = cf.beamform_packet(np.stack([iq, iq * np.complex64(2.0)]), scan)
    assert packet.shape == (2,) + scan.shape and np.array_equal(bits(packet[0]), bits(cf.beamform(iq, scan)))
    assert np.array_equal(bits(packet[1]), bits(packet[0] * np.complex64(2.0)))


def _plate_scan(ui, step, half_x, half_z):
    return dict(x_range=(-(half_x + 0.5) * step, half_x * step), z_range=(0.05 - (half_z + 0.5) * step, 0.05 + half_z * step), step=step)


@pytest.mark.parametrize("kind", ["slsc", "cf"])
def test_us_render_with_a_coherence_beamformer(mi, kind):
    """the plate phantom (tests/scenes/us_plate.xml) with beamformer=ShortLagSpatialCoherence() / CoherenceFactor(): is_iq selects the
    I/Q chain by itself -- rf2iq, the coherence kernel, (CF: the modulus,) log compression -- on a 25 x 65 scan at lambda / 2.  One
    path per ray: the replayed chain is compared bit for bit."""
    sc = mi.load_file(scene_path("us_plate.xml"), paths_per_ray=1, seed=4)
    ui = sc.integrator()
    lam = ui.sound_speed / ui.frequency
    kw = _plate_scan(ui, lam / 2, 12, 32)
    make = mi.ShortLagSpatialCoherence if kind == "slsc" else mi.CoherenceFactor
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
    assert np.isfinite(env).all() and np.isfinite(disp).all() and env.dtype == np.float32
    # the host classes on the channel buffer the device chain used: the same bits, step by step
    plan = ui._render_plan
    chan = np.asarray(ui.channel_buf, np.float32).reshape(ui.n_angles, ui.n_elements, ui.time_samples)
    delays = np.asarray(ui.transmission_delays_buf, np.float32).reshape(ui.n_angles, ui.n_elements)
    probe = mi.build_probe("linear", ui.n_elements, ui.pitch, ui.frequency, 70)
    iq = mi.rf2iq(chan, ui.frequency, ui.fs, decimation=1)
    host_bf = make().automatic_setup({"sampling_freq": ui.fs, "t0": 0, "delays": delays, "sound_speed": ui.sound_speed}, probe)
    scan = mi.GridScan(xs, zs)
    img = host_bf.beamform(iq, scan)
    assert np.array_equal(plan.d_iq.numpy(), iq) and np.any(img != 0)
    if kind == "cf":
        assert np.array_equal(bits(plan.d_bf_iq.numpy()), bits(img))
    assert np.array_equal(bits(np.ascontiguousarray(host_bf.compute_envelope(img), np.float32)), bits(env))
    # a changed setup is a new recording and another image
    bf.update_setup(*(("lag_prop", 1.0) if kind == "slsc" else ("gamma", 2.0)))
    tm = {}
    _, env_other, _ = mi.us_render(sc, beamformer=bf, timing=tm, **kw)
    assert not tm["replayed"] and not np.array_equal(env_other, env)
    # on_device, the host-pointer chain on an acquisition of its own, and a sector
    d_img, d_env, _ = mi.us_render(sc, beamformer=bf, on_device=True, **kw)
    sc.device().ctx.synchronize()
    assert np.array_equal(d_env.numpy(), env_other) and d_img.numpy().T.shape == disp.shape
    d_host, b_host, _ = mi.us_render(sc, beamformer=bf, device_resident=False, **kw)
    assert d_host.shape == disp.shape and np.isfinite(b_host).all() and b_host.max() > 0
    disp, env, (xs, zs) = mi.us_render(sc, beamformer=make(), scan="polar", **kw)
    assert np.isfinite(env).all() and env.max() > 0 and disp.shape == (len(zs), len(xs)) and env.shape == (len(xs), len(zs))
