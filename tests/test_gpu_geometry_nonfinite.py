"""Non-finite and out-of-range GEOMETRY through every beamformer on the device (include/pbrt_hip.h "non-finite and out-of-range
geometry"): NaN, infinities and positions beyond 2^31 samples in the transmit delays, the element positions or
element table, the pixel axes or pixel tables, and a caller's first-arrival table.  test_geometry_rule_restatement.py is the CPU half:
its index model and its conditions pass before any of this runs.

The shapes are walk_cases' smallest with a partial tile, a second and third block of elements, a second trip of angles, both
interpolations, both f-number arms and both probes (117 to 384 pixels, traces of 160 samples).  Every family runs in the forms dev,
table (the library makes the first-arrival table from the same poisoned tables) and host, and the three must agree bit for bit.

V1 late delays, V2 a silent transmission and V4 an absent element are clean problems under the rule (geom_util.stand_in): the device is
held to the float64 restatement of the stand-in with the bound of the family's own test, 4 x the restatement's float32 floor on the
stand-in (D19, D20, D23; with a receive window + 4 * 2^-24 for the weights, D22 -- printed, and the plain 4 x floor is asserted, which
the windows meet too).  Each case prints its floor and the device's ratio before it asserts; DESIGN.md D25 records them."""
import numpy as np
import pytest

import geom_util as gu
from walk_cases import C0, geometry

pytestmark = pytest.mark.gpu

CASES = [(name, family) for name in gu.NAMES + (gu.BIG,) for family in gu.families_of(name)]
STAND_INS = [(name, family, variant) for name, family in CASES
             for variant in ("V1", "V2", "V4") + (("V4n",) if geometry(name)["elem"].ndim == 2 else ())]
_CLEAN = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(a.shape + ((2,) if a.dtype.kind == "c" else ()))


def nan_everywhere(v):
    """NaN in every component"""
    v = np.asarray(v)
    return bool(np.all(np.isnan(v.real)) and (v.dtype.kind != "c" or np.all(np.isnan(v.imag))))


def image(mi, family, p, data, form="dev", tables=None, table=None, t0=0.0):
    """the library's image of a family through the Python layer: form 'dev', 'table' or 'host'; tables: (px, pz) pixel tables instead
    of the axes of p; table: a first-arrival table to use instead of the one the library makes of p's tables"""
    method, pw, window, capon = gu.FAMILIES[family]
    gx, gz = tables if tables is not None else (p["x"], p["z"])
    tab = tables is not None
    kw = dict(p["kw"], t0=t0)
    if form != "host":
        data = mi.DeviceBuffer.from_host(mi.default_context(), np.ascontiguousarray(data))
        if form == "table":
            first = mi.scan_first_arrival if tab else mi.das_first_arrival
            kw["table"] = table if table is not None else first(p["tx"], p["elem"], gx, gz, C0)
    args = (data, p["tx"], p["elem"], gx, gz, p["fs"], C0)
    if capon is not None:
        out = mi.capon_beamform(*args, gu.F_D, l_prop=capon[0], delta_l=capon[1], tables=tab, **kw)
    else:
        kw["rx_apodization"] = window
        if tab:
            out = mi.scan_beamform(*args, method=method, p=pw, demod_freq=gu.F_D if method == "iq" else None, **kw)
        elif method == "das":
            out = mi.das_beamform(*args, **kw)
        elif method == "iq":
            out = mi.iq_beamform(*args, gu.F_D, **kw)
        else:
            out = mi.nonlinear_beamform(*args, method=method, p=pw, **kw)
    return out if form == "host" else out.numpy()


def every_form(mi, family, p, data, **kw):
    """the image in the form dev, after the forms table and host gave its bits"""
    got = image(mi, family, p, data, "dev", **kw)
    for form in ("table", "host"):
        assert np.array_equal(bits(image(mi, family, p, data, form, **kw)), bits(got)), (family, form)
    return got


def clean_image(mi, name, family):
    if (name, family) not in _CLEAN:
        _CLEAN[name, family] = every_form(mi, family, geometry(name), gu.case_data(name, family))
    return _CLEAN[name, family]


def still_clean(mi, name, family):
    """a clean call on the same context afterwards gives the clean bits"""
    again = image(mi, family, geometry(name), gu.case_data(name, family))
    assert np.array_equal(bits(again), bits(clean_image(mi, name, family))), (name, family)


def ratio_of(got, ref, B, used):
    return float((np.abs(got.astype(ref.dtype) - ref)[used] / B[used]).max())


# ---- V1, V2, V4: clean problems under the rule ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,family,variant", STAND_INS)
def test_late_delays_silent_transmissions_and_absent_elements(mi, name, family, variant):
    g = geometry(name)
    data = gu.case_data(name, family)
    clean = clean_image(mi, name, family)
    p, ref, B, used, floor = gu.restated(name, family, variant)
    copies = {label: every_form(mi, family, bad, data) for label, bad in gu.poisoned(variant, g).items()}
    label, got = next(iter(copies.items()))
    ratio = ratio_of(got, ref, B, used)
    print(f"\n{name} {family} {variant} {label}: float32 floor {floor:.3e}, device {ratio:.3e} ({ratio / floor:.2f} x; the family's bound "
          f"{gu.bound(family, floor) / floor:.2f} x), {int(used.sum())} pixels, {int(p['left_out'].sum())} left out")
    unused = (p["n_a"].sum(axis=0) == 0) & ~p["left_out"]
    assert used.any() and np.all(bits(got)[unused] == 0), (name, family, variant)       # a pixel that uses no element is exactly (+0)
    assert ratio <= 4.0 * floor, (name, family, variant, ratio, floor)
    for other, img in copies.items():                                                  # NaN, +inf and -inf: one image
        assert np.array_equal(bits(img), bits(got)), (name, family, variant, other)
    if variant in ("V1", "V2"):                                                        # ... and the 1e30 of the stand-in gives it too
        assert np.array_equal(bits(image(mi, family, p, data)), bits(got)), (name, family, variant)
    if variant == "V4n" and not g["kw"]["f_number"] > 0:
        assert np.array_equal(bits(got), bits(clean))                                  # (no f-number: the normals are not read)
    else:
        assert not np.array_equal(bits(got), bits(clean)), (name, family, variant)
    still_clean(mi, name, family)


# ---- V3: a first arrival of -inf ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,family", CASES)
def test_an_early_delay(mi, name, family):
    """tx[1, 3] = -inf makes the first arrival of transmission 1 -inf at every pixel.  Delay-and-sum, p-DAS, F-DMAS and Capon add nothing
    for it (V2's bits).  The I/Q walk turns the transmission's sum by rot_a = exp(2 pi i frac(f_d * -inf)) = NaN, zero sum or not: NaN in
    both components at every pixel of every 8 x 8 tile that is walked (one of its pixels sees the line of elements; an element table:
    every tile), exact zeros in the tiles that are left early"""
    g = geometry(name)
    data = gu.case_data(name, family)
    got = every_form(mi, family, gu.poisoned("V3", g)["-inf"], data)
    if family in gu.IQ_WALK:
        w = gu.walked(g)
        assert w.any() and nan_everywhere(got[w]) and np.all(bits(got)[~w] == 0), (name, family)
    else:
        silent = image(mi, family, gu.poisoned("V2", g)["nan"], data)
        assert np.array_equal(bits(got), bits(silent)), (name, family)
        assert np.isfinite(got).all() and not np.array_equal(bits(got), bits(clean_image(mi, name, family)))
    still_clean(mi, name, family)


# ---- V5: bad pixels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,family", CASES)
def test_bad_pixels_are_zero_and_touch_no_other(mi, name, family):
    g = geometry(name)
    data = gu.case_data(name, family)
    clean = clean_image(mi, name, family)
    got = every_form(mi, family, gu.poisoned("V5", g)["axes"], data)
    bad = np.zeros(clean.shape, bool)
    bad[2, :] = bad[:, 5] = True
    assert np.all(bits(got)[bad] == 0), (name, family, "axes")                          # exactly (+0)
    assert np.array_equal(bits(got)[~bad], bits(clean)[~bad]) and np.any(clean[bad] != 0), (name, family, "axes")
    px, pz, bad = gu.bad_pixel_tables(g)
    got = every_form(mi, family, g, data, tables=(px, pz))
    assert np.all(bits(got)[bad] == 0), (name, family, "tables")
    assert np.array_equal(bits(got)[~bad], bits(clean)[~bad]) and np.any(clean[bad] != 0), (name, family, "tables")
    still_clean(mi, name, family)


# ---- V6: entries of a caller's first-arrival table ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,family", CASES)
def test_table_entries(mi, name, family):
    """NaN, +inf and -inf in ttx[1] at three pixels of different tiles.  The I/Q walk: NaN (rot_a).  Otherwise nearest interpolation
    takes nothing for the transmission, and so does linear interpolation for an infinity -- the pixel is the silent transmission's (V2)
    -- while under a NaN entry linear interpolation reads an in-range sample with a NaN weight: a NaN pixel"""
    g = geometry(name)
    data = gu.case_data(name, family)
    clean = clean_image(mi, name, family)
    cx = mi.default_context()
    tab = mi.das_first_arrival(g["tx"], g["elem"], g["x"], g["z"], C0).numpy()
    sites = gu.table_sites(name)
    values = (np.nan, np.inf, -np.inf)
    for (ix, iz), v in zip(sites, values):
        assert np.isfinite(tab[gu.SITE_A, ix, iz])
        tab[gu.SITE_A, ix, iz] = v
    got = image(mi, family, g, data, "table", table=mi.DeviceBuffer.from_host(cx, tab))
    other = np.ones(clean.shape, bool)
    for ix, iz in sites:
        other[ix, iz] = False
    assert np.array_equal(bits(got)[other], bits(clean)[other]), (name, family)
    _, ref, B, used, floor = gu.restated(name, family, "V2")
    linear = g["kw"]["interpolation"] == "linear"
    for (ix, iz), v in zip(sites, values):
        if family in gu.IQ_WALK or (linear and np.isnan(v)):
            assert nan_everywhere(got[ix, iz]), (name, family, v, got[ix, iz])
        else:
            ratio = abs(complex(got[ix, iz]) - complex(ref[ix, iz])) / B[ix, iz]
            print(f"\n{name} {family} entry {v}: the pixel against the silent transmission's, {ratio:.3e} (floor {floor:.3e})")
            assert used[ix, iz] and ratio <= 4.0 * floor, (name, family, v, ratio, floor)
            assert got[ix, iz] != clean[ix, iz]
    still_clean(mi, name, family)


# ---- V7: every position beyond 2^31 samples ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,family", CASES)
def test_a_time_origin_200_seconds_back(mi, name, family):
    got = every_form(mi, family, geometry(name), gu.case_data(name, family), t0=-200.0)
    assert np.isfinite(got).all() and np.all(bits(got) == 0), (name, family)
    still_clean(mi, name, family)
