"""The convex (curved) array of DESIGN.md D18 on the host: the element table and the transmit delays of the library
(pbrt_us_array_elements, pbrt_us_tx_delays: host-only helpers, no device) against the float64 restatement of tests/convex_util.py,
the linear limit of the delays, build_probe('convex'), what Python refuses, and the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import convex_util as cu
from conftest import ROOT

F32 = 2.0 ** -24


def _params(capi, n, radius, opening, angles=(-8.0, 0.0, 8.0), c=1540.0, convex=True):
    p = capi.UsParams()
    p.n_elements, p.n_angles, p.sound_speed, p.pitch = n, len(angles), c, 3e-4
    for i, a in enumerate(angles):
        p.angles_deg[i] = a
    p.primary = capi.US_PRIMARY_ELEMENT | (capi.US_ARRAY_CONVEX if convex else 0)
    p.emitter.number_of_elements, p.emitter.radius, p.emitter.opening_angle = n, radius, opening
    return p


def _elements(capi, p):
    out = np.full((p.n_elements, 4), np.nan, np.float32)
    return capi.load_library().pbrt_us_array_elements(C.byref(p), capi.addr(out)), out


def _delays(capi, p):
    out = np.full((p.n_angles, p.n_elements), np.nan, np.float32)
    return capi.load_library().pbrt_us_tx_delays(C.byref(p), capi.addr(out)), out


@pytest.mark.parametrize("n", [1, 16, 70])
@pytest.mark.parametrize("radius,opening", [(0.04, 40.0), (0.06, 120.0)])
def test_element_table_and_delays_against_float64(capi, n, radius, opening):
    """float32 statements of a handful of operations each: the angle (span, division, fma: 3 roundings of values <= span / 2), sin /
    cos (the polynomial within 1 ulp up to 45 degrees, libm beyond), the product with R -- 8 units of 2^-24 relative to R cover the
    positions, and the same relative to |x_e| + |z_e - R| (plus the sum's own rounding) the delays, which are formed in float64
    from the float32 table"""
    p = _params(capi, n, radius, opening)
    rc, got = _elements(capi, p)
    assert rc == 0
    ref = cu.element_table(n, np.float32(radius), np.float32(opening))
    assert np.abs(got[:, :2] - ref[:, :2]).max() <= 8 * F32 * radius
    assert np.abs(got[:, 2:] - ref[:, 2:]).max() <= 8 * F32
    assert np.allclose(np.hypot(got[:, 2], got[:, 3]), 1.0, atol=4 * F32)
    if n > 1:
        assert np.array_equal(got[:, 0], -got[::-1, 0]) or np.abs(got[:, 0] + got[::-1, 0]).max() <= 8 * F32 * radius
        assert (np.diff(got[:, 0]) > 0).all()
    rc, tx = _delays(capi, p)
    assert rc == 0
    want = cu.tx_delays(ref, float(np.float32(radius)), [-8.0, 0.0, 8.0], 1540.0)
    tol = (16 * F32 * radius + F32 * np.abs(want) * 1540.0) / 1540.0
    assert (np.abs(tx - want) <= tol).all(), float(np.abs(tx - want).max())
    # the apex element of an odd array, or any element at angle 0 on the axis, has no delay beyond the sagitta
    assert (tx[1] <= 0).all()                      # a = 0: (z_e - R) / c <= 0, the apex leads


def test_delays_reach_the_linear_array_at_large_radius(capi):
    """R = 10 m, apex held fixed: tx -> x_e sin(a) / c.  The difference is the sagitta term (z_e - R) cos(a) / c, at most
    R (1 - cos(span / 2)) / c; both sides are float32 tables (2^-24 of their largest value each)"""
    n, pitch, R, c = 16, 3e-4, 10.0, 1540.0
    opening = np.rad2deg((n - 1) * pitch / R)          # arc length of the array = its linear aperture
    angles = (-8.0, 0.0, 8.0)
    rc, tx = _delays(capi, _params(capi, n, R, opening, angles))
    assert rc == 0
    lin = _params(capi, n, 0.0, 0.0, angles, convex=False)
    rc, tl = _delays(capi, lin)
    assert rc == 0
    span = np.deg2rad(opening)
    sagitta = R * (1 - np.cos(span / 2))
    # x_e = R sin(th_e) against the linear th_e R: a relative 1 - sinc(span / 2) <= span^2 / 24; and the float32 rounding of
    # z_e = R cos(th_e) ~ 10 m (2^-24 R = 6e-7 m: the price of referencing the delays to an apex 10 m from the origin)
    bound = (sagitta + np.abs(tl).max() * c * span ** 2 / 24 + 2 * F32 * R) / c + 2 * F32 * np.abs(tl).max()
    assert np.abs(tx - tl).max() <= bound, (float(np.abs(tx - tl).max()), bound)
    assert bound < 1e-9                              # i.e. a twentieth of a 50 MHz sample: the limit is a limit


def test_library_refuses_bad_arrays(capi):
    for radius, opening, n_em in [(0.0, 40.0, 16), (-0.04, 40.0, 16), (np.inf, 40.0, 16), (np.nan, 40.0, 16), (0.04, 0.0, 16),
                                  (0.04, 180.0, 16), (0.04, -10.0, 16), (0.04, np.nan, 16), (0.04, 40.0, 15)]:
        p = _params(capi, 16, radius, opening)
        p.emitter.number_of_elements = n_em
        assert _elements(capi, p)[0] == -1, (radius, opening, n_em)
        assert _delays(capi, p)[0] == -1, (radius, opening, n_em)
    # without the bit the emitter block is not read: the line of elements
    p = _params(capi, 16, np.nan, np.nan, convex=False)
    rc, el = _elements(capi, p)
    assert rc == 0 and np.array_equal(el[:, 1:], np.tile(np.float32([0, 0, 1]), (16, 1)))
    assert np.array_equal(el[:, 0], (np.float64(np.float32(3e-4)) * (np.arange(16) - 7.5)).astype(np.float32))


def test_build_probe_convex(mi):
    probe = mi.build_probe("convex", 16, 3e-4, 5e6, 70, radius=0.04, opening_angle=40.0)
    ref = cu.element_table(16, 0.04, 40.0)
    assert probe.geometry_type == "convex" and probe.geometry.shape == (3, 16) and probe.geometry.dtype == np.float32
    assert np.abs(probe.geometry[0] - ref[:, 0]).max() <= 8 * F32 * 0.04 and np.abs(probe.geometry[2] - ref[:, 1]).max() <= 8 * F32 * 0.04
    assert not probe.geometry[1].any()
    assert np.abs(probe.normals[0] - ref[:, 2]).max() <= 8 * F32 and np.abs(probe.normals[2] - ref[:, 3]).max() <= 8 * F32
    assert probe.das_elements.shape == (16, 4) and probe.pitch == pytest.approx(3e-4)
    lin = mi.build_probe("linear", 16, 3e-4, 5e6, 70)       # unchanged
    assert lin.das_elements.shape == (16,) and not lin.geometry[2].any() and (lin.normals[2] == 1).all()


def test_python_refusals(mi):
    with pytest.raises(NotImplementedError):
        mi.build_probe("convex", 16, 3e-4, 5e6, 70)                                         # by pitch alone: not built
    for radius, opening in [(0.0, 40.0), (-1.0, 40.0), (np.inf, 40.0), (0.04, 0.0), (0.04, 180.0), (0.04, np.nan)]:
        with pytest.raises(ValueError):
            mi.build_probe("convex", 16, 3e-4, 5e6, 70, radius=radius, opening_angle=opening)
    with pytest.raises(ValueError):
        mi.build_probe("linear", 16, 3e-4, 5e6, 70, radius=0.04, opening_angle=40.0)
    with pytest.raises(NotImplementedError):
        mi.build_probe("matrix", 16, 3e-4, 5e6, 70)

    def scene(integ, emitter=None):
        d = {"type": "scene", "integrator": {"type": "ultrasound_integrator", "n_elements": 16, "angles": [0.0], "time_samples": 64, **integ},
             "sensor": {"type": "ultrasound_sensor"}}
        if emitter is not None:
            d["emitter"] = {"type": "ultrasound_emitter", "number_of_elements": 16, **emitter}
        return mi.load_dict(d)

    sc = scene({"radius": 0.04, "opening_angle": 40.0})
    p = sc.integrator().us_params(sc)
    assert p.primary == (mi._capi.US_PRIMARY_ELEMENT | mi._capi.US_ARRAY_CONVEX)
    assert p.emitter.number_of_elements == 16 and p.emitter.radius == np.float32(0.04) and p.emitter.opening_angle == 40.0
    assert scene({}).integrator().us_params(None).primary == mi._capi.US_PRIMARY_ELEMENT        # default: linear, as before
    for bad in ({"radius": 0.04, "opening_angle": 180.0}, {"radius": 0.04}, {"radius": -0.04, "opening_angle": 40.0}):
        sc = scene(bad)
        with pytest.raises(ValueError):
            sc.integrator().us_params(sc)
    # the hole: a curved emitter under a linear integrator; and two different arcs
    sc = scene({"primary_rays": "emitter"}, {"radius": 0.04, "opening_angle": 40.0})
    with pytest.raises(ValueError, match="arc"):
        sc.integrator().us_params(sc)
    sc = scene({"primary_rays": "emitter", "radius": 0.05, "opening_angle": 40.0}, {"radius": 0.04, "opening_angle": 40.0})
    with pytest.raises(ValueError):
        sc.integrator().us_params(sc)
    sc = scene({"primary_rays": "emitter", "radius": 0.04, "opening_angle": 40.0}, {"radius": 0.04, "opening_angle": 40.0})
    assert sc.integrator().us_params(sc).primary == (mi._capi.US_PRIMARY_EMITTER | mi._capi.US_ARRAY_CONVEX)
    # radius and opening angle are scene parameters
    params = mi.traverse(sc)
    assert "integrator.radius" in params and "integrator.opening_angle" in params
    params["integrator.opening_angle"] = 30.0
    params["emitter.opening_angle"] = 30.0
    params.update()
    assert sc.integrator().us_params(sc).emitter.opening_angle == 30.0


def test_header_declares_the_switch_and_keeps_the_abi():
    with open(os.path.join(ROOT, "include", "pbrt_hip.h")) as f:
        h = f.read()
    assert re.search(r"^#define PBRT_US_ARRAY_CONVEX 0x100u$", h, re.M)
    assert re.search(r"^#define PBRT_ABI_VERSION 5$", h, re.M)
    for name in ("pbrt_us_array_elements", "pbrt_das_beamform_probe", "pbrt_das_beamform_probe_dev", "pbrt_das_first_arrival_probe_dev",
                 "pbrt_das_beamform_table_probe_dev"):
        assert re.search(rf"^int {name}\(", h, re.M), name
