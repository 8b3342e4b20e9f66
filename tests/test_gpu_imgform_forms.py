"""One beamform request, whichever entry point carries it: for delay-and-sum, p-DAS (p = 3), F-DMAS and I/Q delay-and-sum, with element
positions and with an element table, the host form, the _dev form and the _table_dev form of the entry points on axes
(pbrt_das_beamform* / pbrt_bf_beamform* / pbrt_iq_beamform*) and the same three forms of pbrt_scan_* on np.meshgrid(x, z, indexing="ij")
give one image, bit for bit; das_first_arrival and scan_first_arrival give one table.  (Which entry point each Python call reaches is
tests/test_beamform_dispatch.py; parity of the arithmetic with the float64 restatements is tests/test_gpu_{beamform,nlbf,iq,scan}.py.)

Two shapes, tiles of 8 x 8 pixels: A = 2, E = 3, T = 16 on 5 x 7 pixels (one partial tile), and A = 6, E = 5, T = 40 on 9 x 17 pixels
(two trips of DAS_ANG = 5 angles, 2 x 3 tiles with partial edges).  Seeded random samples; the pixels lie 1 - 1.6 mm deep, so that every
delayed sample (two-way time 1.3 - 2.3 us) falls inside the trace.

One refusal per parameter block goes through the library itself (rc = PBRT_E_INVALID), and the context beamforms the same bits after."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C0, F_D = 1540.0, 2.0e6
SHAPES = {"one_partial_tile": (2, 3, 16, 5, 7, 5.0e6), "two_trips_six_tiles": (6, 5, 40, 9, 17, 12.0e6)}
METHODS = ("das", "pdas", "fdmas", "iq")
KW = dict(t0=0.0, f_number=0.5, interpolation="linear", compound="sum")


def geometry(shape, probe):
    A, E, T, nx, nz, fs = SHAPES[shape]
    rng = np.random.default_rng(1234 + A)
    ex = (3e-4 * (np.arange(E) - (E - 1) / 2)).astype(np.float32)
    elem = np.stack([ex, np.zeros(E), np.zeros(E), np.ones(E)], axis=1).astype(np.float32) if probe else ex
    x = np.linspace(-5e-4, 5e-4, nx).astype(np.float32)
    z = np.linspace(1.0e-3, 1.6e-3, nz).astype(np.float32)
    # the latest delayed sample: first arrival <= 1e-7 + |pixel - nearest element| / c, receive path <= |pixel - farthest element| / c
    far = np.hypot(5e-4 + 6e-4, 1.6e-3)
    assert (1e-7 + 2.0 * far / C0) * fs < T - 1
    return dict(A=A, E=E, T=T, fs=fs, elem=elem, x=x, z=z, tx=rng.uniform(0.0, 1e-7, (A, E)).astype(np.float32),
                rf=rng.standard_normal((A, E, T)).astype(np.float32),
                iq=(rng.standard_normal((A, E, T)) + 1j * rng.standard_normal((A, E, T))).astype(np.complex64))


def on_axes(mi, g, data, method, table=None):
    args = (g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0)
    if method == "das":
        return mi.das_beamform(data, *args, table=table, **KW)
    if method == "iq":
        return mi.iq_beamform(data, *args, F_D, table=table, **KW)
    return mi.nonlinear_beamform(data, *args, method=method, p=3.0, table=table, **KW)


def on_tables(mi, g, data, method, px, pz, table=None):
    return mi.scan_beamform(data, g["tx"], g["elem"], px, pz, g["fs"], C0, method=method, p=3.0, demod_freq=F_D if method == "iq" else None,
                            table=table, **KW)


@pytest.mark.parametrize("probe", (False, True), ids=("positions", "element_table"))
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_form_gives_one_image(mi, shape, method, probe):
    g = geometry(shape, probe)
    cx = mi.default_context()
    data = g["iq"] if method == "iq" else g["rf"]
    px, pz = np.meshgrid(g["x"], g["z"], indexing="ij")
    want = on_axes(mi, g, data, method)
    assert want.shape == px.shape and want.dtype == data.dtype and np.all(np.isfinite(want)) and np.all(want != 0)
    d_data = mi.DeviceBuffer.from_host(cx, data)
    t_axes = mi.das_first_arrival(g["tx"], g["elem"], g["x"], g["z"], C0)
    t_tabs = mi.scan_first_arrival(g["tx"], g["elem"], px, pz, C0)
    first = t_axes.numpy()
    assert first.shape == (g["A"],) + px.shape and np.all(first > 0) and np.array_equal(t_tabs.numpy(), first)
    forms = {"axes _dev": on_axes(mi, g, d_data, method).numpy(),
             "axes _table_dev": on_axes(mi, g, d_data, method, table=t_axes).numpy(),
             "tables host": on_tables(mi, g, data, method, px, pz),
             "tables _dev": on_tables(mi, g, d_data, method, px, pz).numpy(),
             "tables _table_dev": on_tables(mi, g, d_data, method, px, pz, table=t_tabs).numpy()}
    for form, got in forms.items():
        assert got.dtype == want.dtype and np.array_equal(got, want), (shape, method, probe, form)


def test_one_refusal_per_parameter_block_and_the_context_goes_on(mi, capi):
    g = geometry("one_partial_tile", False)
    cx = mi.default_context()
    want = on_axes(mi, g, g["rf"], "das")
    nx, nz = len(g["x"]), len(g["z"])
    px, pz = np.meshgrid(g["x"], g["z"], indexing="ij")
    out, out_c = np.empty((nx, nz), np.float32), np.empty((nx, nz), np.complex64)

    def das(**kw):
        p = capi.DasParams()
        p.n_angles, p.n_elements, p.time_samples, p.fs, p.sound_speed, p.f_number = g["A"], g["E"], g["T"], g["fs"], C0, 0.5
        p.interpolation, p.nx, p.nz = capi.DAS_LINEAR, nx, nz
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(name, block, data, gx, gz, res):
        return getattr(cx.lib, name)(cx.handle, C.byref(block), capi.addr(data), capi.addr(g["tx"]), capi.addr(g["elem"]), capi.addr(gx),
                                     capi.addr(gz), capi.addr(res))

    bp = capi.BfParams()
    bp.das, bp.method, bp.p = das(), capi.BF_PDAS, 9.0
    ip = capi.IqParams()
    ip.das, ip.demod_freq = das(), -1.0
    sp = capi.ScanParams()
    sp.das, sp.method, sp.p = das(), 4, 2.0
    E_INVALID = -1
    assert call("pbrt_bf_beamform", bp, g["rf"], g["x"], g["z"], out) == E_INVALID
    assert b"invalid argument" in cx.lib.pbrt_last_error(cx.handle)
    assert call("pbrt_iq_beamform", ip, g["iq"], g["x"], g["z"], out_c) == E_INVALID
    assert call("pbrt_scan_beamform", sp, g["rf"], px, pz, out) == E_INVALID
    assert call("pbrt_das_beamform", das(interpolation=2), g["rf"], g["x"], g["z"], out) == E_INVALID
    # the blocks were refused for that one field: mended, each is taken
    bp.p, ip.demod_freq, sp.method = 3.0, F_D, capi.SCAN_DAS
    assert call("pbrt_bf_beamform", bp, g["rf"], g["x"], g["z"], out) == 0
    assert np.array_equal(out, on_axes(mi, g, g["rf"], "pdas"))
    assert call("pbrt_iq_beamform", ip, g["iq"], g["x"], g["z"], out_c) == 0
    assert np.array_equal(out_c, on_axes(mi, g, g["iq"], "iq"))
    assert call("pbrt_scan_beamform", sp, g["rf"], px, pz, out) == 0
    assert np.array_equal(out, want)
    assert call("pbrt_das_beamform", das(), g["rf"], g["x"], g["z"], out) == 0
    assert np.array_equal(out, want)
