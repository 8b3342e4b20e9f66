"""What the Python image-formation layer (beamform.py) hands to the library, without a GPU: a recording stand-in for libpbrt_hip.so
sits behind a stand-in context in _capi._default_ctx, and every public call is held to the entry point it reaches, the type and the
fields of its parameter block, the buffers in its pointer slots (their contents: uploads and host arrays are copied as they pass),
the shape and dtype of its result and the members of `_keep`.

Covered: das_beamform / nonlinear_beamform / iq_beamform on axes and scan_beamform on pixel tables (host and DeviceBuffer data,
elements [E] and [E, 4], with and without a first-arrival table), the two first-arrival functions, DelayAndSum (RF and I/Q),
PDelayAndSum and FilteredDelayMultiplyAndSum on a GridScan and a PolarScan (the sequence kernel, band-pass), and the seven step
wrappers.  (DelayAndSum has no `band` setup: its cases have no band-pass.)  Shapes: A = 2, E = 3, T = 16, 5 x 7 pixels.
us_render, which drives these calls from a render plan, is held the same way in test_us_render_dispatch.py; the stand-in itself is
dispatch_util.py."""
import importlib
import itertools

import numpy as np
import pytest

from dispatch_util import capi, cx, dev, fields, held  # noqa: F401  (cx is the fixture)

bf = importlib.import_module("physics-based-ray-tracing_amd.beamform")

A, E, T, NX, NZ = 2, 3, 16, 5, 7
FS, C0, T0, FD = 20e6, 1540.0, 1e-6, 2.5e6
KW = dict(t0=T0, f_number=1.5, interpolation="nearest", compound="mean")
RNG = np.random.default_rng(7)
RF = RNG.standard_normal((A, E, T)).astype(np.float32)
IQ = (RNG.standard_normal((A, E, T)) + 1j * RNG.standard_normal((A, E, T))).astype(np.complex64)
TX = RNG.uniform(0.0, 1e-7, (A, E)).astype(np.float32)
EX = np.array([-1e-4, 0.0, 1e-4], np.float32)
ETAB = np.stack([EX, np.zeros(E), np.zeros(E), np.ones(E)], axis=1).astype(np.float32)
X = np.linspace(-2e-4, 2e-4, NX).astype(np.float32)
Z = (1e-3 + 1e-4 * np.arange(NZ)).astype(np.float32)
PX, PZ = np.meshgrid(X, Z, indexing="ij")


def das_fields(nx=NX, nz=NZ):
    return dict(n_angles=A, n_elements=E, time_samples=T, fs=np.float32(FS), sound_speed=np.float32(C0), t0=np.float32(T0),
                f_number=np.float32(1.5), interpolation=capi.DAS_NEAREST, compound_mean=1, nx=nx, nz=nz)


def held(cx, buf, want):
    """the DeviceBuffer `buf` was uploaded from `want` (same bytes, shape and dtype)"""
    want = np.ascontiguousarray(want)
    return buf.shape == want.shape and buf.dtype == want.dtype and cx.lib.mem[buf.ptr] == want.tobytes()


METHODS = {"das": (None, 0, 0.0), "pdas": (3.0, capi.BF_PDAS, 3.0), "fdmas": (2.0, capi.BF_FDMAS, 2.0), "iq": (None, capi.SCAN_IQ, 2.0)}
CASES = [(m, d, pr, tb, ax) for m, d, pr, tb, ax in itertools.product(METHODS, (False, True), (False, True), (False, True), (True, False))
         if d or not tb]


@pytest.mark.parametrize("method,on_dev,probe,with_table,axes", CASES)
def test_a_beamform_call_reaches_its_entry_point(cx, method, on_dev, probe, with_table, axes):
    iq = method == "iq"
    data, elem = (IQ if iq else RF), (ETAB if probe else EX)
    gx, gz = (X, Z) if axes else (PX, PZ)
    table = capi.DeviceBuffer(cx, (A, NX, NZ), np.float64) if with_table else None
    out = capi.DeviceBuffer(cx, (NX, NZ), data.dtype) if on_dev and probe else None     # (`out` given in half of the device cases)
    arg = dev(cx, data) if on_dev else data
    kw = dict(KW, out=out, table=table)
    p = METHODS[method][0]
    if not axes:
        stem, typ = "pbrt_scan_beamform", capi.ScanParams
        res = bf.scan_beamform(arg, TX, elem, gx, gz, FS, C0, method=method, demod_freq=FD if iq else None, **dict(kw, **({"p": p} if p else {})))
        want = dict(das_fields(), method=METHODS[method][1], p=np.float32(p or 2.0), demod_freq=np.float32(FD if iq else 0.0), probe=int(probe))
    elif method == "das":
        stem, typ = "pbrt_das_beamform", capi.DasParams
        res = bf.das_beamform(arg, TX, elem, gx, gz, FS, C0, **kw)
        want = das_fields()
    elif iq:
        stem, typ = "pbrt_iq_beamform", capi.IqParams
        res = bf.iq_beamform(arg, TX, elem, gx, gz, FS, C0, FD, **kw)
        want = dict(das_fields(), demod_freq=np.float32(FD), probe=int(probe))
    else:
        stem, typ = "pbrt_bf_beamform", capi.BfParams
        res = bf.nonlinear_beamform(arg, TX, elem, gx, gz, FS, C0, method=method, p=p, **kw)
        want = dict(das_fields(), method=METHODS[method][1], p=np.float32(p), probe=int(probe))
    name = stem + ("_table" if with_table else "") + ("_probe" if probe and typ is capi.DasParams else "") + ("_dev" if on_dev else "")
    if not on_dev:
        # the host form reads its arrays during the call: run it again with the sizes of its pointer arguments named
        cx.lib.calls.clear()
        cx.lib.peek[name] = {0: data.nbytes, 1: TX.nbytes, 2: elem.nbytes, 3: gx.size * 4, 4: gz.size * 4}
        fn = {"pbrt_scan_beamform": lambda: bf.scan_beamform(data, TX, elem, gx, gz, FS, C0, method=method, p=p or 2.0,
                                                             demod_freq=FD if iq else None, **KW),
              "pbrt_das_beamform": lambda: bf.das_beamform(data, TX, elem, gx, gz, FS, C0, **KW),
              "pbrt_iq_beamform": lambda: bf.iq_beamform(data, TX, elem, gx, gz, FS, C0, FD, **KW),
              "pbrt_bf_beamform": lambda: bf.nonlinear_beamform(data, TX, elem, gx, gz, FS, C0, method=method, p=p, **KW)}[stem]
        res = fn()
    assert [c[0] for c in cx.lib.calls] == [name]
    call = cx.lib.calls[0]
    assert call[1] is typ and fields(call) == want
    assert res.shape == (NX, NZ) and res.dtype == data.dtype
    ptrs = call[3]
    assert len(ptrs) == 6
    if not on_dev:
        assert isinstance(res, np.ndarray) and ptrs[5] == res.ctypes.data
        assert [call[4][i] for i in range(5)] == [a.tobytes() for a in (data, TX, elem, gx, gz)]
        return
    assert isinstance(res, capi.DeviceBuffer) and (res is out if out is not None else True) and ptrs[5] == res.ptr
    d_tx, d_ex, d_x, d_z, kept = res._keep
    assert kept is table
    assert held(cx, d_tx, TX) and held(cx, d_ex, elem) and held(cx, d_x, gx) and held(cx, d_z, gz)
    assert ptrs == [arg.ptr, (table if with_table else d_tx).ptr, d_ex.ptr, d_x.ptr, d_z.ptr, res.ptr]


def test_buffers_that_are_in_hbm_already_are_handed_on(cx):
    d = [dev(cx, a) for a in (RF, TX, ETAB, X, Z, PX, PZ)]
    res = bf.das_beamform(d[0], d[1], d[2], d[3], d[4], FS, C0, **KW)
    assert res._keep == (d[1], d[2], d[3], d[4], None) and cx.lib.calls[-1][0] == "pbrt_das_beamform_probe_dev"
    res = bf.scan_beamform(d[0], d[1], d[2], d[5], d[6], FS, C0, **KW)
    assert res._keep == (d[1], d[2], d[5], d[6], None) and cx.lib.calls[-1][0] == "pbrt_scan_beamform_dev"
    tab = bf.das_first_arrival(d[1], d[2], d[3], d[4], C0)
    assert tab._keep == (d[1], d[2], d[3], d[4])
    tab = bf.scan_first_arrival(d[1], d[2], d[5], d[6], C0)
    assert tab._keep == (d[1], d[2], d[5], d[6])


@pytest.mark.parametrize("probe", (False, True))
@pytest.mark.parametrize("axes", (True, False))
def test_a_first_arrival_call_reaches_its_entry_point(cx, probe, axes):
    elem = ETAB if probe else EX
    gx, gz = (X, Z) if axes else (PX, PZ)
    first = dict(n_angles=A, n_elements=E, time_samples=2, fs=1.0, sound_speed=np.float32(C0), t0=0.0, f_number=0.0,
                 interpolation=capi.DAS_LINEAR, compound_mean=0, nx=NX, nz=NZ)
    if axes:
        tab = bf.das_first_arrival(TX, elem, gx, gz, C0)
        name, typ, want = "pbrt_das_first_arrival" + ("_probe" if probe else "") + "_dev", capi.DasParams, first
    else:
        tab = bf.scan_first_arrival(TX, elem, gx, gz, C0)
        name, typ, want = "pbrt_scan_first_arrival_dev", capi.ScanParams, dict(first, method=0, p=2.0, demod_freq=0.0, probe=int(probe))
    assert [c[0] for c in cx.lib.calls] == [name]
    call = cx.lib.calls[0]
    assert call[1] is typ and fields(call) == want
    assert isinstance(tab, capi.DeviceBuffer) and tab.shape == (A, NX, NZ) and tab.dtype == np.float64
    d_tx, d_ex, d_x, d_z = tab._keep
    assert held(cx, d_tx, TX) and held(cx, d_ex, elem) and held(cx, d_x, gx) and held(cx, d_z, gz)
    assert call[3] == [d_tx.ptr, d_ex.ptr, d_x.ptr, d_z.ptr, tab.ptr]
    out = capi.DeviceBuffer(cx, (A, NX, NZ), np.float64)
    assert (bf.das_first_arrival if axes else bf.scan_first_arrival)(TX, elem, gx, gz, C0, out=out) is out
    with pytest.raises(ValueError, match="out must hold n_angles \\* n[x0] \\* n[z1] float64"):
        (bf.das_first_arrival if axes else bf.scan_first_arrival)(TX, elem, gx, gz, C0, out=capi.DeviceBuffer(cx, (A, NX, NZ)))


def test_the_dispatcher_keeps_its_refusals(cx):
    d_rf, d_iq = dev(cx, RF), dev(cx, IQ)
    small, small_c = capi.DeviceBuffer(cx, (NX, NZ - 1)), capi.DeviceBuffer(cx, (NX, NZ - 1), np.complex64)
    with pytest.raises(ValueError, match="out must hold nx \\* nz float32"):
        bf.das_beamform(d_rf, TX, EX, X, Z, FS, C0, out=small)
    with pytest.raises(ValueError, match="out must hold nx \\* nz complex64"):
        bf.iq_beamform(d_iq, TX, EX, X, Z, FS, C0, FD, out=small_c)
    with pytest.raises(ValueError, match="out must hold n0 \\* n1 float32"):
        bf.scan_beamform(d_rf, TX, EX, PX, PZ, FS, C0, method="fdmas", out=small)
    with pytest.raises(ValueError, match="table must be the \\[n_angles, nx, nz\\] float64 buffer of das_first_arrival"):
        bf.nonlinear_beamform(d_rf, TX, EX, X, Z, FS, C0, table=small)
    with pytest.raises(ValueError, match="table must be the \\[n_angles, n0, n1\\] float64 buffer of scan_first_arrival"):
        bf.scan_beamform(d_rf, TX, EX, PX, PZ, FS, C0, table=small)
    with pytest.raises(ValueError, match="float32 \\(RF\\), got a complex64 DeviceBuffer"):
        bf.das_beamform(d_iq, TX, EX, X, Z, FS, C0)
    with pytest.raises(ValueError, match="complex64 \\(I/Q\\), got a float32 DeviceBuffer"):
        bf.scan_beamform(d_rf, TX, EX, PX, PZ, FS, C0, method="iq", demod_freq=FD)
    with pytest.raises(ValueError, match="data must be \\[n_angles, n_elements, time_samples\\]"):
        bf.das_beamform(RF[0], TX, EX, X, Z, FS, C0)
    with pytest.raises(ValueError, match="element positions must be \\[3\\] or an element table \\[3, 4\\], got \\[2\\]"):
        bf.scan_beamform(RF, TX, EX[:2], PX, PZ, FS, C0)
    with pytest.raises(ValueError, match="one shape"):
        bf.scan_beamform(RF, TX, EX, PX, PZ[:, :3], FS, C0)
    with pytest.raises(ValueError, match="px and pz must both be host arrays or both DeviceBuffers"):
        bf.scan_first_arrival(TX, EX, dev(cx, PX), PZ, C0)
    with pytest.raises(ValueError, match="method must be 'pdas' or 'fdmas'"):
        bf.nonlinear_beamform(RF, TX, EX, X, Z, FS, C0, method="das")
    with pytest.raises(ValueError, match="method must be one of"):
        bf.scan_beamform(RF, TX, EX, PX, PZ, FS, C0, method="bmode")
    with pytest.raises(ValueError, match="demod_freq must be finite and >= 0, got None"):
        bf.scan_beamform(IQ, TX, EX, PX, PZ, FS, C0, method="iq")
    with pytest.raises(ValueError, match="demod_freq must be finite and >= 0, got -1.0"):
        bf.iq_beamform(IQ, TX, EX, X, Z, FS, C0, -1.0)
    assert [c[0] for c in cx.lib.calls] == []


# ---- the ultraspy-shaped classes ---------------------------------------------------------------------------------------------------
BAND, K_TAPS = (1e6, 2e6), 4     # below the axial Nyquist frequency c / (4 dz) = 3.85 MHz of the 1e-4 m depth step
RHOS, THETAS = 1e-3 + 1e-4 * np.arange(NZ), np.linspace(-0.3, 0.3, NX)


def _beamformer(kind, band):
    nl = dict(band=band, taps_half_length=K_TAPS)
    b = {"das": lambda: bf.DelayAndSum(f_number=1.5, interpolation="nearest", compound="mean"),
         "iq": lambda: bf.DelayAndSum(f_number=1.5, interpolation="nearest", compound="mean", is_iq=True),
         "pdas": lambda: bf.PDelayAndSum(p=3, f_number=1.5, interpolation="nearest", compound="mean", **nl),
         "fdmas": lambda: bf.FilteredDelayMultiplyAndSum(f_number=1.5, interpolation="nearest", compound="mean", **nl)}[kind]()
    probe = bf.build_probe("linear", nb_elements=E, pitch=1e-4, central_freq=FD)
    return b.automatic_setup({"delays": TX, "sampling_freq": FS, "sound_speed": C0, "t0": T0}, probe)


CLASS_CASES = [(k, b, pol, d) for k, b, pol, d in itertools.product(("das", "iq", "pdas", "fdmas"), (None, BAND), (False, True), (False, True))
               if b is None or k in ("pdas", "fdmas")]


@pytest.mark.parametrize("kind,band,polar,on_dev", CLASS_CASES)
def test_a_beamformer_class_reaches_its_entry_points(cx, kind, band, polar, on_dev):
    b = _beamformer(kind, band)
    scan = bf.PolarScan(RHOS, THETAS) if polar else bf.GridScan(X, Z)
    data = IQ if kind == "iq" else RF
    table = capi.DeviceBuffer(cx, (A, NX, NZ), np.float64)
    out = capi.DeviceBuffer(cx, (NX, NZ), data.dtype) if on_dev else None
    arg = dev(cx, data) if on_dev else data[np.newaxis]      # (host: frames first, as USMain.py hands reader.data)
    res = b.beamform(arg, scan, out=out, table=table)        # (a table beside host data is not read)
    tail = ("_table_dev" if on_dev else "")
    stem, typ = (("pbrt_scan_beamform", capi.ScanParams) if polar else
                 {"das": ("pbrt_das_beamform", capi.DasParams), "iq": ("pbrt_iq_beamform", capi.IqParams)}.get(kind, ("pbrt_bf_beamform", capi.BfParams)))
    names = [stem + tail] + (["pbrt_axial_fir" + ("_dev" if on_dev else "")] if band else [])
    assert [c[0] for c in cx.lib.calls] == names
    call = cx.lib.calls[0]
    want = das_fields()
    p = {"pdas": 3.0}.get(kind, 2.0)
    if polar:
        want.update(method=METHODS[kind][1], p=p, demod_freq=np.float32(FD if kind == "iq" else 0.0), probe=0)
    elif kind == "iq":
        want.update(demod_freq=np.float32(FD), probe=0)
    elif kind != "das":
        want.update(method=METHODS[kind][1], p=p, probe=0)
    assert call[1] is typ and fields(call) == want
    assert res.shape == (NX, NZ) and res.dtype == data.dtype
    if not on_dev:
        assert isinstance(res, np.ndarray)
        if band:
            assert cx.lib.calls[1][3][:3] == [NX, NZ, K_TAPS] and cx.lib.calls[1][3][5] == res.ctypes.data
        return
    assert res is out
    raw_ptr = call[3][5]
    d_tx, d_ex, d_x, d_z, kept = (res._keep[0] if band else res)._keep
    px, pz = scan.pixels() if polar else (scan.x_axis.astype(np.float32), scan.z_axis.astype(np.float32))
    assert kept is table and held(cx, d_tx, TX) and held(cx, d_ex, EX) and held(cx, d_x, px) and held(cx, d_z, pz)
    assert call[3] == [arg.ptr, table.ptr, d_ex.ptr, d_x.ptr, d_z.ptr, raw_ptr]
    if band:
        raw, d_taps = res._keep
        assert raw.ptr == raw_ptr != out.ptr and raw.shape == (NX, NZ)
        assert held(cx, d_taps, bf.bandpass_taps(*BAND, C0 / 2e-4, K_TAPS)) or held(cx, d_taps, b.filter_taps(scan, C0))
        assert cx.lib.calls[1][3] == [NX, NZ, K_TAPS, d_taps.ptr, raw.ptr, out.ptr]
    else:
        assert raw_ptr == out.ptr


def test_the_tables_a_renderer_left_in_hbm_are_used(cx):
    b = _beamformer("fdmas", BAND)
    scan = bf.GridScan(X, Z)
    scan.d_x, scan.d_z, b.probe_dev, b.scratch_dev = dev(cx, X), dev(cx, Z), dev(cx, EX), capi.DeviceBuffer(cx, (NX, NZ))
    res = b.beamform(dev(cx, RF), scan)
    raw = res._keep[0]
    assert raw is b.scratch_dev and raw._keep[1:] == (b.probe_dev, scan.d_x, scan.d_z, None)
    assert [c[0] for c in cx.lib.calls] == ["pbrt_bf_beamform_dev", "pbrt_axial_fir_dev"]
    d_taps = res._keep[1]
    assert b.beamform(dev(cx, RF), scan)._keep[1] is d_taps          # the taps are uploaded once
    polar = bf.PolarScan(RHOS, THETAS)
    polar.d_px, polar.d_pz = (dev(cx, t) for t in polar.pixels())
    d = _beamformer("das", None)
    res = d.beamform(dev(cx, RF), polar)
    assert res._keep[2:] == (polar.d_px, polar.d_pz, None) and cx.lib.calls[-1][0] == "pbrt_scan_beamform_dev"
    assert d.beamform(RF, polar).shape == (NX, NZ) and cx.lib.calls[-1][0] == "pbrt_scan_beamform"


def test_the_classes_keep_their_refusals(cx):
    with pytest.raises(RuntimeError, match="DelayAndSum.automatic_setup\\(acquisition_info, probe\\) has not been called"):
        bf.DelayAndSum().beamform(RF, bf.GridScan(X, Z))
    with pytest.raises(RuntimeError, match="PDelayAndSum.automatic_setup\\(acquisition_info, probe\\) has not been called"):
        bf.PDelayAndSum().beamform(RF, bf.GridScan(X, Z))
    with pytest.raises(ValueError, match="DelayAndSum: complex \\(I/Q\\) data, but is_iq is off"):
        _beamformer("das", None).beamform(IQ, bf.GridScan(X, Z))
    with pytest.raises(ValueError, match="FilteredDelayMultiplyAndSum: complex \\(I/Q\\) data, but is_iq is off"):
        _beamformer("fdmas", None).beamform(dev(cx, IQ), bf.GridScan(X, Z))
    with pytest.raises(ValueError, match="DelayAndSum: is_iq is on, but the data are real"):
        _beamformer("iq", None).beamform(RF, bf.PolarScan(RHOS, THETAS))
    with pytest.raises(ValueError, match="step below .* m would fit"):
        _beamformer("fdmas", (1e6, 4e6)).beamform(RF, bf.GridScan(X, Z))
    assert cx.lib.calls == []


# ---- the step wrappers -------------------------------------------------------------------------------------------------------------
IMG = RNG.standard_normal((NX, NZ)).astype(np.float32)
CIMG = (IMG + 1j * IMG[::-1]).astype(np.complex64)
TAPS = np.array([0.25, 0.5, 0.25], np.float32)


def _steps():
    """name -> (wrapper call on `a`, host input, entry-point stem, scalar arguments, extra inputs, result shape, result dtype, message)"""
    sector = bf.PolarScan(RHOS, THETAS)
    return {
        "scan_convert": (lambda a, **kw: bf.scan_convert(a, sector, X[:4], Z[:3], fill=-1.0, **kw), IMG, "pbrt_scan_convert", None,
                         [X[:4], Z[:3]], (4, 3), np.float32, "out must hold nx \\* nz float32"),
        "rf2iq": (lambda a, **kw: bf.rf2iq(a, FD, FS, t0=T0, decimation=3, taps=TAPS, **kw), RF, "pbrt_rf2iq",
                  [A * E, T, FS, T0, FD, 3, 1], [TAPS], (A, E, 6), np.complex64, "out must hold \\[2, 3, 6\\] complex64"),
        "iq_envelope": (lambda a, **kw: bf.iq_envelope(a, **kw), CIMG, "pbrt_iq_envelope", [NX * NZ], [], (NX, NZ), np.float32,
                        "out must hold one float32 per pixel"),
        "axial_fir": (lambda a, **kw: bf.axial_fir(a, TAPS, **kw), IMG, "pbrt_axial_fir", [NX, NZ, 1], [TAPS], (NX, NZ), np.float32,
                      "out must hold nx \\* nz float32"),
        "envelope": (lambda a, **kw: bf.envelope(a, **kw), IMG, "pbrt_envelope", [NX, NZ], [], (NX, NZ), np.float32, None),
        "log_compress": (lambda a, **kw: bf.log_compress(a, 40.0, **kw), IMG, "pbrt_log_compress", [NX * NZ, 40.0], [], (NX, NZ), np.float32, None),
        "apply_pulse": (lambda a, **kw: bf.apply_pulse(a, FS, FD, 2e-7, **kw), RF, "pbrt_us_apply_pulse", [A * E, T, FS, FD, 2e-7], [],
                        (A, E, T), np.float32, None),
    }


@pytest.mark.parametrize("step", list(_steps()))
def test_a_step_wrapper_reaches_both_of_its_forms(cx, step):
    fn, host, stem, scalars, extra, shape, dtype, message = _steps()[step]
    # the host form: a host array out, every input read during the call
    n_sc = 0 if scalars is None else len(scalars)
    order = [host] + extra if step in ("scan_convert", "iq_envelope", "envelope", "apply_pulse") else extra + [host]
    cx.lib.peek[stem] = {1: host.nbytes} if step == "log_compress" else {n_sc + i: a.nbytes for i, a in enumerate(order)}
    res = fn(host)
    assert [c[0] for c in cx.lib.calls] == [stem]
    name, typ, raw, rest, seen = cx.lib.calls[0]
    assert isinstance(res, np.ndarray) and res.shape == shape and res.dtype == dtype
    if step == "log_compress":     # (pbrt_log_compress: n, env, dynamic_range, out)
        assert rest[0] == NX * NZ and rest[2] == 40.0 and rest[3] == res.ctypes.data and seen[1] == host.tobytes()
    else:
        assert (scalars is None or rest[:n_sc] == scalars) and rest[-1] == res.ctypes.data and len(rest) == n_sc + len(order) + 1
        assert [seen[n_sc + i] for i in range(len(order))] == [a.tobytes() for a in order]
    if step == "scan_convert":
        sc = fields(cx.lib.calls[0])
        assert typ is capi.ScanConvertParams and (sc["n_theta"], sc["n_rho"], sc["nx"], sc["nz"], sc["fill"]) == (NX, NZ, 4, 3, -1.0)
        assert (sc["theta0"], sc["rho0"], sc["ox"], sc["oz"]) == (THETAS[0], RHOS[0], 0.0, 0.0)
        assert sc["dtheta"] == (THETAS[-1] - THETAS[0]) / (NX - 1) and sc["drho"] == (RHOS[-1] - RHOS[0]) / (NZ - 1)
    # the device form: a DeviceBuffer out (`out`, or a new one), the inputs kept alive with it
    cx.lib.calls.clear()
    d_in = dev(cx, host)
    res = fn(d_in)
    assert [c[0] for c in cx.lib.calls] == [stem + "_dev"]
    rest_dev = cx.lib.calls[0][3]
    assert isinstance(res, capi.DeviceBuffer) and res.shape == shape and res.dtype == dtype
    assert res._keep[0] is d_in and len(res._keep) == 1 + len(extra)
    assert all(held(cx, k, a) for k, a in zip(res._keep[1:], extra))
    by_pos = [d_in] + list(res._keep[1:]) if order[0] is host else list(res._keep[1:]) + [d_in]
    if step == "log_compress":
        assert rest_dev == [NX * NZ, d_in.ptr, 40.0, res.ptr]
    else:
        assert rest_dev == (rest[:n_sc] + [k.ptr for k in by_pos] + [res.ptr])
    assert cx.lib.calls[0][2] == raw                     # the same parameter block as the host form (scan_convert), or none
    out = capi.DeviceBuffer(cx, shape, dtype)
    assert fn(d_in, out=out) is out and cx.lib.calls[-1][3][-1] == out.ptr
    if message:
        with pytest.raises(ValueError, match=message):
            fn(d_in, out=capi.DeviceBuffer(cx, shape[:-1] + (shape[-1] + 1,), dtype))


def test_the_step_wrappers_keep_their_refusals(cx):
    with pytest.raises(ValueError, match="the image must have the scan's shape \\[5, 7\\] = \\[n_theta, n_rho\\], got \\[7, 5\\]"):
        bf.scan_convert(IMG.T, bf.PolarScan(RHOS, THETAS), X, Z)
    with pytest.raises(ValueError, match="scan_convert takes a float32 image \\(an envelope\\), got a complex64 DeviceBuffer"):
        bf.scan_convert(dev(cx, CIMG), bf.PolarScan(RHOS, THETAS), X, Z)
    with pytest.raises(ValueError, match="rf2iq takes float32 RF traces, got a complex64 DeviceBuffer"):
        bf.rf2iq(dev(cx, IQ), FD, FS, taps=TAPS)
    with pytest.raises(ValueError, match="rf2iq takes real RF traces, got complex data"):
        bf.rf2iq(IQ, FD, FS, taps=TAPS)
    with pytest.raises(ValueError, match="iq_envelope takes complex64 data, got a float32 DeviceBuffer"):
        bf.iq_envelope(dev(cx, IMG))
    with pytest.raises(ValueError, match="iq_envelope takes complex data"):
        bf.iq_envelope(IMG)
    with pytest.raises(ValueError, match="taps must be \\[2 K \\+ 1\\]"):
        bf.axial_fir(IMG, TAPS[:2])
    assert cx.lib.calls == []
    # a single column or trace: the 1-D forms
    assert bf.envelope(IMG[0]).shape == (1, NZ) and cx.lib.calls[-1][3][:2] == [1, NZ]
    assert bf.axial_fir(dev(cx, IMG[0]), TAPS).shape == (NZ,) and cx.lib.calls[-1][3][:3] == [1, NZ, 1]
    assert bf.envelope(dev(cx, IMG[0])).shape == (NZ,) and cx.lib.calls[-1][3][:2] == [1, NZ]
