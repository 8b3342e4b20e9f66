"""Image formation behind the ultrasound hot path: delay-and-sum beamforming of the
channel buffer, envelope and log compression -- the second half of the reference's `us_render`
(USMain.py:93-224), which the reference delegates to the third-party `ultraspy` package.  `ultraspy` is not
available, so the arithmetic is this build's own definition (include/pbrt_hip.h, csrc/kernels_beamform.h,
restated in oracle/beamform.py; parity unpinned).  The classes keep the call shapes USMain.py uses:

    probe = build_probe(geometry_type='linear', nb_elements=N, pitch=p, central_freq=fc, bandwidth=70)   # :130-136
    beamformer = DelayAndSum(on_gpu=False); beamformer.automatic_setup(acquisition_info, probe)         # :174-175
    d_output = beamformer.beamform(d_data, GridScan(x_scan, z_scan))                                    # :204
    envelope = beamformer.compute_envelope(d_output, scan)                                              # :205

PDelayAndSum and FilteredDelayMultiplyAndSum (ultraspy's non-linear beamformers, which the reference does not call) have the same shape;
their arithmetic, from the papers, and the axial band-pass they need are DESIGN.md D19.

I/Q data (`data_info['is_iq']`, USMain.py:158): rf2iq demodulates and decimates, DelayAndSum(is_iq=True) / iq_beamform beamform complex
samples, and the envelope of an I/Q image is its modulus (iq_envelope) -- DESIGN.md D20.

Sector scans: PolarScan beside GridScan, scan_beamform / scan_first_arrival on pixel tables (every method above),
scan_convert from the sector onto a Cartesian grid, us_render(scan="polar").

Capon: ultraspy's fourth beamformer, minimum-variance weights per pixel and transmission on I/Q data -- capon_beamform
and the class Capon, on both kinds of scan; us_render(beamformer=Capon()) runs the I/Q chain with it.
Spatial coherence (not ultraspy's): short-lag spatial coherence and the coherence factor on I/Q data -- coherence_beamform
and the classes ShortLagSpatialCoherence (a float32 detection image: no envelope step) and CoherenceFactor, on both kinds of scan and in us_render.

All work runs on the GPU through libpbrt_hip.so (no CPU fallback; `on_gpu` is accepted for compatibility)."""
from __future__ import annotations

import ctypes as C
import copy
import dataclasses
import math
import time

import numpy as np

from . import _capi


def _das_params(A, E, T, nx, nz, fs, sound_speed, t0, f_number, interpolation, compound) -> "_capi.DasParams":
    p = _capi.DasParams()
    p.n_angles, p.n_elements, p.time_samples = int(A), int(E), int(T)
    p.fs, p.sound_speed, p.t0, p.f_number = float(fs), float(sound_speed), float(t0), float(f_number or 0.0)
    p.interpolation = {"nearest": _capi.DAS_NEAREST, "linear": _capi.DAS_LINEAR}[interpolation]
    p.compound_mean = {"sum": 0, "mean": 1}[compound]
    p.nx, p.nz = int(nx), int(nz)
    return p


def _is_dev(a) -> bool:
    return isinstance(a, _capi.DeviceBuffer)


def _elem_arg(elem, E):
    """the element argument of the beamformer: positions [E] on the line z = 0 (-> the plain entry points), or the element table
    [E, 4] = (x, z, nx, nz) of a curved probe (-> the *_probe entry points; Probe.elements, pbrt_us_array_elements)"""
    if not _is_dev(elem):
        elem = np.asarray(elem)
    shape = tuple(elem.shape)
    probe = shape == (E, 4)
    # (a device buffer goes to the kernel as it is: a table of another size would be read out of bounds)
    if not probe and math.prod(shape) != E:
        raise ValueError(f"element positions must be [{E}] or an element table [{E}, 4], got {list(shape)}")
    return elem, probe, ((E, 4) if probe else (E,))


def _arg(cx, a, shape=None, dev=True):
    """a small table as a call takes it: a DeviceBuffer as it is; a host array as float32 of `shape`, uploaded where the call is a
    device form"""
    if _is_dev(a):
        return a
    a = _capi.f32(np.asarray(a))
    a = a if shape is None else a.reshape(shape)
    return _capi.DeviceBuffer.from_host(cx, a) if dev else a


def _pixel_tables(cx, px, pz, dev):
    """the two pixel tables [n0, n1] of a scan as they are handed on (host float32 arrays, or DeviceBuffers), and (n0, n1)"""
    if _is_dev(px) != _is_dev(pz):
        raise ValueError("px and pz must both be host arrays or both DeviceBuffers")
    if not _is_dev(px):
        px, pz = _capi.f32(np.asarray(px)), _capi.f32(np.asarray(pz))
    if len(px.shape) != 2 or tuple(px.shape) != tuple(pz.shape):
        raise ValueError(f"px and pz must be two tables of one shape [n0, n1], got {list(px.shape)} and {list(pz.shape)}")
    return _arg(cx, px, None, dev), _arg(cx, pz, None, dev), tuple(int(v) for v in px.shape)


def _pixels(cx, gx, gz, tables, dev):
    """the pixel arguments of a call as they are handed on, and the image shape: two tables [n0, n1] (`tables`), or the axes x [nx], z [nz]"""
    if tables:
        return _pixel_tables(cx, gx, gz, dev)
    gx, gz = _arg(cx, gx, (-1,), dev), _arg(cx, gz, (-1,), dev)
    return gx, gz, (gx.shape[0], gz.shape[0])


_METHODS = {"das": _capi.SCAN_DAS, "pdas": _capi.BF_PDAS, "fdmas": _capi.BF_FDMAS, "iq": _capi.SCAN_IQ}
_WINDOWS = {"boxcar": _capi.APOD_BOXCAR, "tukey": _capi.APOD_TUKEY, "hann": _capi.APOD_HANN, "hamming": _capi.APOD_HAMMING}


def _checked_window(rx_apodization, rx_apodization_alpha, f_number):
    """(window, alpha) of a request as the library takes them; ValueError for what it would refuse: an unknown window, a Tukey alpha
    outside (0, 1], and a window other than boxcar without an f-number (there is no aperture to be a window of).  alpha is read by
    "tukey" only."""
    if not isinstance(rx_apodization, str) or rx_apodization not in _WINDOWS:
        raise ValueError(f"rx_apodization must be one of {tuple(_WINDOWS)}, got {rx_apodization!r}")
    alpha = 1.0
    if rx_apodization == "tukey":
        try:
            alpha = float(rx_apodization_alpha)
        except (TypeError, ValueError):
            alpha = float("nan")
        if not (math.isfinite(alpha) and 0.0 < alpha <= 1.0):
            raise ValueError(f"rx_apodization_alpha must lie in (0, 1] for a Tukey window, got {rx_apodization_alpha!r}")
    if rx_apodization != "boxcar" and not (f_number is not None and float(f_number) > 0.0):
        raise ValueError(f"rx_apodization={rx_apodization!r} is a window on the f-number aperture: it needs f_number > 0, got {f_number!r}")
    return _WINDOWS[rx_apodization], alpha


def _block(das, tables, method, p, demod_freq, probe, window=_capi.APOD_BOXCAR, alpha=1.0, capon=None, coherence=None):
    """the parameter block of a request and the family of entry points that takes it: pbrt_scan_* for pixel tables (one block for
    every method); on axes pbrt_das_* (the element table is in the NAME: *_probe), pbrt_bf_* or pbrt_iq_* (a probe flag in the block);
    with a receive window other than boxcar pbrt_apod_* (one block for every method, probe and scan kind, DESIGN D22); capon =
    (l_prop, delta_l): pbrt_capon_* (I/Q data, every probe and scan kind, DESIGN D23); coherence = (kind, half_kernel, lag_prop, gamma):
    pbrt_coherence_* (likewise, DESIGN D26)"""
    if coherence is not None:
        par = _capi.CoherenceParams()
        par.scan.das, par.scan.probe, par.scan.method, par.scan.p = das, int(bool(probe)), _METHODS[method], float(p)
        par.scan.demod_freq = float(demod_freq or 0.0)
        par.tables, par.kind, par.half_kernel = int(bool(tables)), int(coherence[0]), int(coherence[1])
        par.lag_prop, par.gamma = float(coherence[2]), float(coherence[3])
        return par, "coherence"
    if capon is not None:
        par = _capi.CaponParams()
        par.scan.das, par.scan.probe, par.scan.method, par.scan.p = das, int(bool(probe)), _METHODS[method], float(p)
        par.scan.demod_freq = float(demod_freq or 0.0)
        par.tables, par.l_prop, par.delta_l = int(bool(tables)), float(capon[0]), float(capon[1])
        return par, "capon"
    if window != _capi.APOD_BOXCAR:
        par = _capi.ApodParams()
        par.scan.das, par.scan.probe, par.scan.method, par.scan.p = das, int(bool(probe)), _METHODS[method], float(p)
        par.scan.demod_freq = float(demod_freq or 0.0)
        par.tables, par.window, par.alpha = int(bool(tables)), int(window), float(alpha)
        return par, "apod"
    if not tables and method == "das":
        return das, "das"
    par, family = ((_capi.ScanParams(), "scan") if tables else (_capi.IqParams(), "iq") if method == "iq" else (_capi.BfParams(), "bf"))
    par.das, par.probe = das, int(bool(probe))
    if family in ("scan", "bf"):
        par.method, par.p = _METHODS[method], float(p)
    if family in ("scan", "iq"):
        par.demod_freq = float(demod_freq or 0.0)
    return par, family


def _checked_demod_freq(demod_freq) -> float:
    if demod_freq is None or not (math.isfinite(float(demod_freq)) and float(demod_freq) >= 0.0):
        raise ValueError(f"demod_freq must be finite and >= 0, got {demod_freq}")
    return float(demod_freq)


def _first_arrival(tx_delays, elem, gx, gz, tables, sound_speed, out):
    """das_first_arrival (axes) and scan_first_arrival (pixel tables): uploads what is on the host, validates `out`, queues
    pbrt_{das,scan}_first_arrival[_probe]_dev and keeps what the kernel reads alive with the table"""
    cx = next((a.ctx for a in (tx_delays, elem, gx, gz) if _is_dev(a)), None) or _capi.default_context()
    d_tx = tx_delays if _is_dev(tx_delays) else _arg(cx, np.atleast_2d(np.asarray(tx_delays)))
    A, E = d_tx.shape
    elem, probe, eshape = _elem_arg(elem, E)
    d_ex = _arg(cx, elem, eshape)
    d_gx, d_gz, (n0, n1) = _pixels(cx, gx, gz, tables, True)
    par, family = _block(_das_params(A, E, 2, n0, n1, 1.0, sound_speed, 0.0, 0.0, "linear", "sum"), tables, "das", 2.0, None, probe)
    tab = out if out is not None else _capi.DeviceBuffer(cx, (A, n0, n1), np.float64)
    if tab.nbytes != A * n0 * n1 * 8:
        raise ValueError(f"out must hold n_angles * {'n0 * n1' if tables else 'nx * nz'} float64")
    name = f"pbrt_{family}_first_arrival" + ("_probe" if probe and family == "das" else "") + "_dev"
    cx.check(getattr(cx.lib, name)(cx.handle, C.byref(par), d_tx.ptr, d_ex.ptr, d_gx.ptr, d_gz.ptr, tab.ptr), name)
    tab._keep = (d_tx, d_ex, d_gx, d_gz)
    return tab


def das_first_arrival(tx_delays, elem_x, x, z, sound_speed, out=None):
    """first-arrival table of a scan, [n_angles, nx, nz] float64 in HBM: t_tx(a; x, z) = min_e (tx_delays[a, e] + distance to element e / c)
    (pbrt_das_first_arrival_dev; elem_x an element table [n_elements, 4]: pbrt_das_first_arrival_probe_dev).  It depends on the delays and the grid only: a loop that changes neither (USMain.py:262-289) makes it
    once and hands it to every das_beamform(..., table=...) call, which then skips its pass over all elements (same image bit for bit)."""
    return _first_arrival(tx_delays, elem_x, x, z, False, sound_speed, out)


def _beamform(data, tx_delays, elem, gx, gz, tables, fs, sound_speed, *, method, p=2.0, demod_freq=None, t0, f_number, interpolation,
              compound, out, table, rx_apodization="boxcar", rx_apodization_alpha=0.5, capon=None, coherence=None):
    """One beamform request, from every public call to its entry point: `data` by `method` ("das", "pdas" with p, "fdmas", or "iq"
    with demod_freq: data and result complex64) on the pixels gx, gz -- the axes x, z, or (`tables`) two pixel tables.  Shapes the
    arguments, holds RF against I/Q, uploads the small tables where the data is a DeviceBuffer, validates `out` and `table`, selects
    the parameter block and the entry point (_block; [_table] with a first-arrival table, [_dev] for data in HBM), calls it and keeps
    what a queued kernel reads alive with its result.  Host arrays in: a host array out, `out` and `table` are not read.
    rx_apodization: the receive window on the f-number aperture, "boxcar" (today's entry points), "tukey" (with rx_apodization_alpha),
    "hann" or "hamming" (pbrt_apod_*, DESIGN D22); validated before a context is made.
    capon: (l_prop, delta_l) -- the I/Q data go through pbrt_capon_* (DESIGN D23), which has no receive window.
    coherence: (kind, half_kernel, lag_prop, gamma) -- the I/Q data go through pbrt_coherence_* (DESIGN D26), likewise; the image of
    SLSC is float32."""
    window, alpha = _checked_window(rx_apodization, rx_apodization_alpha, f_number)
    if coherence is not None and (method != "iq" or window != _capi.APOD_BOXCAR or capon is not None):
        raise ValueError("SLSC and the coherence factor take I/Q data and no receive window: method 'iq' and rx_apodization='boxcar'")
    if capon is not None and (method != "iq" or window != _capi.APOD_BOXCAR):
        raise ValueError("Capon beamforms I/Q data and makes its own weights: method 'iq' and rx_apodization='boxcar'")
    dev = _is_dev(data)
    iq = method == "iq"
    dtype = np.dtype(np.complex64 if iq else np.float32)
    out_dtype = np.dtype(np.float32) if coherence is not None and coherence[0] == _capi.COH_SLSC else dtype
    cx = data.ctx if dev else _capi.default_context()
    if not dev:
        data, out, table = np.ascontiguousarray(data, dtype=dtype), None, None
    elif iq != (data.dtype.kind == "c"):
        raise ValueError(f"the channel data must be {'complex64 (I/Q)' if iq else 'float32 (RF)'}, got a {data.dtype} DeviceBuffer")
    if len(data.shape) != 3:
        raise ValueError("data must be [n_angles, n_elements, time_samples]")
    A, E, T = data.shape
    elem, probe, eshape = _elem_arg(elem, E)
    tx, ex = _arg(cx, tx_delays, (A, E), dev), _arg(cx, elem, eshape, dev)
    gx, gz, (n0, n1) = _pixels(cx, gx, gz, tables, dev)
    par, family = _block(_das_params(A, E, T, n0, n1, fs, sound_speed, t0, f_number, interpolation, compound), tables, method, p,
                         demod_freq, probe, window, alpha, capon, coherence)
    d0, d1 = ("n0", "n1") if tables else ("nx", "nz")
    res = out if out is not None else _capi.DeviceBuffer(cx, (n0, n1), out_dtype) if dev else np.empty((n0, n1), out_dtype)
    if res.nbytes != n0 * n1 * out_dtype.itemsize:
        raise ValueError(f"out must hold {d0} * {d1} {out_dtype.name}")
    if table is not None and table.nbytes != A * n0 * n1 * 8:   # the first-arrival times of this scan, made once
        raise ValueError(f"table must be the [n_angles, {d0}, {d1}] float64 buffer of {'scan' if tables else 'das'}_first_arrival for this scan")
    name = (f"pbrt_{family}_beamform" + ("_table" if table is not None else "") + ("_probe" if probe and family == "das" else "")
            + ("_dev" if dev else ""))
    args = (data, tx if table is None else table, ex, gx, gz, res)
    cx.check(getattr(cx.lib, name)(cx.handle, C.byref(par), *[a.ptr if dev else a.ctypes.data for a in args]), name)
    if dev:
        res._keep = (tx, ex, gx, gz, table)  # the queued kernel reads them: they live as long as its result
    return res


def das_beamform(data, tx_delays, elem_x, x, z, fs, sound_speed, t0=0.0, f_number=1.0, interpolation="linear",
                 compound="sum", out=None, table=None, rx_apodization="boxcar", rx_apodization_alpha=0.5):
    """data [n_angles, n_elements, T] f32, tx_delays [n_angles, n_elements] (s), elem_x [n_elements] (m),
    grid x [nx], z [nz] (m)  ->  beamformed RF image [nx, nz].
    Host arrays in: pbrt_das_beamform, a host array out.  `data` a DeviceBuffer (the channel buffer of an acquisition that
    stayed in HBM): pbrt_das_beamform_dev -- the small tables are uploaded if they are host arrays, the kernel is queued on
    the context's stream and the result is a DeviceBuffer (`out`, or a new one); nothing waits.  table: the scan's first-arrival
    times from das_first_arrival (pbrt_das_beamform_table_dev).
    elem_x [n_elements, 4] = (x, z, nx, nz): the element table of a curved probe; the same calls with `_probe` in their names
    (distances to (x_e, z_e), the f-number aperture in the element's frame: include/pbrt_hip.h).
    rx_apodization: "boxcar" (the default: every element inside the f-number aperture weighs 1), "tukey" (rx_apodization_alpha in
    (0, 1]), "hann" or "hamming" -- a window on the aperture of every pixel (DESIGN D22, pbrt_apod_beamform*); it needs f_number > 0."""
    return _beamform(data, tx_delays, elem_x, x, z, False, fs, sound_speed, method="das", t0=t0, f_number=f_number,
                     interpolation=interpolation, compound=compound, out=out, table=table, rx_apodization=rx_apodization,
                     rx_apodization_alpha=rx_apodization_alpha)


def nonlinear_beamform(data, tx_delays, elem_x, x, z, fs, sound_speed, method="fdmas", p=2.0, t0=0.0, f_number=1.0,
                       interpolation="linear", compound="sum", out=None, table=None, rx_apodization="boxcar",
                       rx_apodization_alpha=0.5):
    """p-DAS (method="pdas", 1 <= p <= 8) or F-DMAS (method="fdmas") of the channel buffer, BEFORE the axial band-pass both need
    (axial_fir; DESIGN D19, include/pbrt_hip.h).  Arguments and the host / DeviceBuffer rule as das_beamform: host arrays in ->
    pbrt_bf_beamform and a host array out; `data` a DeviceBuffer -> pbrt_bf_beamform_dev (or _table_dev with `table` from
    das_first_arrival), queued, a DeviceBuffer out.  elem_x [n_elements] or the element table [n_elements, 4].
    rx_apodization, rx_apodization_alpha: the receive window of das_beamform; the roots are taken of the weighted samples."""
    if method not in ("pdas", "fdmas"):
        raise ValueError(f"method must be 'pdas' or 'fdmas', got {method!r}")
    return _beamform(data, tx_delays, elem_x, x, z, False, fs, sound_speed, method=method, p=p, t0=t0, f_number=f_number,
                     interpolation=interpolation, compound=compound, out=out, table=table, rx_apodization=rx_apodization,
                     rx_apodization_alpha=rx_apodization_alpha)


def iq_beamform(iq, tx_delays, elem, x, z, fs_iq, sound_speed, demod_freq, t0=0.0, f_number=1.0, interpolation="linear",
                compound="sum", out=None, table=None, rx_apodization="boxcar", rx_apodization_alpha=0.5):
    """Delay-and-sum of I/Q channel data (DESIGN D20, include/pbrt_hip.h): iq [n_angles, n_elements, T] complex64 at the rate fs_iq,
    demodulated at demod_freq (rf2iq), sample m at t0 + m / fs_iq  ->  complex64 image [nx, nz].  The delayed samples are
    das_beamform's (same delays, aperture and interpolation, on complex samples), each turned back by the carrier phase of its delay.
    Arguments and the host / DeviceBuffer rule as das_beamform: host arrays in -> pbrt_iq_beamform and a host array out; `iq` a complex
    DeviceBuffer -> pbrt_iq_beamform_dev (or _table_dev with `table` from das_first_arrival), queued, a complex DeviceBuffer out.
    elem [n_elements] or the element table [n_elements, 4].
    rx_apodization, rx_apodization_alpha: the receive window of das_beamform, on both components of a sample."""
    return _beamform(iq, tx_delays, elem, x, z, False, fs_iq, sound_speed, method="iq", demod_freq=_checked_demod_freq(float(demod_freq)),
                     t0=t0, f_number=f_number, interpolation=interpolation, compound=compound, out=out, table=table,
                     rx_apodization=rx_apodization, rx_apodization_alpha=rx_apodization_alpha)


def _checked_capon(l_prop, delta_l, E):
    """(l_prop, delta_l) as the library takes them; ValueError for what it would refuse (include/pbrt_hip.h "Capon")"""
    try:
        lp, dl = float(l_prop), float(delta_l)
    except (TypeError, ValueError):
        lp = dl = float("nan")
    if not (math.isfinite(lp) and 0.0 <= lp <= 0.5):
        raise ValueError(f"l_prop must lie in [0, 0.5], got {l_prop!r}")
    if not (math.isfinite(dl) and 0.0 < dl <= 1e3):
        raise ValueError(f"delta_l must lie in (0, 1e3], got {delta_l!r}")
    if E > _capi.CAPON_MAX_E:
        raise ValueError(f"Capon takes at most {_capi.CAPON_MAX_E} elements, got {E}")
    return lp, dl


def capon_beamform(iq, tx_delays, elem, x, z, fs_iq, sound_speed, demod_freq, l_prop=0.5, delta_l=0.01, t0=0.0, f_number=1.0,
                   interpolation="linear", compound="sum", out=None, table=None, tables=False):
    """Capon (minimum-variance) beamforming of I/Q channel data (DESIGN D23, include/pbrt_hip.h): the delayed and turned samples of
    iq_beamform -- same delays, aperture and interpolation -- are not added with weights fixed in advance: per pixel and transmission
    the covariance of the subarrays of L = floor(l_prop N) elements (1 <= L <= 32) of the N elements in use is formed, loaded with
    delta_l times its mean diagonal and solved for the minimum-variance weights.  l_prop in [0, 0.5] (0: iq_beamform's image in
    another order of operations), delta_l in (0, 1e3], at most 256 elements.  Arguments and the host / DeviceBuffer rule as
    iq_beamform: host arrays in -> pbrt_capon_beamform and a host array out; `iq` a complex DeviceBuffer -> pbrt_capon_beamform_dev
    (or _table_dev with `table` from das_first_arrival / scan_first_arrival), queued, a complex DeviceBuffer out.  elem [n_elements] or
    the element table [n_elements, 4]; tables: x, z are two pixel tables [n0, n1] (scan_beamform's), not the axes.  There is no
    receive window: the method makes its own weights."""
    shape = tuple(iq.shape) if _is_dev(iq) else np.shape(iq)
    E = shape[1] if len(shape) == 3 else 0   # (any other shape is _beamform's ValueError)
    return _beamform(iq, tx_delays, elem, x, z, bool(tables), fs_iq, sound_speed, method="iq",
                     demod_freq=_checked_demod_freq(float(demod_freq)), t0=t0, f_number=f_number, interpolation=interpolation,
                     compound=compound, out=out, table=table, capon=_checked_capon(l_prop, delta_l, int(E)))


_COH_KINDS = {"slsc": _capi.COH_SLSC, "cf": _capi.COH_CF}


def _checked_coherence(kind, lag_prop, half_kernel, gamma, E):
    """(kind, half_kernel, lag_prop, gamma) as the library takes them; ValueError for what it would refuse (include/pbrt_hip.h
    "spatial coherence").  lag_prop and half_kernel are SLSC's, gamma is the coherence factor's: the other kind's are not read (the
    block carries half_kernel 0 for "cf")."""
    if not isinstance(kind, str) or kind not in _COH_KINDS:
        raise ValueError(f"kind must be one of {tuple(_COH_KINDS)}, got {kind!r}")
    if E > _capi.COH_MAX_E:
        raise ValueError(f"{kind.upper()} takes at most {_capi.COH_MAX_E} elements, got {E}")
    if kind == "slsc":
        try:
            lp = float(lag_prop)
        except (TypeError, ValueError):
            lp = float("nan")
        if not (math.isfinite(lp) and 0.0 < lp <= 1.0):
            raise ValueError(f"lag_prop must lie in (0, 1], got {lag_prop!r}")
        if isinstance(half_kernel, bool) or not isinstance(half_kernel, (int, np.integer)) or not 0 <= int(half_kernel) <= _capi.COH_MAX_H:
            raise ValueError(f"half_kernel must be an integer in [0, {_capi.COH_MAX_H}], got {half_kernel!r}")
        return _capi.COH_SLSC, int(half_kernel), lp, 1.0
    try:
        gm = float(gamma)
    except (TypeError, ValueError):
        gm = float("nan")
    if not (math.isfinite(gm) and 0.0 <= gm <= 4.0):
        raise ValueError(f"gamma must lie in [0, 4], got {gamma!r}")
    return _capi.COH_CF, 0, 0.3, gm


def coherence_beamform(iq, tx_delays, elem, x, z, fs_iq, sound_speed, demod_freq, kind="slsc", lag_prop=0.3, half_kernel=1, gamma=1.0,
                       t0=0.0, f_number=1.0, interpolation="linear", compound="sum", out=None, table=None, tables=False):
    """Spatial-coherence beamforming of I/Q channel data (DESIGN D26, include/pbrt_hip.h): the delayed and turned samples of
    iq_beamform -- same delays, aperture and interpolation -- are not added up as amplitudes; the image is the coherence of the aperture.
    kind="slsc": short-lag spatial coherence (Lediju et al. 2011) -- the normalised correlation between the elements m ranks apart over
    an axial kernel of 2 half_kernel + 1 samples (0 <= half_kernel <= 4), averaged over the pairs and summed over the lags m = 1 ..
    floor(lag_prop N) (0 < lag_prop <= 1, at most 64 lags); a float32 image, clamped at 0.  kind="cf": the coherence factor (Mallart and
    Fink 1994) -- coherent over incoherent power of the aperture, raised to gamma (0 <= gamma <= 4) and multiplied onto delay-and-sum; a
    complex64 image, gamma=0 is iq_beamform's image in another order of operations.  At most 256 elements.  Arguments and the host /
    DeviceBuffer rule as capon_beamform: host arrays in -> pbrt_coherence_beamform and a host array out; `iq` a complex DeviceBuffer ->
    pbrt_coherence_beamform_dev (or _table_dev with `table`), queued, a DeviceBuffer out.  There is no receive window."""
    shape = tuple(iq.shape) if _is_dev(iq) else np.shape(iq)
    E = shape[1] if len(shape) == 3 else 0   # (any other shape is _beamform's ValueError)
    return _beamform(iq, tx_delays, elem, x, z, bool(tables), fs_iq, sound_speed, method="iq",
                     demod_freq=_checked_demod_freq(float(demod_freq)), t0=t0, f_number=f_number, interpolation=interpolation,
                     compound=compound, out=out, table=table, coherence=_checked_coherence(kind, lag_prop, half_kernel, gamma, int(E)))


_SCAN_METHODS = ("das", "pdas", "fdmas", "iq")


def scan_first_arrival(tx_delays, elem, px, pz, sound_speed, out=None):
    """das_first_arrival for a scan given as pixel tables px, pz [n0, n1] (metres, the probe's frame): [n_angles, n0, n1] float64 in
    HBM, t_tx(a; pixel) = min_e (tx_delays[a, e] + distance to element e / c) (pbrt_scan_first_arrival_dev).  elem [n_elements] or
    the element table [n_elements, 4].  On the tables of a separable scan it equals das_first_arrival bit for bit."""
    return _first_arrival(tx_delays, elem, px, pz, True, sound_speed, out)


def scan_beamform(data, tx_delays, elem, px, pz, fs, sound_speed, method="das", p=2.0, demod_freq=None, t0=0.0, f_number=1.0,
                  interpolation="linear", compound="sum", out=None, table=None, rx_apodization="boxcar", rx_apodization_alpha=0.5):
    """Beamforming on a scan given as two pixel tables px, pz [n0, n1] (metres, the probe's frame; a PolarScan's .pixels(), or any
    other list of pixels) -> image [n0, n1] (DESIGN D21, pbrt_scan_beamform).  method: "das" (das_beamform's arithmetic), "pdas" (with
    p) / "fdmas" (nonlinear_beamform's, BEFORE the axial band-pass) or "iq" (iq_beamform's: complex64 data at the rate fs, demodulated
    at demod_freq, a complex64 image).  On np.meshgrid(x, z, indexing="ij") the result is that call's on the axes x, z, bit for bit.
    The host / DeviceBuffer rule is das_beamform's: host arrays in -> a host array out; `data` a DeviceBuffer ->
    pbrt_scan_beamform_dev, queued, a DeviceBuffer out (`out`, or a new one; host tables are uploaded), with `table` from
    scan_first_arrival -> pbrt_scan_beamform_table_dev.  elem [n_elements] or the element table [n_elements, 4].
    rx_apodization, rx_apodization_alpha: the receive window of das_beamform (pbrt_apod_beamform* with tables = 1)."""
    if method not in _SCAN_METHODS:
        raise ValueError(f"method must be one of {_SCAN_METHODS}, got {method!r}")
    if method == "iq":
        _checked_demod_freq(demod_freq)
    return _beamform(data, tx_delays, elem, px, pz, True, fs, sound_speed, method=method, p=p, demod_freq=demod_freq, t0=t0,
                     f_number=f_number, interpolation=interpolation, compound=compound, out=out, table=table,
                     rx_apodization=rx_apodization, rx_apodization_alpha=rx_apodization_alpha)


def _step(stem, src, args, shape, dtype, out, message=None):
    """One step around the beamformer in its host or its device form.  src: the input that decides -- a host array -> the entry
    point `stem`, a host array of `shape` and `dtype` out; a DeviceBuffer -> stem + "_dev", queued, the result `out` (which must
    hold `shape`: ValueError(message), where the step has one) or a new DeviceBuffer, which keeps src and the other buffers alive.
    args: what the entry point takes between the context and the output -- scalars, and buffers that are all of src's kind."""
    if not isinstance(src, _capi.DeviceBuffer):
        cx, res = _capi.default_context(), np.empty(shape, dtype)
        cx.check(getattr(cx.lib, stem)(cx.handle, *[a.ctypes.data if isinstance(a, np.ndarray) else a for a in args], res.ctypes.data), stem)
        return res
    cx, name = src.ctx, stem + "_dev"
    res = out if out is not None else _capi.DeviceBuffer(cx, shape, dtype)
    if message is not None and res.nbytes != math.prod(shape) * np.dtype(dtype).itemsize:
        raise ValueError(message)
    ptrs, keep = [], [src]
    for a in args:   # (one pass: this runs once per queued step of every us_render call)
        if isinstance(a, _capi.DeviceBuffer):
            ptrs.append(a.ptr)
            if a is not src:
                keep.append(a)
        else:
            ptrs.append(a)
    cx.check(getattr(cx.lib, name)(cx.handle, *ptrs, res.ptr), name)
    res._keep = tuple(keep)
    return res


def scan_convert(img, scan, x_axis, z_axis, fill=0.0, out=None):
    """A sector image img [n_theta, n_rho] on the PolarScan `scan` resampled onto the Cartesian axes x_axis [nx], z_axis [nz] ->
    [nx, nz] (pbrt_scan_convert, DESIGN D21): bilinear in (theta, rho), pixels outside the sector are `fill`.  A host array in gives a
    host array out; a DeviceBuffer in gives a DeviceBuffer out, queued (the axes DeviceBuffers, or host arrays that are uploaded)."""
    dev = _is_dev(img)
    cx = img.ctx if dev else _capi.default_context()
    if not dev:
        img = _capi.f32(np.asarray(img))
    if tuple(img.shape) != scan.shape:
        raise ValueError(f"the image must have the scan's shape {list(scan.shape)} = [n_theta, n_rho], got {list(img.shape)}")
    if dev and img.dtype != np.float32:
        raise ValueError(f"scan_convert takes a float32 image (an envelope), got a {img.dtype} DeviceBuffer")
    gx, gz, (nx, nz) = _pixels(cx, x_axis, z_axis, False, dev)
    sc = _capi.ScanConvertParams()
    sc.n_theta, sc.n_rho, sc.nx, sc.nz = scan.shape[0], scan.shape[1], int(nx), int(nz)
    sc.theta0, sc.dtheta = float(scan.thetas[0]), float((scan.thetas[-1] - scan.thetas[0]) / (len(scan.thetas) - 1))
    sc.rho0, sc.drho = float(scan.rhos[0]), float((scan.rhos[-1] - scan.rhos[0]) / (len(scan.rhos) - 1))
    sc.ox, sc.oz = scan.origin
    sc.fill = float(fill)
    return _step("pbrt_scan_convert", img, (C.byref(sc), img, gx, gz), (nx, nz), np.float32, out, "out must hold nx * nz float32")


RF2IQ_MAX_DECIMATION = 8


def lowpass_taps(f_cut, fs, K=None) -> np.ndarray:
    """Hamming-windowed sinc low-pass below f_cut at the sampling rate fs: bandpass_taps(0, f_cut, fs, K)"""
    return bandpass_taps(0.0, f_cut, fs, K)


def _rf2iq_lowpass(fc, fs, bandwidth, D) -> np.ndarray:
    """rf2iq's default low-pass, cut-off fc * bandwidth / 200 at the rate fs; ValueError when it does not lie below the Nyquist
    frequency fs / (2 D) of the decimated rate -- the message names the largest decimation that fits"""
    f_cut = fc * float(bandwidth) / 200.0
    if not f_cut > 0.0:
        raise ValueError(f"rf2iq: the default low-pass needs central_freq * bandwidth > 0, got a cut-off of {f_cut} Hz")
    if f_cut >= fs / (2.0 * D):
        fits = min(RF2IQ_MAX_DECIMATION, int(np.ceil(fs / (2.0 * f_cut))) - 1)   # the largest D with f_cut < fs / (2 D)
        raise ValueError(
            f"rf2iq: the low-pass cut-off {f_cut:.6g} Hz does not lie below the Nyquist frequency {fs / (2.0 * D):.6g} Hz of "
            f"{fs:.6g} Hz decimated by {D}; " + (f"the largest decimation that fits is {fits}" if fits >= 1 else
                                                 "no decimation fits: the cut-off is not below sampling_freq / 2"))
    return lowpass_taps(f_cut, fs)


def rf2iq(data, central_freq, sampling_freq, t0=0.0, bandwidth=100, decimation=1, taps=None, out=None):
    """RF traces [..., T] (sample j at t0 + j / sampling_freq) -> baseband I/Q [..., Td] complex64, Td = ceil(T / decimation), sample m
    at t0 + m decimation / sampling_freq: mixed with exp(-2 pi i central_freq t), low-passed, decimated, times 2 (pbrt_rf2iq,
    DESIGN D20).  The default low-pass is lowpass_taps(central_freq * bandwidth / 200, sampling_freq) (bandwidth in per cent of the
    carrier, two-sided); it must lie below the Nyquist frequency of the decimated rate.  taps [2 K + 1]: the caller's own low-pass at
    the rate sampling_freq (bandwidth is then not read).  A host array in gives a host array out; a DeviceBuffer in gives a
    DeviceBuffer(dtype=complex64) out, queued (the taps then a DeviceBuffer or a host array that is uploaded)."""
    fc, fs, D = float(central_freq), float(sampling_freq), int(decimation)
    if not 1 <= D <= RF2IQ_MAX_DECIMATION or D != decimation:
        raise ValueError(f"rf2iq: decimation must be an integer in [1, {RF2IQ_MAX_DECIMATION}], got {decimation}")
    if not (np.isfinite(fc) and fc >= 0.0):
        raise ValueError(f"rf2iq: central_freq must be finite and >= 0, got {fc}")
    if not (np.isfinite(fs) and fs > 0.0):
        raise ValueError(f"rf2iq: sampling_freq must be finite and > 0, got {fs}")
    if taps is None:
        taps = _rf2iq_lowpass(fc, fs, bandwidth, D)
    n_taps = taps.shape[0] if _is_dev(taps) else np.asarray(taps).size
    if n_taps % 2 != 1:
        raise ValueError("taps must be [2 K + 1]")
    K = n_taps // 2
    dev = _is_dev(data)
    if dev:
        if data.dtype != np.float32:
            raise ValueError(f"rf2iq takes float32 RF traces, got a {data.dtype} DeviceBuffer")
        x = data
    else:
        if np.iscomplexobj(data):
            raise ValueError("rf2iq takes real RF traces, got complex data")
        x = _capi.f32(np.asarray(data))
    shape = tuple(x.shape)
    T = shape[-1]
    n_traces = int(np.prod(shape[:-1], dtype=np.int64))
    oshape = shape[:-1] + (-(-T // D),)
    h = _arg(x.ctx if dev else None, taps, (-1,), dev)
    return _step("pbrt_rf2iq", x, (n_traces, T, fs, float(t0), fc, D, K, h, x), oshape, np.complex64, out,
                 f"out must hold {list(oshape)} complex64")


def _columns(rf):
    """an image [nx, nz], or one column [nz], as the axial steps take it (a host array: float32 [nx, nz]), and (nx, nz)"""
    if not _is_dev(rf):
        rf = _capi.f32(np.atleast_2d(np.asarray(rf)))
    return rf, (rf.shape if len(rf.shape) == 2 else (1, rf.shape[0]))


def iq_envelope(iq, out=None):
    """envelope of an I/Q image: the modulus of each pixel, on any grid and of any size (pbrt_iq_envelope; a complex DeviceBuffer in
    gives a float32 DeviceBuffer out, queued)"""
    if _is_dev(iq):
        if iq.dtype.kind != "c":
            raise ValueError(f"iq_envelope takes complex64 data, got a {iq.dtype} DeviceBuffer")
    elif not np.iscomplexobj(iq):
        raise ValueError("iq_envelope takes complex data")
    else:
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
    return _step("pbrt_iq_envelope", iq, (iq.nbytes // 8, iq), iq.shape, np.float32, out, "out must hold one float32 per pixel")


def axial_fir(rf, taps, out=None):
    """out[ix, n] = sum_{k = -K .. K} taps[K + k] rf[ix, n - k] along the last (axial) axis of a [nx, nz] image, zero outside the
    column; taps [2 K + 1], K <= 1024 (pbrt_axial_fir; a DeviceBuffer in gives a DeviceBuffer out, queued -- the taps then a
    DeviceBuffer or a host array that is uploaded)."""
    n_taps = taps.shape[0] if _is_dev(taps) else np.asarray(taps).size
    if n_taps % 2 != 1:
        raise ValueError("taps must be [2 K + 1]")
    dev = _is_dev(rf)
    rf, (nx, nz) = _columns(rf)
    h = _arg(rf.ctx if dev else None, taps, (n_taps,), dev)
    return _step("pbrt_axial_fir", rf, (nx, nz, n_taps // 2, h, rf), rf.shape, np.float32, out, "out must hold nx * nz float32")


FIR_MAX_K = 1024


def axial_rate(z_axis, sound_speed) -> float:
    """axial sampling rate of an image, fs_ax = c / (2 dz): a depth step dz is 2 dz / c of round-trip time.  ValueError for a z axis
    that is not uniform to 1e-6 of its step."""
    z = np.asarray(z_axis, dtype=np.float64).ravel()
    if z.size < 2:
        raise ValueError("the z axis needs two samples at least to have a sampling rate")
    d = np.diff(z)
    dz = (z[-1] - z[0]) / (z.size - 1)
    if not (dz > 0.0 and np.all(np.abs(d - dz) <= 1e-6 * dz)):
        raise ValueError("the axial band-pass needs a uniform, increasing z axis (to 1e-6 of its step)")
    return float(sound_speed) / (2.0 * dz)


def bandpass_taps(f_lo, f_hi, fs_ax, K=None) -> np.ndarray:
    """Hamming-windowed sinc band-pass [f_lo, f_hi] at the sampling rate fs_ax (axial_rate), taps [2 K + 1] for axial_fir:
        h[k] = (0.54 + 0.46 cos(pi k / K)) (2 f_hi / fs_ax sinc(2 f_hi k / fs_ax) - 2 f_lo / fs_ax sinc(2 f_lo k / fs_ax)),
    in float64, rounded once to float32.  Default K = min(1024, ceil(4 fs_ax / (f_hi - f_lo))).  ValueError for f_lo >= f_hi,
    f_lo < 0 and f_hi >= fs_ax / 2."""
    f_lo, f_hi, fs_ax = float(f_lo), float(f_hi), float(fs_ax)
    if not (fs_ax > 0.0 and np.isfinite(fs_ax)):
        raise ValueError(f"band-pass: the sampling rate must be finite and > 0, got {fs_ax}")
    if not f_lo >= 0.0:
        raise ValueError(f"band-pass: f_lo must be >= 0, got {f_lo}")
    if not f_lo < f_hi:
        raise ValueError(f"band-pass: f_lo ({f_lo}) must lie below f_hi ({f_hi})")
    if not f_hi < fs_ax / 2.0:
        raise ValueError(f"band-pass: f_hi ({f_hi:.6g} Hz) must lie below the Nyquist frequency fs_ax / 2 = {fs_ax / 2.0:.6g} Hz")
    if K is None:
        K = min(FIR_MAX_K, int(np.ceil(4.0 * fs_ax / (f_hi - f_lo))))
    K = int(K)
    if not 1 <= K <= FIR_MAX_K:
        raise ValueError(f"band-pass: K must lie in [1, {FIR_MAX_K}], got {K}")
    k = np.arange(-K, K + 1, dtype=np.float64)
    hi, lo = 2.0 * f_hi / fs_ax, 2.0 * f_lo / fs_ax
    h = (0.54 + 0.46 * np.cos(np.pi * k / K)) * (hi * np.sinc(hi * k) - lo * np.sinc(lo * k))
    return h.astype(np.float32)


def envelope(rf, out=None):
    """|analytic signal| along the last (axial) axis of a [nx, nz] RF image (pbrt_envelope; a DeviceBuffer in gives a
    DeviceBuffer out, queued on the context's stream)."""
    rf, (nx, nz) = _columns(rf)
    return _step("pbrt_envelope", rf, (nx, nz, rf), rf.shape, np.float32, out)


def log_compress(env, dynamic_range=60.0, out=None):
    """USMain.py:210-218: 20 log10(env + 1e-12) clipped to the top `dynamic_range` dB, mapped to [0, 1]."""
    if not _is_dev(env):
        env = _capi.f32(np.asarray(env))
    return _step("pbrt_log_compress", env, (env.nbytes // 4, env, float(dynamic_range)), env.shape, np.float32, out)


def apply_pulse(traces, fs, frequency, sigma, out=None):
    """SURVEY f-3 pulse model (RayTracingV0.py:194-204): every trace (last axis) convolved with
    h[k] = sin(2 pi f k / fs) exp(-(k / fs)^2 / sigma^2)  (pbrt_us_apply_pulse; DeviceBuffer in -> DeviceBuffer out)."""
    if not _is_dev(traces):
        traces = _capi.f32(np.asarray(traces))
    T = traces.shape[-1]
    return _step("pbrt_us_apply_pulse", traces, ((traces.nbytes // 4) // T, T, float(fs), float(frequency), float(sigma), traces),
                 traces.shape, np.float32, out)


# ---- ultraspy-shaped front end (USMain.py:126-205) ---------------------------------------------------------------
def convex_params(n_elements, radius, opening_angle, params=None) -> "_capi.UsParams":
    """the array part of a pbrt_us_params for a curved array (PBRT_US_ARRAY_CONVEX, DESIGN D18); raises on what the library refuses"""
    import math
    n, radius, opening_angle = int(n_elements), float(radius), float(opening_angle)
    if not (math.isfinite(radius) and radius > 0.0):
        raise ValueError(f"convex array: radius must be finite and > 0, got {radius}")
    if not (math.isfinite(opening_angle) and 0.0 < opening_angle < 180.0):
        raise ValueError(f"convex array: opening_angle must lie in (0, 180) degrees, got {opening_angle}")
    if n <= 0:
        raise ValueError("convex array: no elements")
    p = params if params is not None else _capi.UsParams()
    p.n_elements = n
    p.primary = int(p.primary) | _capi.US_ARRAY_CONVEX
    p.emitter.number_of_elements = n
    p.emitter.radius, p.emitter.opening_angle = radius, opening_angle
    return p


def array_elements(params) -> np.ndarray:
    """[n_elements, 4] = (x, z, nx, nz) of the array a pbrt_us_params describes (pbrt_us_array_elements; host only, no device)"""
    elem = np.empty((int(params.n_elements), 4), np.float32)
    rc = _capi.load_library().pbrt_us_array_elements(C.byref(params), _capi.addr(elem))
    if rc != 0:
        raise ValueError(f"pbrt_us_array_elements refused the array (rc={rc})")
    return elem


class Probe:
    def __init__(self, geometry_type, nb_elements, pitch, central_freq, bandwidth=70, radius=None, opening_angle=None):
        if geometry_type not in ("linear", "convex"):
            raise NotImplementedError(f"probe geometry '{geometry_type}': 'linear' (USMain.py:130-136) and 'convex' are built")
        self.geometry_type = geometry_type
        self.nb_elements = int(nb_elements)
        self.pitch = float(pitch)
        self.central_freq = float(central_freq)
        self.bandwidth = float(bandwidth)
        self.geometry = np.zeros((3, self.nb_elements), dtype=np.float32)
        self.normals = np.zeros((3, self.nb_elements), dtype=np.float32)
        if geometry_type == "linear":
            if radius or opening_angle:
                raise ValueError("a linear probe has no radius / opening_angle")
            # same element positions as the integrator (CustomIntegrator.py:248)
            self.geometry[0] = self.pitch * (np.arange(self.nb_elements, dtype=np.float32) - (self.nb_elements - 1) / 2)
            self.normals[2] = 1.0
            self.radius = self.opening_angle = 0.0
            self.elements = None
        else:
            # the curved array of CustomEmmitter.py:41-47 as the library places it (pbrt_us_array_elements, DESIGN D18): centre of
            # curvature at the origin, apex (0, 0, radius); `pitch` is kept but not read
            if radius is None or opening_angle is None:
                # (ultraspy describes a curved probe by its pitch; that description is not built: the arc is CustomEmitter's)
                raise NotImplementedError("build_probe('convex', ...) is built for radius= (m) and opening_angle= (degrees) only")
            self.radius, self.opening_angle = float(radius), float(opening_angle)
            self.elements = array_elements(convex_params(self.nb_elements, self.radius, self.opening_angle))
            self.geometry[0], self.geometry[2] = self.elements[:, 0], self.elements[:, 1]
            self.normals[0], self.normals[2] = self.elements[:, 2], self.elements[:, 3]

    @property
    def das_elements(self):
        """what the beamformer takes: positions [E] (linear), the element table [E, 4] (convex)"""
        return self.geometry[0] if self.elements is None else self.elements


def build_probe(geometry_type="linear", nb_elements=64, pitch=1.2e-4, central_freq=3e6, bandwidth=70, radius=None,
                opening_angle=None):
    return Probe(geometry_type, nb_elements, pitch, central_freq, bandwidth, radius=radius, opening_angle=opening_angle)


class GridScan:
    def __init__(self, x_axis, z_axis):
        self.x_axis = np.asarray(x_axis, dtype=np.float64).ravel()
        self.z_axis = np.asarray(z_axis, dtype=np.float64).ravel()
        self.d_x = self.d_z = None  # the axes as DeviceBuffers (set by us_render)

    @property
    def shape(self):
        return (len(self.x_axis), len(self.z_axis))


def _uniform_axis(axis, name) -> np.ndarray:
    """a uniform, increasing axis of two samples at least (to 1e-6 of its step, as axial_rate asks of a z axis); ValueError otherwise"""
    a = np.asarray(axis, dtype=np.float64).ravel()
    if a.size < 2:
        raise ValueError(f"PolarScan: the {name} axis needs two samples at least")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"PolarScan: the {name} axis must be finite")
    d = np.diff(a)
    step = (a[-1] - a[0]) / (a.size - 1)
    if not (step > 0.0 and np.all(np.abs(d - step) <= 1e-6 * step)):
        raise ValueError(f"PolarScan: the {name} axis must be uniform and increasing (to 1e-6 of its step)")
    return a


class PolarScan:
    """ultraspy's PolarScan, the sector a curved or a steered array insonifies: pixel (i, j) lies at the angle thetas[i] (radians, from
    the +z axis towards +x) and the distance rhos[j] from `origin` = (ox, oz), in the probe's frame -- x = ox + rho sin(theta),
    z = oz + rho cos(theta).  shape == (n_theta, n_rho): rho is the last (axial) axis, so axial_fir and envelope run along the rays.
    Both axes must be uniform and increasing (scan_convert's rule; ValueError otherwise).  `ultraspy` is absent: the signature
    (rhos, thetas) is from memory and parity with it is unpinned, as everywhere in this file.  The beamformers take it where they take
    a GridScan (scan_beamform on its pixel tables); scan_convert brings the result onto a Cartesian grid."""

    def __init__(self, rhos, thetas, origin=(0.0, 0.0)):
        self.rhos = _uniform_axis(rhos, "rho")
        self.thetas = _uniform_axis(thetas, "theta")
        ox, oz = (float(v) for v in origin)
        if not (np.isfinite(ox) and np.isfinite(oz)):
            raise ValueError(f"PolarScan: the origin must be finite, got {origin}")
        self.origin = (ox, oz)
        self.d_px = self.d_pz = None  # the pixel tables as DeviceBuffers (set by us_render)

    @property
    def shape(self):
        return (len(self.thetas), len(self.rhos))

    def pixels(self):
        """(px, pz), float32 [n_theta, n_rho]: computed in float64, rounded once"""
        th, rho = self.thetas[:, np.newaxis], self.rhos[np.newaxis, :]
        return ((self.origin[0] + rho * np.sin(th)).astype(np.float32), (self.origin[1] + rho * np.cos(th)).astype(np.float32))


def _axial_axis(scan) -> np.ndarray:
    """the axis an image of this scan is sampled along in the propagation direction: rho of a PolarScan, z of a GridScan"""
    return scan.rhos if isinstance(scan, PolarScan) else scan.z_axis


def _scan_tables(scan, dev):
    """what a beamformer hands on for a scan: (True, px, pz) for a PolarScan, (False, x, z) for a GridScan -- the copies in HBM
    (us_render keeps them there between calls) where the data is a DeviceBuffer"""
    if isinstance(scan, PolarScan):
        if dev and scan.d_px is not None and scan.d_pz is not None:
            return True, scan.d_px, scan.d_pz
        return (True,) + scan.pixels()
    gx = scan.d_x if dev and getattr(scan, "d_x", None) is not None else scan.x_axis
    gz = scan.d_z if dev and getattr(scan, "d_z", None) is not None else scan.z_axis
    return False, gx, gz


def polar_n_theta(rho_max, theta_range, step) -> int:
    """us_render's rule for the angles of a sector: the smallest count n_theta >= 2 with rho_max * dtheta <= step, dtheta =
    (theta_range[1] - theta_range[0]) / (n_theta - 1) -- neighbouring rays are no further apart than neighbouring depths anywhere"""
    rho_max, step, span = float(rho_max), float(step), float(theta_range[1]) - float(theta_range[0])
    if not (span > 0.0 and rho_max > 0.0 and step > 0.0 and np.isfinite(span * rho_max / step)):
        raise ValueError(f"a sector needs theta_range[0] < theta_range[1], rho_max > 0 and step > 0, got {theta_range}, {rho_max}, {step}")
    n = max(2, int(np.ceil(rho_max * span / step)) + 1)
    while n > 2 and rho_max * (span / (n - 2)) <= step:   # (the quotient above may round either way)
        n -= 1
    while rho_max * (span / (n - 1)) > step:
        n += 1
    return n


class DelayAndSum:
    """ultraspy's DelayAndSum in the call shapes USMain.py uses.  Setups: f_number, interpolation, compound, is_iq, demod_freq, and the
    receive window rx_apodization ("boxcar", "tukey", "hann", "hamming") with rx_apodization_alpha (read by "tukey" only; DESIGN D22).
    `ultraspy` is absent: the names rx_apodization / rx_apodization_alpha and the values 'boxcar' / 'tukey' are ultraspy's from memory,
    and parity with it is unpinned, as everywhere in this file.  A setup that cannot be beamformed (an unknown window, an alpha outside
    (0, 1], a window with f_number 0) is a ValueError of beamform()."""
    _method = "das"
    real_image = False   # the image of beamform() is what compute_envelope detects (True: it is a detection image already, D26)

    def __init__(self, on_gpu=True, f_number=1.0, interpolation="linear", compound="sum", is_iq=False, rx_apodization="boxcar",
                 rx_apodization_alpha=0.5):
        self.on_gpu = on_gpu  # accepted for compatibility; the beamformer has no CPU path
        # is_iq: the data are I/Q samples (complex64) at the rate acquisition_info['sampling_freq'], demodulated at `demod_freq`
        # (None: probe.central_freq)
        self.setups = {"f_number": f_number, "interpolation": interpolation, "compound": compound, "is_iq": False, "demod_freq": None,
                       "rx_apodization": rx_apodization, "rx_apodization_alpha": rx_apodization_alpha}
        self.set_is_iq(is_iq)
        self.acquisition_info = None
        self.probe = None
        self.probe_dev = None  # element positions as a DeviceBuffer (set by us_render)

    def automatic_setup(self, acquisition_info, probe):
        self.acquisition_info = dict(acquisition_info)
        self.probe = probe
        return self

    def update_setup(self, name, value):
        if name not in self.setups:
            raise KeyError(name)
        if name == "is_iq":
            return self.set_is_iq(value)
        self.setups[name] = value

    def set_is_iq(self, flag):
        """ultraspy's beamformer.set_is_iq: the data given to beamform() are I/Q samples, its result is complex and compute_envelope
        is the modulus"""
        self.setups["is_iq"] = bool(flag)

    @property
    def is_iq(self):
        return bool(self.setups["is_iq"])

    def demod_freq(self):
        f = self.setups["demod_freq"]
        return float(self.probe.central_freq if f is None else f)

    def _checked(self, d_data):
        """the data as they go on: a DeviceBuffer, or the host array without its frame axis.  RuntimeError before automatic_setup;
        ValueError where real or complex data meet the wrong is_iq."""
        if self.acquisition_info is None or self.probe is None:
            raise RuntimeError(f"{type(self).__name__}.automatic_setup(acquisition_info, probe) has not been called")
        data = d_data
        if not _is_dev(data):
            data = np.asarray(d_data)
            if data.ndim == 4:      # (frames, n_angles, n_elements, T): USMain passes reader.data[0]
                data = data[0]
        _check_iq(self, data)
        return data

    def _request(self, data, scan, out, table):
        """the beamform request acquisition_info, the probe, the setups and the scan make up, by the class's method and p"""
        ai, su, iq, dev = self.acquisition_info, self.setups, self.is_iq, _is_dev(data)
        # tables that already sit in HBM (us_render keeps them there between calls) are used where the data is a DeviceBuffer
        ex = self.probe_dev if dev and self.probe_dev is not None else self.probe.das_elements
        polar, gx, gz = _scan_tables(scan, dev)   # (a PolarScan: the same arithmetic on its pixel tables, DESIGN D21)
        return _beamform(data, ai["delays"], ex, gx, gz, polar, ai["sampling_freq"], ai["sound_speed"],
                         method="iq" if iq else self._method, p=su.get("p", 2.0),
                         demod_freq=_checked_demod_freq(self.demod_freq()) if iq else None, t0=ai.get("t0", 0.0) or 0.0,
                         f_number=su["f_number"], interpolation=su["interpolation"], compound=su["compound"], out=out, table=table,
                         rx_apodization=su["rx_apodization"], rx_apodization_alpha=su["rx_apodization_alpha"])

    def beamform(self, d_data, scan, out=None, table=None):
        """host array in -> host array out; a DeviceBuffer in (the channel buffer left in HBM) -> a DeviceBuffer out, queued.
        is_iq: complex64 in (host, or a complex DeviceBuffer), complex out."""
        return self._request(self._checked(d_data), scan, out, table)

    def beamform_packet(self, d_data, scan, out=None):
        """An ensemble of pulses, one image per frame (DESIGN D24; ultraspy's packet beamforming from memory, parity unpinned): host
        data [frames, n_angles, n_elements, T] complex64 -> a host array [frames, nx, nz] complex64; a list of complex DeviceBuffers
        [n_angles, n_elements, T] -> a complex DeviceBuffer [frames, nx, nz] (`out`, or a new one), queued.  The first-arrival table
        of the scan is made once and every frame goes through the _table_dev entry point of this beamformer into its part of the
        ensemble (DeviceBuffer.view): frame n equals beamform() of that frame bit for bit.  I/Q data only: ValueError without is_iq."""
        if self.acquisition_info is None or self.probe is None:
            raise RuntimeError(f"{type(self).__name__}.automatic_setup(acquisition_info, probe) has not been called")
        if not self.is_iq:
            raise ValueError(f"{type(self).__name__}.beamform_packet takes I/Q data: set_is_iq(True) and demodulate the frames (rf2iq)")
        host = not isinstance(d_data, (list, tuple))
        if host:
            data = np.asarray(d_data)
            if data.ndim != 4:
                raise ValueError(f"beamform_packet takes [frames, n_angles, n_elements, T], got {list(data.shape)}")
            _check_iq(self, data)
            cx = _capi.default_context()
            frames = [_capi.DeviceBuffer.from_host(cx, np.ascontiguousarray(f, dtype=np.complex64)) for f in data]
        else:
            frames = list(d_data)
            if not all(_is_dev(f) for f in frames):
                raise ValueError("beamform_packet takes a host array, or a list of DeviceBuffers")
            for f in frames:
                _check_iq(self, f)
        if not frames or any(tuple(f.shape) != tuple(frames[0].shape) or f.ctx is not frames[0].ctx for f in frames):
            raise ValueError("beamform_packet needs one frame at least, all of one shape and on one context")
        cx, N, (n0, n1) = frames[0].ctx, len(frames), scan.shape
        ens = out if out is not None else _capi.DeviceBuffer(cx, (N, n0, n1), np.complex64)
        if not _is_dev(ens) or ens.nbytes != N * n0 * n1 * 8:
            raise ValueError("out must be a DeviceBuffer that holds frames * nx * nz complex64")
        ai = self.acquisition_info
        polar, gx, gz = _scan_tables(scan, True)
        table = _first_arrival(ai["delays"], self.probe_dev if self.probe_dev is not None else self.probe.das_elements, gx, gz, polar,
                               ai["sound_speed"], None)
        # the small tables the table's kernel read sit in HBM now: every frame's call takes them from there
        d_tx, d_ex, d_gx, d_gz = table._keep
        names = ("d_px", "d_pz") if polar else ("d_x", "d_z")
        saved = (self.acquisition_info, self.probe_dev, getattr(scan, names[0], None), getattr(scan, names[1], None))
        self.acquisition_info, self.probe_dev = dict(ai, delays=d_tx), d_ex
        setattr(scan, names[0], d_gx), setattr(scan, names[1], d_gz)
        try:
            for n, f in enumerate(frames):
                self._request(f, scan, ens.view(n * n0 * n1, (n0, n1)), table)
        finally:
            self.acquisition_info, self.probe_dev = saved[0], saved[1]
            setattr(scan, names[0], saved[2]), setattr(scan, names[1], saved[3])
        ens._keep = (tuple(frames), table)
        return ens.numpy() if host else ens

    def compute_envelope(self, d_output, scan=None, out=None):
        if self.is_iq:
            return iq_envelope(d_output, out=out)
        return envelope(d_output, out=out)

    def __str__(self):
        return f"DelayAndSum(MI355X, {self.setups})"


def _check_iq(bf, data):
    """complex data belong to is_iq, real data to RF: anything else is a ValueError"""
    is_complex = data.dtype.kind == "c"
    if is_complex and not bf.is_iq:
        raise ValueError(f"{type(bf).__name__}: complex (I/Q) data, but is_iq is off -- set_is_iq(True), or pass RF data")
    if bf.is_iq and not is_complex:
        raise ValueError(f"{type(bf).__name__}: is_iq is on, but the data are real -- demodulate them first (rf2iq), or set_is_iq(False)")


class _NonlinearBeamformer(DelayAndSum):
    """p-DAS / F-DMAS in the shape of DelayAndSum (DESIGN D19): beamform() runs the non-linear kernel and, unless the setup `band`
    is None, the axial band-pass.  Setup keys: DelayAndSum's, `band` ("default": centre (1 -+ probe.bandwidth / 200) around
    `_centre` x probe.central_freq; (f_lo, f_hi) in Hz; None: no filter) and `taps_half_length` (None: bandpass_taps' default)."""
    _centre = 1.0   # band centre in units of the probe's central frequency

    def __init__(self, on_gpu=True, f_number=1.0, interpolation="linear", compound="sum", band="default", taps_half_length=None,
                 is_iq=False, rx_apodization="boxcar", rx_apodization_alpha=0.5):
        super().__init__(on_gpu=on_gpu, f_number=f_number, interpolation=interpolation, compound=compound, is_iq=is_iq,
                         rx_apodization=rx_apodization, rx_apodization_alpha=rx_apodization_alpha)
        self.setups.update(band=band, taps_half_length=taps_half_length)
        self.scratch_dev = None           # a buffer for the unfiltered image (set by us_render)
        self._taps_cache = (None, None)   # (the taps' bytes, the taps as a DeviceBuffer)

    def set_is_iq(self, flag):
        if flag:
            raise NotImplementedError(f"{type(self).__name__}: is_iq is not built -- the non-linearity is defined on RF samples "
                                      "(DESIGN D19); DelayAndSum beamforms I/Q data (D20)")
        self.setups["is_iq"] = False

    def band(self, probe=None):
        """(f_lo, f_hi) in Hz, or None"""
        b = self.setups["band"]
        if b is None:
            return None
        if isinstance(b, str):
            if b != "default":
                raise ValueError(f"band must be None, 'default' or (f_lo, f_hi), got {b!r}")
            probe = probe or self.probe
            if probe is None:
                raise RuntimeError("the default band follows the probe: automatic_setup(acquisition_info, probe) has not been called")
            centre = self._centre * probe.central_freq
            return centre * (1.0 - probe.bandwidth / 200.0), centre * (1.0 + probe.bandwidth / 200.0)
        f_lo, f_hi = b
        return float(f_lo), float(f_hi)

    def filter_taps(self, scan, sound_speed, probe=None):
        """the band-pass taps [2 K + 1] (float32) for a scan, None with band=None.  ValueError when the band does not fit under the
        Nyquist frequency of the scan's depth step; the message names the step that would."""
        band = self.band(probe)
        if band is None:
            return None
        fs_ax = axial_rate(_axial_axis(scan), sound_speed)   # (a PolarScan: the rate along rho, its last axis)
        f_lo, f_hi = band
        if f_hi >= fs_ax / 2.0:
            c, dz = float(sound_speed), float(sound_speed) / (2.0 * fs_ax)
            raise ValueError(
                f"{type(self).__name__}: the band [{f_lo:.4g}, {f_hi:.4g}] Hz does not fit under the axial Nyquist frequency "
                f"{fs_ax / 2.0:.4g} Hz of a depth step of {dz:.4g} m (fs_ax = c / (2 dz)); a step below c / (4 f_hi) = "
                f"{c / (4.0 * f_hi):.4g} m would fit -- pass step= to us_render (DESIGN D19)")
        return bandpass_taps(f_lo, f_hi, fs_ax, self.setups["taps_half_length"])

    def beamform(self, d_data, scan, out=None, table=None):
        """host array in -> host array out; a DeviceBuffer in -> a DeviceBuffer out, queued (kernel, then the band-pass)"""
        data = self._checked(d_data)
        taps = self.filter_taps(scan, self.acquisition_info["sound_speed"])
        if taps is None:
            return self._request(data, scan, out, table)
        if not _is_dev(data):
            return axial_fir(self._request(data, scan, None, None), taps)
        # the taps in HBM: uploaded once per change (us_render puts its plan's copy here, with the buffer of the unfiltered image)
        key = taps.tobytes()
        if self._taps_cache[0] != key or self._taps_cache[1].ctx is not data.ctx:
            self._taps_cache = (key, _capi.DeviceBuffer.from_host(data.ctx, taps))
        scratch = self.scratch_dev if self.scratch_dev is not None and self.scratch_dev.shape == scan.shape else None
        return axial_fir(self._request(data, scan, scratch, table), self._taps_cache[1], out=out)

    def __str__(self):
        return f"{type(self).__name__}(MI355X, {self.setups})"


class Capon(DelayAndSum):
    """ultraspy's Capon in the shape of DelayAndSum (DESIGN D23): the minimum-variance beamformer on I/Q data.  Setups: DelayAndSum's,
    `l_prop` (the subarray length over the number of elements a pixel uses, [0, 0.5]) and `delta_l` (the diagonal loading over the mean
    diagonal entry of the covariance, (0, 1e3]).  `ultraspy` is absent: the two names are ultraspy's from memory, the arithmetic is this
    build's own definition (include/pbrt_hip.h, after Synnevag, Austeng and Holm 2007 / 2009), and parity with it is unpinned.  Always
    I/Q: set_is_iq(False) raises NotImplementedError; a receive window other than 'boxcar' is a ValueError of beamform() -- the method
    makes its own weights.  It takes a GridScan or a PolarScan, and compute_envelope is the modulus."""

    def __init__(self, on_gpu=True, f_number=1.0, interpolation="linear", compound="sum", l_prop=0.5, delta_l=0.01, is_iq=True,
                 rx_apodization="boxcar", rx_apodization_alpha=0.5):
        super().__init__(on_gpu=on_gpu, f_number=f_number, interpolation=interpolation, compound=compound, is_iq=is_iq,
                         rx_apodization=rx_apodization, rx_apodization_alpha=rx_apodization_alpha)
        self.setups.update(l_prop=l_prop, delta_l=delta_l)

    def set_is_iq(self, flag):
        if not flag:
            raise NotImplementedError("Capon: RF (real) data are not built -- the covariance is defined on I/Q samples (DESIGN D23); "
                                      "demodulate them first (rf2iq)")
        self.setups["is_iq"] = True

    def _request(self, data, scan, out, table):
        ai, su, dev = self.acquisition_info, self.setups, _is_dev(data)
        if su["rx_apodization"] != "boxcar":
            raise ValueError(f"Capon makes its own weights: rx_apodization must be 'boxcar', got {su['rx_apodization']!r}")
        ex = self.probe_dev if dev and self.probe_dev is not None else self.probe.das_elements
        polar, gx, gz = _scan_tables(scan, dev)
        return capon_beamform(data, ai["delays"], ex, gx, gz, ai["sampling_freq"], ai["sound_speed"], self.demod_freq(),
                              l_prop=su["l_prop"], delta_l=su["delta_l"], t0=ai.get("t0", 0.0) or 0.0, f_number=su["f_number"],
                              interpolation=su["interpolation"], compound=su["compound"], out=out, table=table, tables=polar)

    def __str__(self):
        return f"Capon(MI355X, {self.setups})"


class _CoherenceBeamformer(DelayAndSum):
    """what ShortLagSpatialCoherence and CoherenceFactor share (DESIGN D26): always I/Q, no receive window, a GridScan or a PolarScan,
    and the request through coherence_beamform by the class's kind"""
    _kind = None

    def set_is_iq(self, flag):
        if not flag:
            raise NotImplementedError(f"{type(self).__name__}: RF (real) data are not built -- the coherence is defined on I/Q samples "
                                      "(DESIGN D26); demodulate them first (rf2iq)")
        self.setups["is_iq"] = True

    def _request(self, data, scan, out, table):
        ai, su, dev = self.acquisition_info, self.setups, _is_dev(data)
        if su["rx_apodization"] != "boxcar":
            raise ValueError(f"{type(self).__name__} takes no receive window: rx_apodization must be 'boxcar', got {su['rx_apodization']!r}")
        ex = self.probe_dev if dev and self.probe_dev is not None else self.probe.das_elements
        polar, gx, gz = _scan_tables(scan, dev)
        return coherence_beamform(data, ai["delays"], ex, gx, gz, ai["sampling_freq"], ai["sound_speed"], self.demod_freq(),
                                  kind=self._kind, lag_prop=su.get("lag_prop", 0.3), half_kernel=su.get("half_kernel", 0),
                                  gamma=su.get("gamma", 1.0), t0=ai.get("t0", 0.0) or 0.0, f_number=su["f_number"],
                                  interpolation=su["interpolation"], compound=su["compound"], out=out, table=table, tables=polar)

    def __str__(self):
        return f"{type(self).__name__}(MI355X, {self.setups})"


class ShortLagSpatialCoherence(_CoherenceBeamformer):
    """Short-lag spatial coherence (Lediju, Trahey, Byram, Dahl 2011) in the shape of DelayAndSum (DESIGN D26).  NOT one of ultraspy's
    beamformers: the class, its setup names and the arithmetic are this build's own (include/pbrt_hip.h "spatial coherence").  Setups:
    DelayAndSum's, `lag_prop` (the lags summed over the number of elements a pixel uses, (0, 1]) and `half_kernel` (the axial kernel is
    2 half_kernel + 1 samples, 0 .. 4).  Always I/Q; no receive window; a GridScan or a PolarScan.  The image is float32 and already a
    detection image: compute_envelope returns it as it is, and beamform_packet (whose ensemble is complex) is a ValueError."""
    _kind = "slsc"
    real_image = True   # (us_render: the image goes straight into the envelope buffer)

    def __init__(self, on_gpu=True, f_number=1.0, interpolation="linear", compound="sum", lag_prop=0.3, half_kernel=1, is_iq=True,
                 rx_apodization="boxcar", rx_apodization_alpha=0.5):
        super().__init__(on_gpu=on_gpu, f_number=f_number, interpolation=interpolation, compound=compound, is_iq=is_iq,
                         rx_apodization=rx_apodization, rx_apodization_alpha=rx_apodization_alpha)
        self.setups.update(lag_prop=lag_prop, half_kernel=half_kernel)

    def beamform_packet(self, d_data, scan, out=None):
        raise ValueError("ShortLagSpatialCoherence.beamform_packet: the ensemble buffer is complex and an SLSC image is real -- "
                         "beamform the frames one by one")

    def compute_envelope(self, d_output, scan=None, out=None):
        """the image itself: SLSC is a detection image already (`out`: the image is copied there)"""
        if out is None or out is d_output:
            return d_output
        if _is_dev(out):
            raise ValueError("ShortLagSpatialCoherence.compute_envelope: beamform(..., out=) writes the image where it is wanted")
        np.copyto(out, d_output.numpy() if _is_dev(d_output) else d_output)
        return out


class CoherenceFactor(_CoherenceBeamformer):
    """Delay-and-sum weighted by the coherence factor (Mallart and Fink 1994; Hollman, Rigby, O'Donnell 1999) in the shape of DelayAndSum
    (DESIGN D26).  NOT one of ultraspy's beamformers: the class, its setup name and the arithmetic are this build's own
    (include/pbrt_hip.h "spatial coherence").  Setups: DelayAndSum's and `gamma` (the exponent of the weight, [0, 4]; 0 is delay-and-sum).
    Always I/Q; no receive window; a GridScan or a PolarScan; compute_envelope is the modulus."""
    _kind = "cf"

    def __init__(self, on_gpu=True, f_number=1.0, interpolation="linear", compound="sum", gamma=1.0, is_iq=True,
                 rx_apodization="boxcar", rx_apodization_alpha=0.5):
        super().__init__(on_gpu=on_gpu, f_number=f_number, interpolation=interpolation, compound=compound, is_iq=is_iq,
                         rx_apodization=rx_apodization, rx_apodization_alpha=rx_apodization_alpha)
        self.setups.update(gamma=gamma)


class PDelayAndSum(_NonlinearBeamformer):
    """p-DAS (Polichetti et al. 2018): per transmission the signed p-th roots of the delayed samples are summed and the sum is raised
    back to the p-th power, sign kept; band-pass around the carrier.  1 <= p <= 8; p = 1 is DelayAndSum."""
    _method, _centre = "pdas", 1.0

    def __init__(self, p=2.0, **kw):
        super().__init__(**kw)
        self.setups["p"] = p


class FilteredDelayMultiplyAndSum(_NonlinearBeamformer):
    """F-DMAS (Matrone et al. 2015): per transmission the sum over element pairs of the signed square roots' products, then the
    band-pass around TWICE the carrier, where the products of the pairs put the signal."""
    _method, _centre = "fdmas", 2.0


# ---- us_render in stages: a request record, one statement of the chain, a plan that owns its buffers and its recording ------------
@dataclasses.dataclass
class _UsRenderRequest:
    """One us_render call as its stages read it: the integrator, the arguments and what follows from them alone.  Made by
    _us_render_request without a device; every ValueError of us_render is raised there."""
    integ: object
    A: int
    E: int
    T: int
    x_scan: np.ndarray          # the axes of the display image                                        (USMain.py:193-194)
    z_scan: np.ndarray
    scan: object                # what the beamformer runs on: a GridScan on the axes, or the PolarScan of scan="polar"
    polar: bool
    theta_range: tuple          # (polar) the sector's angles as floats, else None
    probe: Probe
    bf: DelayAndSum             # the beamformer that runs: the caller's, a copy of it that beamforms I/Q data, or a DelayAndSum
    iq: bool
    D: int                      # decimation (1 without iq)
    f_demod: float              # (iq) the frequency rf2iq demodulates at, else None
    lp: np.ndarray              # (iq) rf2iq's low-pass taps, else None
    taps: np.ndarray            # (p-DAS / F-DMAS with a band) the band-pass taps of this scan, else None
    fs_img: float               # the rate of the data the beamformer is given
    gaussian: bool              # the pulse is applied after the acquisition (pulse_model 'gaussian')
    seq: dict
    seed: object
    paths_per_ray: object
    dynamic_range: float

    def info(self, delays):
        """the acquisition_info of the beamformer (USMain.py:138-172) for delays on the host or in HBM"""
        return {"sampling_freq": self.fs_img, "t0": 0, "prf": None, "signal_duration": None, "delays": delays,
                "sound_speed": self.integ.sound_speed, "sequence_elements": self.seq}

    def plan_key(self, cx):
        """what the buffers of a _RenderPlan and their constant contents depend on"""
        return (self.A, self.E, self.T,                                  # the shapes of d_channel, d_rf, d_tx, d_iq and d_table
                float(self.integ.pitch),                                 # d_ex: the element positions of a linear array
                self.x_scan.tobytes(), self.z_scan.tobytes(),            # d_x, d_z and the shapes of d_bf, d_env, d_img
                self.gaussian,                                           # d_rf exists
                id(cx),                                                  # the context that owns the memory
                self.probe.geometry_type, self.probe.radius, self.probe.opening_angle,   # d_ex: positions, or an arc's element table
                None if self.taps is None else self.taps.tobytes(),      # d_taps, and d_nl exists
                self.iq, self.D if self.iq else 1,                       # d_iq, d_bf_iq exist; the decimated length of d_iq
                self.bf.real_image,                                      # d_bf_iq does not exist: the image goes to d_env (D26)
                None if self.lp is None else self.lp.tobytes(),          # d_iq_taps
                self.theta_range if self.polar else None,                # d_px, d_pz: the sector's angles ...
                len(self.scan.thetas) if self.polar else None)           # ... and their count: the shapes of d_bf, d_env_sec

    def graph_key(self, scene):
        """what the queued calls depend on besides the CONTENTS of device memory: a recording of them stands for exactly this key.
        (The reference's loop, USMain.py:262-289, repeats one key 100 times and changes a material's roughness in between:
        pbrt_scene_update_material writes device memory, the replay sees it.)"""
        integ, h = self.integ, scene.device().handle
        return (bytes(integ.us_params(scene, integ.quirks)),             # the acquisition's parameter block, by value in the launch
                getattr(h, "value", h),                                  # the device scene it traces
                int(integ.seed if self.seed is None else self.seed) & 0xFFFFFFFF,   # an argument of the acquisition
                int(self.paths_per_ray if self.paths_per_ray is not None else integ.paths_per_ray),   # one more
                float(self.dynamic_range),                               # an argument of the log compression
                type(self.bf).__name__,                                  # which beamform kernel runs, and whether a band-pass follows
                tuple(sorted(self.bf.setups.items())),                   # its parameter block: f-number, interpolation, window, p, band
                float(integ.pulse_sigma) if self.gaussian else None,     # an argument of apply_pulse
                (self.D, self.f_demod) if self.iq else None,             # arguments of rf2iq and of the I/Q beamformer
                (self.theta_range, self.scan.shape) if self.polar else None)   # the parameter block of scan_convert


def _request_scan(x_range, z_range, step, scan, theta_range, convex, opening_angle):
    """(x_scan, z_scan, the scan the beamformer runs on, theta_range as floats or None) of a us_render call"""
    x_scan = np.arange(x_range[0], x_range[1] + step, step)                                            # :193
    z_scan = np.arange(z_range[0], z_range[1] + step, step)                                            # :194
    if scan not in ("grid", "polar"):
        raise ValueError(f"us_render: scan must be 'grid' or 'polar', got {scan!r}")
    if scan == "grid":
        if theta_range is not None:
            raise ValueError("us_render: theta_range belongs to scan='polar'")
        return x_scan, z_scan, GridScan(x_scan, z_scan), None
    if theta_range is None and convex:      # the arc's own opening angle
        theta_range = (-np.radians(float(opening_angle)) / 2.0, np.radians(float(opening_angle)) / 2.0)
    elif theta_range is None:               # the x-range seen from the deepest z
        theta_range = (np.arctan(x_range[0] / z_range[1]), np.arctan(x_range[1] / z_range[1]))
    theta_range = (float(theta_range[0]), float(theta_range[1]))
    rhos = z_scan   # measured from the origin of the probe's frame, as the scan's z is
    return x_scan, z_scan, PolarScan(rhos, np.linspace(theta_range[0], theta_range[1], polar_n_theta(rhos[-1], theta_range, step))), theta_range


def _request_iq(integ, bf, iq, decimation):
    """(the beamformer that runs, iq, D, f_demod, lp): the rules of the I/Q chain (DESIGN D20)"""
    iq, D = bool(iq) or bf.is_iq, int(decimation)      # (a beamformer that has is_iq set selects the I/Q chain by itself)
    if not iq:
        if D != 1:
            raise ValueError("us_render: decimation belongs to the I/Q chain (iq=True)")
        return bf, False, D, None, None
    if not bf.is_iq:
        # the caller's beamformer keeps its setups: this call works on a copy of it that beamforms I/Q data (p-DAS / F-DMAS:
        # NotImplementedError)
        bf = copy.copy(bf)
        bf.setups = dict(bf.setups)
        bf.set_is_iq(True)
    # the frequency rf2iq demodulates at is the one the walk turns back by: the setup `demod_freq`, else the integrator's
    f_demod = float(integ.frequency if bf.setups["demod_freq"] is None else bf.setups["demod_freq"])
    if not 1 <= D <= RF2IQ_MAX_DECIMATION or D != decimation:
        raise ValueError(f"us_render: decimation must be an integer in [1, {RF2IQ_MAX_DECIMATION}], got {decimation}")
    if -(-integ.time_samples // D) < 2:
        raise ValueError(f"us_render: {integ.time_samples} samples decimated by {D} leave fewer than two")
    # rf2iq's default low-pass (bandwidth = 100): refused here, before anything is acquired, when the decimation does not fit
    return bf, True, D, f_demod, _rf2iq_lowpass(f_demod, float(integ.fs), 100, D)


def _us_render_request(integ, x_range, z_range, dynamic_range, step, seed, paths_per_ray, beamformer, iq, decimation, scan, theta_range):
    """the request of a us_render call; its refusals in the order scan, probe, I/Q rules, band"""
    A, E, T = integ.n_angles, integ.n_elements, integ.time_samples
    lam = integ.sound_speed / integ.frequency
    step = step or lam / 4                                                                             # :189-191
    convex = float(getattr(integ, "radius", 0.0)) != 0.0
    x_scan, z_scan, scan, theta_range = _request_scan(x_range, z_range, step, scan, theta_range, convex, getattr(integ, "opening_angle", 0.0))
    if convex:  # the curved array (DESIGN D18): element table instead of positions, the *_probe beamformer
        probe = build_probe("convex", E, integ.pitch, integ.frequency, 70, radius=integ.radius, opening_angle=integ.opening_angle)
    else:
        probe = build_probe("linear", E, integ.pitch, integ.frequency, 70)                             # :130-136
    bf, iq, D, f_demod, lp = _request_iq(integ, beamformer or DelayAndSum(on_gpu=True), iq, decimation)
    # (p-DAS / F-DMAS: the band-pass taps of this scan -- refused here, before anything is acquired, when the band does not fit
    # under the Nyquist frequency of the depth step: the reference's lambda / 4 grid puts that AT the carrier, DESIGN D19)
    taps = bf.filter_taps(scan, integ.sound_speed, probe) if isinstance(bf, _NonlinearBeamformer) else None
    seq = {"emitted": np.tile(np.arange(E), (A, 1)), "received": np.tile(np.arange(E), (A, 1))}
    return _UsRenderRequest(integ=integ, A=A, E=E, T=T, x_scan=x_scan, z_scan=z_scan, scan=scan, polar=isinstance(scan, PolarScan),
                            theta_range=theta_range, probe=probe, bf=bf, iq=iq, D=D, f_demod=f_demod, lp=lp, taps=taps,
                            fs_img=integ.fs / D if iq else integ.fs, gaussian=integ.pulse_model == "gaussian", seq=seq, seed=seed,
                            paths_per_ray=paths_per_ray, dynamic_range=dynamic_range)


class _HostBuffers:
    """the buffers of the chain in its host form: none -- every step hands back a host array of its own"""
    d_rf = d_iq_taps = d_iq = d_bf = d_bf_iq = d_table = d_env_sec = d_env = d_img = d_x = d_z = None


def _form_image(rq, data, delays, b):
    """The image-formation chain of us_render, stated once: channel data -> [pulse] -> [rf2iq] -> beamform -> envelope or modulus ->
    [scan_convert] -> log compression -> (display image [nx, nz], envelope [nx, nz]).  data and delays in HBM: the device forms, queued,
    on the buffers `b` of a _RenderPlan.  On the host (b: _HostBuffers) the host-pointer forms: the pulse was applied inside the
    acquisition, the data get the frame axis USMain.py hands on (reader.data) and the envelope is brought to float32."""
    dev, integ, bf, scan = _is_dev(data), rq.integ, rq.bf, rq.scan
    if rq.gaussian and dev:                                                                            # f-3: carrier on the device
        data = apply_pulse(data, integ.fs, integ.frequency, integ.pulse_sigma, out=b.d_rf)
    bf.automatic_setup(rq.info(delays), rq.probe)                                                      # :175
    if rq.iq:                                                                                          # D20: baseband, then complex DAS
        data = rf2iq(data, rq.f_demod, integ.fs, decimation=rq.D, taps=b.d_iq_taps if dev else rq.lp, out=b.d_iq)
    d_env = b.d_env_sec if rq.polar else b.d_env
    # (D26: a beamformer with a real image -- SLSC -- writes its detection image where the envelope goes, and there is no envelope step)
    img = bf.beamform(data if dev else data[np.newaxis], scan, out=d_env if bf.real_image else b.d_bf_iq if rq.iq else b.d_bf,
                      table=b.d_table)                                                                 # :204
    env = img if bf.real_image else bf.compute_envelope(img, scan, out=d_env)                          # :205 (I/Q: the modulus)
    if not dev:
        env = env.astype(np.float32)                                                                   # :207
    if rq.polar:                                                                                       # D21: sector -> the grid
        env = scan_convert(env, scan, *((b.d_x, b.d_z) if dev else (rq.x_scan, rq.z_scan)), fill=0.0, out=b.d_env)
    return log_compress(env, rq.dynamic_range, out=b.d_img), env                                       # :210-218


def _render_host(scene, rq):
    """device_resident=False: the acquisition and every step of the chain through the host-pointer entry points"""
    integ = rq.integ
    if rq.seed is not None or rq.paths_per_ray is not None:
        integ.channel_buf = integ._acquire(scene, integ.quirks, paths_per_ray=rq.paths_per_ray, seed=rq.seed)
    else:
        integ.simulate_acquisition_parallel(scene)                                                     # :99
    data = np.asarray(integ.channel_buf, dtype=np.float32).reshape(rq.A, rq.E, rq.T)                   # :118
    delays = np.asarray(integ.transmission_delays_buf, dtype=np.float32).reshape(rq.A, rq.E)           # :121
    display, bmode = _form_image(rq, data, delays, _HostBuffers)
    return display.T, bmode, (rq.x_scan, rq.z_scan)                                                    # :221


class _RenderPlan:
    """Device buffers of one us_render configuration (_UsRenderRequest.plan_key: acquisition shape, scan grid, chain): allocated once,
    reused by every call of the reference's loop (USMain.py:262-289 calls us_render 50 times on one scene), with the state that goes
    with their contents -- the delays and the sound speed d_tx and d_table were made with, and the recording.
    The recording: from the third call in a row with one _UsRenderRequest.graph_key on, the queued calls are replayed from it
    (pbrt_ctx_record_begin / pbrt_graph_launch: one submission instead of eleven; same kernels, same bits).  A call runs replay(), and
    queue() where that says no; queue() records the chain at the second call in a row with a key, when the workspace is warm.
    graph_key: the key `graph` stands for; warm_key: that of the last queued call; no_graph_key: one whose chain cannot be recorded."""

    def __init__(self, cx, rq, key):
        A, E, T = rq.A, rq.E, rq.T
        self.key, self.cx = key, cx
        self.d_channel = _capi.DeviceBuffer(cx, (A, E, T))
        self.d_rf = _capi.DeviceBuffer(cx, (A, E, T)) if rq.gaussian else None
        self.d_tx = _capi.DeviceBuffer(cx, (A, E))
        self.tx_host = self.table_c = None   # the delays d_tx holds, the sound speed d_table was made with
        self.d_ex = _capi.DeviceBuffer.from_host(cx, _capi.f32(rq.probe.das_elements))
        self.d_x = _capi.DeviceBuffer.from_host(cx, _capi.f32(rq.x_scan))
        self.d_z = _capi.DeviceBuffer.from_host(cx, _capi.f32(rq.z_scan))
        # polar (a PolarScan, DESIGN D21): the beamformer's buffers have the sector's shape, d_px / d_pz are its pixel tables, d_env_sec
        # its envelope; d_env is then the scan-converted envelope on the Cartesian grid, which d_img always has
        self.d_px = self.d_pz = self.d_env_sec = None
        gx, gz = len(rq.x_scan), len(rq.z_scan)
        nx, nz = rq.scan.shape
        if rq.polar:
            px, pz = rq.scan.pixels()
            self.d_px, self.d_pz = _capi.DeviceBuffer.from_host(cx, px), _capi.DeviceBuffer.from_host(cx, pz)
            self.d_env_sec = _capi.DeviceBuffer(cx, (nx, nz))
        self.d_bf = _capi.DeviceBuffer(cx, (nx, nz))
        self.d_env = _capi.DeviceBuffer(cx, (gx, gz))
        self.d_img = _capi.DeviceBuffer(cx, (gx, gz))
        self.d_table = _capi.DeviceBuffer(cx, (A, nx, nz), np.float64)   # first-arrival times of this scan (das_first_arrival)
        # p-DAS / F-DMAS with a band: the band-pass taps, and the image before the filter
        self.d_taps = _capi.DeviceBuffer.from_host(cx, rq.taps) if rq.taps is not None else None
        self.d_nl = _capi.DeviceBuffer(cx, (nx, nz)) if rq.taps is not None else None
        # the I/Q chain: the low-pass taps, the demodulated channel data and the complex image
        self.d_iq_taps = self.d_iq = self.d_bf_iq = None
        if rq.iq:
            self.d_iq_taps = _capi.DeviceBuffer.from_host(cx, rq.lp)
            self.d_iq = _capi.DeviceBuffer(cx, (A, E, -(-T // rq.D)), np.complex64)
            self.d_bf_iq = None if rq.bf.real_image else _capi.DeviceBuffer(cx, (nx, nz), np.complex64)   # (D26: a real image goes to d_env)
        self.graph = self.graph_key = self.warm_key = self.no_graph_key = None

    @classmethod
    def of(cls, cx, rq):
        """the plan the integrator keeps, or a new one where the request's plan key is another; bound to the request"""
        key = rq.plan_key(cx)
        plan = getattr(rq.integ, "_render_plan", None)
        if plan is None or plan.key != key:
            plan = rq.integ._render_plan = cls(cx, rq, key)
        plan.bind(rq)
        return plan

    def bind(self, rq):
        """the tables this plan holds in HBM, handed to the request's scan and beamformer, which use them where the data is in HBM"""
        if rq.polar:
            rq.scan.d_px, rq.scan.d_pz = self.d_px, self.d_pz
        else:
            rq.scan.d_x, rq.scan.d_z = self.d_x, self.d_z
        rq.bf.probe_dev = self.d_ex
        if isinstance(rq.bf, _NonlinearBeamformer):
            rq.bf.scratch_dev = self.d_nl
            if rq.taps is not None:
                rq.bf._taps_cache = (rq.taps.tobytes(), self.d_taps)

    def refresh_delays(self, delays, sound_speed):
        """d_tx and d_table for the delays [A, E] an acquisition handed back and the integrator's sound speed.  The scan's first-arrival
        times follow the delays, the sound speed and the grid: made again only when those change (never, in the loop of
        USMain.py:262-289; a single 0 degree angle has zero delays at every sound speed), and the recording, which reads both, is
        dropped with them."""
        if self.tx_host is not None and np.array_equal(self.tx_host, delays) and self.table_c == float(sound_speed):
            return
        self.d_tx.upload(delays)
        self.tx_host, self.table_c = delays.copy(), float(sound_speed)
        if self.d_px is not None:
            scan_first_arrival(self.d_tx, self.d_ex, self.d_px, self.d_pz, sound_speed, out=self.d_table)
        else:
            das_first_arrival(self.d_tx, self.d_ex, self.d_x, self.d_z, sound_speed, out=self.d_table)
        self.graph = self.graph_key = self.warm_key = None

    def replay(self, rq, gkey) -> bool:
        """launch the recording if it stands for gkey, and leave on the integrator and the beamformer what the queued calls would have;
        False: nothing was submitted"""
        if gkey is None or self.graph is None or self.graph_key != gkey:
            return False
        try:
            self.graph.launch()
        except RuntimeError:
            # stale (the context freed or replaced memory the recording refers to): the caller queues the chain the plain way.
            # ADVICE.md finding 1: every failure of the launch lands here, a deferred device error of the queued work included.
            self.graph = self.graph_key = None
            return False
        rq.integ.transmission_delays_buf = self.tx_host.reshape(-1).copy()
        rq.integ._ray_count = None
        rq.integ._stats_ctx = self.cx
        rq.bf.automatic_setup(rq.info(self.d_tx), rq.probe)
        return True

    def _acquire(self, scene, rq):
        integ = rq.integ
        integ._acquire(scene, integ.quirks, paths_per_ray=rq.paths_per_ray, seed=rq.seed, out_dev=self.d_channel.ptr, pulse=False,
                       queue=True)                                                                     # :99 (queued, not waited for)

    def queue(self, scene, rq, gkey) -> float:
        """queue the acquisition and the chain call by call -> the time at which the acquisition was queued.  At the second call in a
        row with gkey the chain is queued once more inside a recording, for the calls that follow."""
        self._acquire(scene, rq)
        t1 = time.perf_counter()
        self.refresh_delays(np.asarray(rq.integ.transmission_delays_buf, dtype=np.float32).reshape(rq.A, rq.E), rq.integ.sound_speed)   # :121
        _form_image(rq, self.d_channel, self.d_tx, self)
        if gkey is not None and self.warm_key == gkey and self.no_graph_key != gkey:
            try:
                with self.cx.record() as rec:
                    self._acquire(scene, rq)
                    _form_image(rq, self.d_channel, self.d_tx, self)
                self.graph, self.graph_key = rec.graph, gkey
            except RuntimeError:
                # (a chain that cannot be recorded -- e.g. a pass whose size follows the free device memory of the moment -- is
                # queued call by call from now on, not tried again at every call)
                self.graph = self.graph_key = None
                self.no_graph_key = gkey
        self.warm_key = gkey
        return t1


def us_render(scene, x_range=(-0.04, 0.04), z_range=(0.001, 0.05), dynamic_range=60.0, step=None, seed=None,
              paths_per_ray=None, beamformer=None, device_resident=True, return_bmode=True, timing=None, graph=True,
              on_device=False, iq=False, decimation=1, scan="grid", theta_range=None):
    """The reference's us_render (USMain.py:93-224) without the plotting: acquisition -> DAS -> envelope -> log
    compression.  Returns (display_image [nz, nx] in [0, 1], bmode envelope [nx, nz] (None with return_bmode=False),
    (x_scan, z_scan)).

    device_resident (default): the channel buffer never leaves HBM -- pbrt_us_acquire_dev writes it, the image-formation
    kernels are queued behind it on the context's stream (*_dev entry points, ABI 5), and ONE copy brings the display image to
    the host (a second one the envelope, if asked for).  `integrator.channel_buf` is fetched only if somebody reads it.
    device_resident=False is round 4's path through the host-pointer entry points (every step up and down PCIe), kept for the
    A/B and the bit-for-bit test.  timing: a dict that receives host wall-clock seconds (acquire, queue, wait_copy).
    graph (default): from the third call in a row with the same arguments on, the queued calls are replayed from a recording
    (_RenderPlan: one submission, same kernels, same bits); graph=False, or a context that profiles (Context.set_profiling), queues
    them one by one.
    on_device: nothing is copied and nothing waits -- the display image and the envelope come back as DeviceBuffers [nx, nz] (the
    reference's display image is their transpose), still being written by the queued kernels; a caller that keeps its loss on
    the GPU (USMain.py:5 imports torch: `torch.as_tensor(buf, device="cuda")` through __cuda_array_interface__) calls
    scene.device().ctx.synchronize() before it reads them.  The buffers belong to the integrator's render plan: the next
    us_render with the same scan overwrites them.
    iq: the I/Q chain (DESIGN D20) -- acquisition -> [pulse] -> rf2iq at the integrator's frequency, decimated by `decimation` ->
    I/Q delay-and-sum -> modulus -> log compression, on every path above.  The envelope is a modulus per pixel, so `step` is free
    of the carrier (lambda / 2, a coarse loss grid) and nz has no limit.  A `beamformer` of the caller keeps its setups: the call
    works on a copy of it that beamforms I/Q data; one that has is_iq set selects this chain by itself, and its setup `demod_freq`, where set,
    is the frequency rf2iq demodulates at (default: the integrator's).
    scan: "grid" (the reference's GridScan) or "polar" (DESIGN D21) -- the beamformer runs on a PolarScan around the origin of the
    probe's frame, rhos = np.arange(z_range[0], z_range[1] + step, step), thetas over `theta_range` (radians; default: +- opening_angle
    / 2 of a curved array, atan(x_range / z_range[1]) of a linear one) with the smallest count that keeps rho_max * dtheta <= step
    (polar_n_theta); the envelope (or modulus) is taken along rho, the propagation direction of every ray, and scan_convert brings it
    onto the Cartesian grid of "grid" (0 outside the sector) before the log compression.  The display image, the returned envelope
    and the axes have the shapes "grid" gives; every path above runs this chain."""
    rq = _us_render_request(scene.integrator(), x_range, z_range, dynamic_range, step, seed, paths_per_ray, beamformer, iq, decimation,
                            scan, theta_range)
    if not device_resident:
        return _render_host(scene, rq)
    cx = scene.device().ctx
    plan = _RenderPlan.of(cx, rq)
    t0 = time.perf_counter()
    gkey = rq.graph_key(scene) if graph and not getattr(cx, "profiling", False) else None
    replayed = plan.replay(rq, gkey)
    t1 = time.perf_counter() if replayed else plan.queue(scene, rq, gkey)
    rq.integ._set_device_channel(plan.d_rf if rq.gaussian else plan.d_channel)
    t2 = time.perf_counter()
    if on_device:
        display, bmode = plan.d_img, (plan.d_env if return_bmode else None)
    else:
        display = plan.d_img.numpy().T                                                                 # :221  (the one copy)
        bmode = plan.d_env.numpy() if return_bmode else None
    if timing is not None:
        timing.update(acquire=t1 - t0, queue=t2 - t1, wait_copy=0.0 if on_device else time.perf_counter() - t2, replayed=replayed)
    return display, bmode, (rq.x_scan, rq.z_scan)


# ---- colour and power Doppler on an ensemble of I/Q frames (DESIGN D24, include/pbrt_hip.h) -----------------------------------------
# `ultraspy` is absent, as everywhere in this file: the names follow its Doppler module from memory (apply_wall_filter,
# get_color_doppler_map, get_power_doppler_map), the arithmetic is this build's own definition and parity with it is unpinned.
DOPPLER_MAX_FRAMES, DOPPLER_MAX_DEGREE, DOPPLER_MAX_K = _capi.DOPPLER_MAX_FRAMES, _capi.DOPPLER_MAX_DEGREE, _capi.DOPPLER_MAX_K
_SMOOTHING = {"boxcar": _capi.DOPPLER_BOXCAR, "hamming": _capi.DOPPLER_HAMMING}


def nyquist_velocity(sound_speed, prf, demod_freq) -> float:
    """c prf / (4 f): the axial velocity whose echo turns by pi between two pulses, the largest a colour map can tell from its alias"""
    c, prf, f = float(sound_speed), float(prf), float(demod_freq)
    if not (math.isfinite(c * prf / f if f else math.nan) and c > 0.0 and prf > 0.0 and f > 0.0):
        raise ValueError(f"nyquist_velocity needs sound_speed, prf and demod_freq finite and > 0, got {sound_speed}, {prf}, {demod_freq}")
    return c * prf / (4.0 * f)


def _checked_ensemble_length(n_frames) -> int:
    N = int(n_frames)
    if N != n_frames or not 2 <= N <= DOPPLER_MAX_FRAMES:
        raise ValueError(f"an ensemble has 2 to {DOPPLER_MAX_FRAMES} frames, got {n_frames}")
    return N


def _wall_degree(wall_filter, degree, N):
    """the degree of the polynomial regression filter a call names, None for "none"; ValueError for what the library would refuse"""
    if wall_filter not in ("none", "mean", "poly"):
        raise ValueError(f"wall_filter must be 'none', 'mean' or 'poly', got {wall_filter!r}")
    if wall_filter == "none":
        return None
    d = 0 if wall_filter == "mean" else degree
    if isinstance(d, bool) or int(d) != d or not 0 <= int(d) <= DOPPLER_MAX_DEGREE:
        raise ValueError(f"the degree of the wall filter must be an integer in [0, {DOPPLER_MAX_DEGREE}], got {degree!r}")
    if int(d) + 1 >= N:
        raise ValueError(f"a wall filter of degree {int(d)} leaves nothing of {N} frames: degree + 1 < frames is required")
    return int(d)


def wall_basis(n_frames, degree) -> np.ndarray:
    """The table pbrt_doppler_autocorr takes: float32 [degree + 1, n_frames], row k the k-th member of the orthonormal basis of the
    polynomials of degree <= `degree` on the slow-time points 0 .. n_frames - 1 (row 0 constant; the leading coefficient of every row
    positive), made in float64 -- a QR factorisation of the centred Vandermonde matrix -- and rounded once.  The wall filter is
    y = x - Q^T (Q x); degree 0 is mean removal."""
    N = _checked_ensemble_length(n_frames)
    d = _wall_degree("poly", degree, N)
    t = (np.arange(N, dtype=np.float64) - (N - 1) / 2.0) / ((N - 1) / 2.0)
    q, r = np.linalg.qr(np.vander(t, d + 1, increasing=True))
    return np.ascontiguousarray((q * np.sign(np.diag(r))[None, :]).T.astype(np.float32))


def _wall_basis_dev(cx, N, d):
    """wall_basis(N, d) in HBM, uploaded once per context: a queued call neither allocates nor waits"""
    cache = cx.__dict__.setdefault("_wall_basis_dev", {})
    if (N, d) not in cache:
        cache[(N, d)] = _capi.DeviceBuffer.from_host(cx, wall_basis(N, d))
    return cache[(N, d)]


def _checked_smoothing(smoothing, kernel):
    if smoothing not in _SMOOTHING:
        raise ValueError(f"smoothing must be one of {tuple(_SMOOTHING)}, got {smoothing!r}")
    try:
        kx, kz = kernel
        ok = all(not isinstance(k, bool) and int(k) == k and 1 <= int(k) <= DOPPLER_MAX_K and int(k) % 2 == 1 for k in (kx, kz))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"kernel must be two odd sizes (kx, kz) in [1, {DOPPLER_MAX_K}], got {kernel!r}")
    return _SMOOTHING[smoothing], int(kx), int(kz)


def _checked_ensemble(frames):
    """an ensemble [frames, nx, nz] as the autocorrelation takes it: a complex DeviceBuffer, or a host array as complex64"""
    if _is_dev(frames):
        if frames.dtype.kind != "c":
            raise ValueError(f"the ensemble must be complex64 (beamformed I/Q frames), got a {frames.dtype} DeviceBuffer")
    elif not np.iscomplexobj(frames):
        raise ValueError("the ensemble must be complex (beamformed I/Q frames)")
    else:
        frames = np.ascontiguousarray(frames, dtype=np.complex64)
    if len(frames.shape) != 3:
        raise ValueError(f"the ensemble must be [frames, nx, nz], got {list(frames.shape)}")
    _checked_ensemble_length(frames.shape[0])
    return frames


def doppler_autocorr(frames, wall_filter="none", degree=1, out=None):
    """Slow-time autocorrelation of an ensemble frames [N, nx, nz] complex64 (frame n = pulse n; beamform_packet makes one) ->
    acf [3, nx, nz] float32, the planes Re R1, Im R1 and R0 (pbrt_doppler_autocorr, DESIGN D24): R1 = sum_n y[n + 1] conj(y[n]),
    R0 = mean |y[n]|^2 of the wall-filtered samples y.  wall_filter: "none", "mean" (the slow-time mean is removed: ultraspy's 'mean')
    or "poly" (the polynomial regression filter of `degree` 0 .. 3; degree + 1 < N).  The filter is part of this step and not one of
    its own (ultraspy's apply_wall_filter): the filtered ensemble is never written.  A host array in gives a host array out; a complex
    DeviceBuffer in gives a DeviceBuffer out (`out`, or a new one), queued."""
    frames = _checked_ensemble(frames)
    N, nx, nz = (int(v) for v in frames.shape)
    d = _wall_degree(wall_filter, degree, N)
    par = _capi.DopplerParams()
    par.n_frames, par.nx, par.nz = N, nx, nz
    par.wall_degree = _capi.DOPPLER_WALL_NONE if d is None else d
    par.kx = par.kz = 1
    par.window, par.nyquist_velocity = _capi.DOPPLER_BOXCAR, 1.0
    q = None if d is None else _wall_basis_dev(frames.ctx, N, d) if _is_dev(frames) else wall_basis(N, d)
    return _step("pbrt_doppler_autocorr", frames, (C.byref(par), frames, q), (3, nx, nz), np.float32, out, "out must hold 3 * nx * nz float32")


def doppler_maps(acf, nyquist_velocity, smoothing="hamming", kernel=(1, 1), out=None):
    """acf [3, nx, nz] (doppler_autocorr) -> (velocity [nx, nz], amplitude [nx, nz]) float32 (pbrt_doppler_maps, DESIGN D24): the
    three planes smoothed by a separable `smoothing` window ("boxcar" / "hamming") of kernel = (kx, kz) pixels, odd and at most 15,
    zero outside the image; velocity = nyquist_velocity * arg(R1) / pi -- NEGATIVE for a target that moves away from the probe --
    and amplitude = sqrt(R0).  A host array in gives host arrays out; a DeviceBuffer in gives DeviceBuffers out (`out` = (velocity,
    amplitude), or new ones), queued."""
    window, kx, kz = _checked_smoothing(smoothing, kernel)
    nyq = float(nyquist_velocity)
    if not (math.isfinite(nyq) and nyq > 0.0):
        raise ValueError(f"nyquist_velocity must be finite and > 0, got {nyquist_velocity!r}")
    dev = _is_dev(acf)
    if not dev:
        acf = _capi.f32(np.asarray(acf))
    if len(acf.shape) != 3 or acf.shape[0] != 3 or (dev and acf.dtype != np.float32):
        raise ValueError(f"acf must be float32 [3, nx, nz], got {acf.dtype} {list(acf.shape)}")
    nx, nz = int(acf.shape[1]), int(acf.shape[2])
    par = _capi.DopplerParams()
    par.n_frames, par.nx, par.nz, par.wall_degree = 2, nx, nz, _capi.DOPPLER_WALL_NONE
    par.kx, par.kz, par.window, par.nyquist_velocity = kx, kz, window, nyq
    if not dev:
        cx, vel, amp = _capi.default_context(), np.empty((nx, nz), np.float32), np.empty((nx, nz), np.float32)
        cx.check(cx.lib.pbrt_doppler_maps(cx.handle, C.byref(par), acf.ctypes.data, vel.ctypes.data, amp.ctypes.data), "pbrt_doppler_maps")
        return vel, amp
    cx = acf.ctx
    vel, amp = out if out is not None else (_capi.DeviceBuffer(cx, (nx, nz)), _capi.DeviceBuffer(cx, (nx, nz)))
    if not (_is_dev(vel) and _is_dev(amp)) or vel.nbytes != nx * nz * 4 or amp.nbytes != nx * nz * 4:
        raise ValueError("out must be two DeviceBuffers that hold nx * nz float32 each")
    cx.check(cx.lib.pbrt_doppler_maps_dev(cx.handle, C.byref(par), acf.ptr, vel.ptr, amp.ptr), "pbrt_doppler_maps_dev")
    vel._keep = amp._keep = (acf,)
    return vel, amp


def get_color_doppler_map(frames, nyquist_velocity, wall_filter="none", degree=1, smoothing="hamming", kernel=(1, 1)):
    """Colour-flow velocity map [nx, nz] (m/s) of an ensemble frames [N, nx, nz] complex64: doppler_autocorr, then doppler_maps.
    nyquist_velocity: nyquist_velocity(sound_speed, prf, demod_freq).  Negative: away from the probe.  Host in, host out; a
    DeviceBuffer in gives a DeviceBuffer out, queued."""
    _checked_smoothing(smoothing, kernel)
    return doppler_maps(doppler_autocorr(frames, wall_filter, degree), nyquist_velocity, smoothing, kernel)[0]


def get_power_doppler_map(frames, wall_filter="none", degree=1, smoothing="hamming", kernel=(1, 1), dynamic_range=None):
    """Power-Doppler map [nx, nz] of an ensemble: the amplitude sqrt(R0) of the wall-filtered, smoothed lag-zero autocorrelation; with
    dynamic_range (dB) the display log_compress makes of it -- 20 log10 of an amplitude is 10 log10 of a power -- in [0, 1].  It does
    not depend on a velocity scale, so it takes none.  Host in, host out; a DeviceBuffer in gives a DeviceBuffer out, queued."""
    _checked_smoothing(smoothing, kernel)
    amp = doppler_maps(doppler_autocorr(frames, wall_filter, degree), 1.0, smoothing, kernel)[1]
    return amp if dynamic_range is None else log_compress(amp, dynamic_range)


def _acquisition_key(integ, scene):
    """everything of an integrator that an acquisition and its pulse read"""
    return (bytes(integ.us_params(scene, integ.quirks)), int(integ.seed), int(integ.paths_per_ray), integ.pulse_model,
            float(integ.pulse_sigma), float(integ.fs))


def _doppler_render_request(scenes, prf, x_range, z_range, step, seed, paths_per_ray, decimation, beamformer, wall_filter, degree,
                            smoothing, kernel, dynamic_range):
    """the checks of doppler_render, all of them before any device work -> (scenes, the us_render request of the first scene's
    integrator with the I/Q chain on, the wall filter's degree, nyquist velocity)"""
    scenes = list(scenes)
    if len(scenes) < 2:
        raise ValueError(f"doppler_render needs an ensemble of two scenes at least (one per pulse), got {len(scenes)}")
    N = _checked_ensemble_length(len(scenes))
    integs = [s.integrator() for s in scenes]
    if any(getattr(i, "pulse_model", None) != "gaussian" for i in integs):
        raise ValueError("doppler_render needs pulse_model='gaussian': the 'impulse' model deposits sin(2 pi f t) at the absolute "
                         "arrival time t, so its carrier is tied to absolute time and a moving target shifts no phase from pulse to pulse")
    key = _acquisition_key(integs[0], scenes[0])
    for n in range(1, N):
        if _acquisition_key(integs[n], scenes[n]) != key:
            raise ValueError(f"doppler_render: the integrator of scene {n} differs from that of scene 0 in something an acquisition reads "
                             "(array, angles, sampling, frequency, sensor, quirks, seed, paths_per_ray or pulse): only the geometry may move")
    if not (math.isfinite(float(prf)) and float(prf) > 0.0):
        raise ValueError(f"doppler_render: prf must be finite and > 0, got {prf!r}")
    d = _wall_degree(wall_filter, degree, N)
    _checked_smoothing(smoothing, kernel)
    integ = integs[0]
    step = step or integ.sound_speed / integ.frequency / 2
    rq = _us_render_request(integ, x_range, z_range, dynamic_range, step, seed, paths_per_ray, beamformer, True, decimation, "grid", None)
    return scenes, rq, d, nyquist_velocity(integ.sound_speed, prf, rq.f_demod)


def doppler_render(scenes, prf, x_range=(-0.04, 0.04), z_range=(0.001, 0.05), step=None, seed=None, paths_per_ray=None, decimation=1,
                   beamformer=None, wall_filter="none", degree=1, smoothing="hamming", kernel=(1, 1), dynamic_range=60.0,
                   on_device=False, buffers=None):
    """Colour and power Doppler of a moving scene, beside us_render (DESIGN D24).  scenes: N scenes, 2 <= N <= 64, one per pulse at the
    pulse repetition frequency prf -- a sequence, because geometry cannot be updated in place (only materials can: Scene.device()).
    Per scene: acquisition -> pulse -> rf2iq (decimated by `decimation`) -> I/Q beamform (`beamformer`: a DelayAndSum or Capon, as
    us_render(iq=True) takes it) into frame n of the ensemble, every pulse with the SAME seed (common random numbers: between two
    pulses only the echoes of what moved change) and one first-arrival table; then doppler_autocorr(wall_filter, degree),
    doppler_maps(smoothing, kernel) with nyquist_velocity(c, prf, f) and the log compression of the amplitude.  Everything is queued
    on the context's stream; one copy per returned image.  The default step is lambda / 2.
    -> (velocity [nz, nx] in m/s, negative away from the probe; power display [nz, nx] in [0, 1]; (x, z)).  on_device: the two images
    come back as DeviceBuffers [nx, nz], still being written.  buffers: a dict that receives "frames" (the ensemble [N, nx, nz]
    complex64), "acf" and "amplitude" as DeviceBuffers.
    ValueError, before any device work: fewer than 2 scenes; integrators that differ in anything an acquisition reads; and
    pulse_model='impulse' -- its carrier is tied to absolute time, so a moving target shifts no phase.  Replaying the chain from a
    recording, as us_render does, is not built."""
    scenes, rq, d, nyq = _doppler_render_request(scenes, prf, x_range, z_range, step, seed, paths_per_ray, decimation, beamformer,
                                                 wall_filter, degree, smoothing, kernel, dynamic_range)
    integ, N = rq.integ, len(scenes)
    cx = scenes[0].device().ctx
    key = (rq.plan_key(cx), N)
    plan = getattr(integ, "_doppler_plan", None)
    if plan is None or plan.key != key:
        plan = integ._doppler_plan = _RenderPlan(cx, rq, key)
        nx, nz = rq.scan.shape
        plan.d_frames = _capi.DeviceBuffer(cx, (N, nx, nz), np.complex64)
        plan.d_acf = _capi.DeviceBuffer(cx, (3, nx, nz))
        plan.d_vel, plan.d_amp = _capi.DeviceBuffer(cx, (nx, nz)), _capi.DeviceBuffer(cx, (nx, nz))
    plan.bind(rq)
    nx, nz = rq.scan.shape
    sd = int(integ.seed if rq.seed is None else rq.seed)
    for n, scene in enumerate(scenes):
        it = scene.integrator()
        it._acquire(scene, it.quirks, paths_per_ray=rq.paths_per_ray, seed=sd, out_dev=plan.d_channel.ptr, pulse=False, queue=True)
        plan.refresh_delays(np.asarray(it.transmission_delays_buf, dtype=np.float32).reshape(rq.A, rq.E), integ.sound_speed)
        data = apply_pulse(plan.d_channel, integ.fs, integ.frequency, integ.pulse_sigma, out=plan.d_rf)
        rq.bf.automatic_setup(rq.info(plan.d_tx), rq.probe)
        data = rf2iq(data, rq.f_demod, integ.fs, decimation=rq.D, taps=plan.d_iq_taps, out=plan.d_iq)
        rq.bf.beamform(data, rq.scan, out=plan.d_frames.view(n * nx * nz, (nx, nz)), table=plan.d_table)
    doppler_autocorr(plan.d_frames, wall_filter, degree, out=plan.d_acf)
    doppler_maps(plan.d_acf, nyq, smoothing, kernel, out=(plan.d_vel, plan.d_amp))
    log_compress(plan.d_amp, rq.dynamic_range, out=plan.d_img)
    if buffers is not None:
        buffers.update(frames=plan.d_frames, acf=plan.d_acf, amplitude=plan.d_amp)
    if on_device:
        return plan.d_vel, plan.d_img, (rq.x_scan, rq.z_scan)
    return plan.d_vel.numpy().T, plan.d_img.numpy().T, (rq.x_scan, rq.z_scan)
