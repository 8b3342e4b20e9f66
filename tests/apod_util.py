"""Receive apodisation (include/pbrt_hip.h) restated in NumPy for test_apod_restatement.py (CPU) and test_gpu_apod.py
(GPU): the windows on the f-number aperture and the four beamformers on weighted samples, written from the header's formulas and
sharing no text with the kernel.

  window     w(u) of a window name: 1 at the aperture's centre u = 0, the window's edge value at u = 1
  weights    w_e of every (element, pixel), and which elements lie inside the pixel's aperture
  beamform   'das' | 'pdas' | 'fdmas' | 'iq' of the WEIGHTED delayed samples -> (image, B); B is the per-pixel sum over transmissions
             and used elements of the UNWEIGHTED magnitudes (nlbf_util.beamform's B, iq_util.iq_beamform's B): the weights are <= 1,
             so B bounds what the pixel adds up, and a weight's error scales with |s|, not with |w s|, which vanishes at a Hann edge
  side_lobe_db  the first side lobe of a lateral profile, relative to its peak

In float64, or with dtype=np.float32 following the arithmetic of the header: u and t in float64, t rounded once to float32, the cosine
rounded to float32, one fused multiply-add and the product with the sample in float32; the delayed samples, roots, sums and rotations
in float32 as nlbf_util and iq_util model them."""
import numpy as np

import das_util as du
import iq_util as iu
import nlbf_util as nu
from oracle import beamform as obf

A0 = {"tukey": 0.5, "hann": 0.5, "hamming": float(np.float32(0.54))}
WINDOWS = ("boxcar", "tukey", "hann", "hamming")
WEIGHT_BOUND = 4.0 * 2.0 ** -24      # a float32 weight against its float64 value (include/pbrt_hip.h)


def window(u, name, alpha=0.5, dtype=np.float64):
    """w(u) for u in [0, 1] (float64 in): t = clip((u - (1 - alpha)) / alpha, 0, 1), w = a0 + (1 - a0) cos(pi t); alpha is read by
    'tukey' only ('hann' and 'hamming' span the whole aperture), and is the float32 the library is given"""
    u = np.asarray(u, np.float64)
    if name == "boxcar":
        return np.ones(u.shape, dtype)
    if name not in A0:
        raise ValueError(name)
    al = float(np.float32(alpha)) if name == "tukey" else 1.0
    t = np.clip((u - (1.0 - al)) / al, 0.0, 1.0)
    a0 = A0[name]
    if dtype is np.float64:
        return a0 + (1.0 - a0) * np.cos(np.pi * t)
    t = t.astype(np.float32).astype(np.float64)                  # rounded once
    cs = np.cos(np.pi * t).astype(np.float32).astype(np.float64)  # the float32 cosine
    a1 = float(np.float32(1.0) - np.float32(a0))                 # 1 - a0 in float32
    return (a0 + a1 * cs).astype(np.float32)                     # one rounding: the product of two float32 is exact in float64


def distances(elem, x, z, f_number):
    """-> (u [E, nx, nz] float64, inside [E, nx, nz]): the distance of element e from the centre of the pixel's aperture over the
    aperture's half width -- |x - x_e| / (z / (2 f#)) for a line of elements [E], 2 f# |d_t| / d_n in the element's own frame for an
    element table [E, 4] -- and whether the element lies inside the aperture (u <= 1; the table also asks d_n > 0)"""
    fn = float(np.float32(f_number))
    if not fn > 0.0:
        raise ValueError("a window needs an f-number aperture")
    gx, gz = du.f64(x).ravel(), du.f64(z).ravel()
    X, Z = np.meshgrid(gx, gz, indexing="ij")
    if nu._table(elem):
        el = du.f64(elem).reshape(-1, 4)
        dx, dz = X[None] - el[:, 0, None, None], Z[None] - el[:, 1, None, None]
        dn = dx * el[:, 2, None, None] + dz * el[:, 3, None, None]
        dt = dx * el[:, 3, None, None] - dz * el[:, 2, None, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            u = 2.0 * fn * np.abs(dt) / dn
        inside = (dn > 0) & (2.0 * fn * np.abs(dt) <= dn)
    else:
        ex = du.f64(elem).ravel()
        dx = np.abs(X[None] - ex[:, None, None])
        half = Z[None] / (2.0 * fn)
        with np.errstate(divide="ignore", invalid="ignore"):
            u = dx / half
        inside = dx <= half
    return np.where(inside, u, 1.0), inside


def weights(elem, x, z, f_number, name, alpha=0.5, dtype=np.float64):
    """-> (w [E, nx, nz] in `dtype`, inside [E, nx, nz]); outside the aperture the weight is the window's edge value and is not used"""
    u, inside = distances(elem, x, z, f_number)
    return window(u, name, alpha, dtype), inside


def beamform(method, data, tx, elem, x, z, fs, c, name, alpha=0.5, p=2.0, f_d=None, t0=0.0, f_number=1.0, interpolation="linear",
             compound="sum", dtype=np.float64):
    """method 'das' | 'pdas' | 'fdmas' (data real) | 'iq' (data complex, demodulated at f_d) with the window `name` -> (image, B).
    Every delayed sample s_{a,e} of nlbf_util.delayed becomes w_e s_{a,e} before the method's arithmetic (nlbf_util.beamform's,
    iq_util.iq_beamform's); B is of the unweighted samples."""
    w, _ = weights(elem, x, z, f_number, name, alpha, dtype)
    kw = dict(t0=t0, f_number=f_number, interpolation=interpolation)
    if method == "iq":
        return _iq(data, tx, elem, x, z, fs, c, f_d, w, compound, dtype, kw)
    A = np.shape(data)[0]
    _, B = nu.beamform(method, data, tx, elem, x, z, fs, c, p=p, compound=compound, dtype=np.float64, **kw)
    img = None
    for val, ok in nu.delayed(data, tx, elem, x, z, fs, c, dtype=dtype, **kw):
        val = np.where(ok, (w * val).astype(dtype), dtype(0))
        if method == "das":
            y = val.sum(axis=0, dtype=dtype)
        else:
            pp = 2 if method == "fdmas" else p
            q = nu.signed_root(val, pp, dtype).sum(axis=0, dtype=dtype)
            y = dtype(0.5) * (q * q - np.abs(val).sum(axis=0, dtype=dtype)) if method == "fdmas" else nu.signed_power(q, pp, dtype)
        img = y if img is None else img + y
    return (img / dtype(A) if compound == "mean" else img), B


def _iq(iq, tx, elem, x, z, fs, c, f_d, w, compound, dtype, kw):
    iq = np.asarray(iq, np.complex64)
    A = iq.shape[0]
    fs64, fd64, t064 = iu._f32(fs), iu._f32(f_d), iu._f32(kw["t0"])
    re_it = nu.delayed(iq.real, tx, elem, x, z, fs, c, dtype=dtype, **kw)
    im_it = nu.delayed(iq.imag, tx, elem, x, z, fs, c, dtype=dtype, **kw)
    pos_it = nu._positions(tx, elem, x, z, fs, c, kw["t0"], kw["f_number"])
    img_re = img_im = B = None
    for (sr, ok), (si, _), (_, _, s_tx, s_rx) in zip(re_it, im_it, pos_it):
        b = np.where(ok, np.hypot(sr.astype(np.float64), si.astype(np.float64)), 0.0).sum(axis=0)    # unweighted
        sr, si = np.where(ok, (w * sr).astype(dtype), dtype(0)), np.where(ok, (w * si).astype(dtype), dtype(0))
        ce, se = iu._unit(fd64 * (s_rx / fs64), dtype)
        ca, sa = iu._unit(fd64 * (s_tx / fs64 + t064), dtype)
        qr = (ce * sr - se * si).sum(axis=0, dtype=dtype)
        qi = (ce * si + se * sr).sum(axis=0, dtype=dtype)
        yr, yi = ca * qr - sa * qi, ca * qi + sa * qr
        img_re = yr if img_re is None else img_re + yr
        img_im = yi if img_im is None else img_im + yi
        B = b if B is None else B + b
    if compound == "mean":
        img_re, img_im, B = img_re / dtype(A), img_im / dtype(A), B / A
    return iu._complex(img_re, img_im), B


def side_lobe_db(rf, iz):
    """the first side lobe of the envelope's lateral profile at depth index iz, in dB relative to the peak: the largest value beyond
    the first local minimum on either side of the peak"""
    prof = obf.envelope(rf)[:, iz]
    k = int(np.argmax(prof))
    best = 0.0
    for step in (-1, +1):
        i = k
        while 0 <= i + step < len(prof) and prof[i + step] < prof[i]:
            i += step
        tail = prof[i::step] if step > 0 else prof[i::-1]
        if 0 <= i + step < len(prof):         # a minimum inside the scan: what lies beyond it
            best = max(best, float(tail.max()))
    return 20.0 * np.log10(best / prof[k]) if best > 0 else -np.inf
