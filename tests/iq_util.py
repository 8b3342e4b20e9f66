"""I/Q beamforming (include/pbrt_hip.h) restated in NumPy for test_iq_restatement.py (CPU) and test_gpu_iq.py (GPU):
demodulation, complex delay-and-sum and the modulus envelope, written from the header's formulas and sharing no text with the kernels.

  rf2iq        mix with the carrier, low-pass, decimate            -> (iq [n, Td], B [n, Td]),   B = 2 sum_k |h[k]| |x[m D - k]|
  iq_beamform  complex delay-and-sum with the split re-modulation  -> (image [nx, nz], B [nx, nz]), B = sum_a sum_e |s_{a,e}|
  modulus      the envelope of an I/Q image
  response     frequency response of a set of taps

Both run in float64, or with dtype=np.float32 modelling the stated precisions: phases as float32 fractions of a cycle (the fraction itself
is taken in float64 in either case), positions split into whole samples plus a float32 fraction (nlbf_util.delayed), float32 products and
sums.  The float32 runs set the floor the device is compared on; positions, apertures and left-out pixels are nlbf_util's."""
import numpy as np

import das_util as du
import nlbf_util as nu


def _f32(v):
    """an operand as the library reads it: float32, carried on in float64"""
    return float(np.float32(v))


def _unit(cycles, dtype):
    """exp(2 pi i frac(cycles)) as (cos, sin) in `dtype`; the fraction is taken in float64, then (float32) rounded to float32 before the
    cosine and sine, which are themselves rounded to float32"""
    ph = cycles - np.floor(cycles)
    if dtype is np.float32:
        ph = ph.astype(np.float32).astype(np.float64)
    ang = 2.0 * np.pi * ph
    return np.cos(ang).astype(dtype), np.sin(ang).astype(dtype)


def _complex(re, im):
    """re + i im as complex128, component by component: the product 1j * im of complex arithmetic turns an infinite im into a NaN real
    part (0 * inf), which no kernel computes"""
    out = np.empty(np.shape(re), np.complex128)
    out.real, out.imag = re, im
    return out


def rf2iq(x, fs, t0, f_d, D, taps, dtype=np.float64):
    """x [n, T] real, sample j at t0 + j / fs -> (iq [n, Td] complex, B [n, Td]), Td = ceil(T / D):
         u_j = x_j cos(2 pi f_d t_j), v_j = -x_j sin(2 pi f_d t_j),  iq[m] = 2 sum_{k = -K .. K} h[k] (u + i v)[m D - k], zero outside"""
    x = du.f64(np.atleast_2d(x))
    h = du.f64(taps).ravel()
    n, T = x.shape
    K, D = len(h) // 2, int(D)
    Td = -(-T // D)
    t = _f32(t0) + np.arange(T, dtype=np.float64) / _f32(fs)
    cs, sn = _unit(_f32(f_d) * t, dtype)
    xd = x.astype(dtype)
    u, v = xd * cs[None], -(xd * sn[None])
    m = np.arange(Td) * D
    B = 2.0 * np.stack([np.convolve(np.abs(row), np.abs(h), "full")[K + m] for row in x])
    if dtype is np.float64:
        re = np.stack([np.convolve(row, h, "full")[K + m] for row in u])
        im = np.stack([np.convolve(row, h, "full")[K + m] for row in v])
        return _complex(2.0 * re, 2.0 * im), B
    # float32: products and sums in order of increasing k
    pad = np.zeros((n, K), dtype)
    up, vp = np.concatenate([pad, u, pad, np.zeros((n, D), dtype)], axis=1), np.concatenate([pad, v, pad, np.zeros((n, D), dtype)], axis=1)
    hd = h.astype(dtype)
    re, im = np.zeros((n, Td), dtype), np.zeros((n, Td), dtype)
    for j in range(2 * K + 1):            # k = j - K; sample m D - k sits at padded index m D - k + K = m D + 2 K - j
        idx = m + 2 * K - j
        re = re + hd[j] * up[:, idx]
        im = im + hd[j] * vp[:, idx]
    return _complex(dtype(2) * re, dtype(2) * im), B


def iq_beamform(iq, tx, elem, x, z, fs, c, f_d, t0=0.0, f_number=1.0, interpolation="linear", compound="sum", dtype=np.float64):
    """iq [A, E, T] complex at the rate fs -> (image [nx, nz] complex, B [nx, nz]).  Per transmission a, over the elements U(a) of the pixel:
         q_a = sum_e exp(2 pi i frac(f_d d_e / c)) s_{a,e},   image = sum_a exp(2 pi i frac(f_d t_tx(a))) q_a  (/ A for 'mean'),
       s_{a,e} the delayed complex sample (nlbf_util.delayed on both components: delay-and-sum's own), B = sum_a sum_e |s_{a,e}| (likewise)"""
    iq = np.asarray(iq, np.complex64)
    A = iq.shape[0]
    fs64, fd64, t064 = _f32(fs), _f32(f_d), _f32(t0)
    kw = dict(t0=t0, f_number=f_number, interpolation=interpolation, dtype=dtype)
    re_it = nu.delayed(iq.real, tx, elem, x, z, fs, c, **kw)
    im_it = nu.delayed(iq.imag, tx, elem, x, z, fs, c, **kw)
    pos_it = nu._positions(tx, elem, x, z, fs, c, t0, f_number)
    img_re = img_im = B = None
    for (sr, ok), (si, _), (_, _, s_tx, s_rx) in zip(re_it, im_it, pos_it):
        sr, si = np.where(ok, sr, dtype(0)), np.where(ok, si, dtype(0))
        ce, se = _unit(fd64 * (s_rx / fs64), dtype)                    # receive: d_e / c
        ca, sa = _unit(fd64 * (s_tx / fs64 + t064), dtype)             # transmit: t_tx(a)
        qr = (ce * sr - se * si).sum(axis=0, dtype=dtype)
        qi = (ce * si + se * sr).sum(axis=0, dtype=dtype)
        yr, yi = ca * qr - sa * qi, ca * qi + sa * qr
        b = np.hypot(sr.astype(np.float64), si.astype(np.float64)).sum(axis=0)
        img_re = yr if img_re is None else img_re + yr
        img_im = yi if img_im is None else img_im + yi
        B = b if B is None else B + b
    if compound == "mean":
        img_re, img_im, B = img_re / dtype(A), img_im / dtype(A), B / A
    return _complex(img_re, img_im), B


def modulus(iq):
    iq = np.asarray(iq)
    return np.sqrt(iq.real.astype(np.float64) ** 2 + iq.imag.astype(np.float64) ** 2)


def response(taps, f, fs):
    """H(f) = sum_k h[k] exp(-2 pi i f k / fs) of taps [2 K + 1], in float64"""
    h = np.asarray(taps, np.float64).ravel()
    k = np.arange(len(h)) - len(h) // 2
    return np.sum(h * np.exp(-2j * np.pi * f * k / fs))


def rf2iq_bad_mask(T, K, D, j):
    """the outputs m in [0, ceil(T / D)) of a trace that a bad sample at index j reaches: |m D - j| <= K"""
    return np.abs(np.arange(-(-T // D)) * D - j) <= K
