"""Spatial-coherence beamforming on I/Q data -- SLSC and the coherence factor (include/pbrt_hip.h "spatial coherence") --
restated in NumPy for test_coherence_restatement.py (CPU) and test_gpu_coherence.py (GPU): written from the header's formulas and
sharing no text with the kernel.

  lags          M = min(max(1, floor(lag_prop N)), N - 1, 64), the product in float32; 0 for N < 2
  rows          per transmission the kernel samples v_k[h] of the elements a pixel uses, at their ranks
  coherence     the image -> (image [nx, nz], B [nx, nz], edge [nx, nz]);  SLSC: B = sum_a M_a, CF: B = sum_a sum_k |v_k|
  restated      coherence on a walk case with capon_util.case_data, cached;  floor_of: the float32 floor of a case

The positions and the elements a pixel uses are nlbf_util's (_positions, _split), the rotations iq_util's (_unit), the inputs
capon_util's (case_data).  Everything runs in float64, or with dtype=np.float32 in one of two orders of every sum (order 0: ascending,
1: descending): the float32 runs set the floor the device is compared on.  The header is followed as written: the rows are normalised,
then the products are taken.  (The power of two that the header puts on a row or on an aperture is exact and is left out.)
`edge`: pixels with a pair whose kernel reaches an end of the trace while its position lies within das_util.EDGE_SAMPLES of a whole
(linear) or half (nearest) sample -- there another order of operations may take a sample where this one takes (0, 0)."""
import functools

import numpy as np

import capon_util as ku
import das_util as du
import iq_util as iu
import nlbf_util as nu
from walk_cases import C0, T, geometry

MAX_E, MAX_H, MAX_LAG = 256, 4, 64


def lags(N, lag_prop):
    N = int(N)
    if N < 2:
        return 0
    return min(max(1, int(np.floor(np.float32(lag_prop) * np.float32(N)))), N - 1, MAX_LAG)


def _ordered_sum(a, axis, dtype, order):
    """the sum along `axis` one term after the other in `dtype`, ascending (order 0) or descending (1); in float64, where the order
    moves the 16th digit, numpy's own"""
    a = np.moveaxis(np.asarray(a, dtype), axis, -1)
    if a.shape[-1] == 0:
        return np.zeros(a.shape[:-1], dtype)
    if dtype is np.float64:
        return a.sum(axis=-1)
    if order:
        a = a[..., ::-1]
    return np.cumsum(a, axis=-1, dtype=dtype)[..., -1]


def rows(iq, tx, elem, x, z, fs, c, f_d, H, t0=0.0, f_number=1.0, interpolation="linear", dtype=np.float64):
    """for every transmission a: (re, im [pixels, E, 2 H + 1] the v_k[h] at rank k, zero beyond N; N [pixels]; (ca, sa) [pixels] rot_a;
    edge [pixels]; (before, past) the kept pairs with a kernel sample before sample 0 / past the last one)"""
    iq = np.asarray(iq, np.complex64)
    A, E, nT = iq.shape
    fs64, fd64, t064 = iu._f32(fs), iu._f32(f_d), iu._f32(t0)
    ee = np.arange(E)[:, None, None]
    hh = np.arange(-H, H + 1)
    for a, (s, use, s_tx, s_rx) in enumerate(nu._positions(tx, elem, x, z, fs, c, t0, f_number)):
        dre, dim = iq[a].real.astype(dtype), iq[a].imag.astype(dtype)
        if interpolation == "nearest":
            ctr = np.rint(s)
            ok = (ctr >= 0) & (ctr <= nT - 1) & use
            near = np.abs(s - np.floor(s) - 0.5) < du.EDGE_SAMPLES
            w = None
        else:
            ctr = np.floor(s)
            ok = (((ctr >= 0) & (ctr < nT - 1)) | (s == nT - 1)) & use
            near = np.abs(s - np.rint(s)) < du.EDGE_SAMPLES
            if dtype is np.float32:
                (ti, tf), (ri, rf) = nu._split(s_tx), nu._split(s_rx)
                fr = tf[None] + rf
                carry = np.floor(fr)
                ctr, w = ti[None] + ri + carry, fr - carry
            else:
                w = (s - ctr).astype(np.float32).astype(dtype)
        ctr = np.where(ok, ctr, 0.0)
        lo, hi = np.rint(s) - H - 1, np.rint(s) + H + 1
        edge = (ok & near & ((lo < 0) | (hi > nT - 1))).any(axis=0)
        before, past = int((ok & (ctr - H < 0)).sum()), int((ok & (ctr + H > nT - 1)).sum())
        ce, se = iu._unit(fd64 * (s_rx / fs64), dtype)
        ca, sa = iu._unit(fd64 * (s_tx / fs64 + t064), dtype)
        vre = np.zeros(s.shape + (2 * H + 1,), dtype)
        vim = np.zeros_like(vre)
        for k, h in enumerate(hh):
            j = ctr + h
            if interpolation == "nearest":
                inside = (j >= 0) & (j <= nT - 1)
                jj = np.clip(j, 0, nT - 1).astype(int)
                sr, si = dre[ee, jj], dim[ee, jj]
            else:
                between, last = (j >= 0) & (j < nT - 1), (j == nT - 1) & (w == 0)
                inside = between | last
                j0 = np.clip(j, 0, nT - 1).astype(int)
                j1 = np.clip(j0 + 1, 0, nT - 1)
                with np.errstate(invalid="ignore"):
                    sr = np.where(last, dre[ee, j0], dre[ee, j0] + w * (dre[ee, j1] - dre[ee, j0]))
                    si = np.where(last, dim[ee, j0], dim[ee, j0] + w * (dim[ee, j1] - dim[ee, j0]))
            sr, si = np.where(inside & ok, sr, dtype(0)).astype(dtype), np.where(inside & ok, si, dtype(0)).astype(dtype)
            with np.errstate(invalid="ignore"):
                vre[..., k], vim[..., k] = (ce * sr - se * si).astype(dtype), (ce * si + se * sr).astype(dtype)
        # the elements in use, in index order, at the front of every row (a stable sort of the flags)
        okp = ok.reshape(E, -1).T
        front = np.argsort(~okp, axis=1, kind="stable")
        n = okp.sum(axis=1)
        live = (np.arange(E)[None, :] < n[:, None])[:, :, None]

        def packed(v):
            v = np.moveaxis(v.reshape(E, -1, 2 * H + 1), 0, 1)               # [pixels, E, K]
            return np.where(live, np.take_along_axis(v, front[:, :, None], axis=1), dtype(0))

        yield packed(vre), packed(vim), n, (ca.ravel(), sa.ravel()), edge.ravel(), (before, past)


def _slsc(vre, vim, N, lag_prop, dtype, order):
    """one transmission: v [P, E, K] at the ranks, N [P] -> (y [P], M [P])"""
    P_, E, _ = vre.shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pw = _ordered_sum(vre * vre + vim * vim, 2, dtype, order)             # P_k [P, E]
        nrm = np.sqrt(pw)[:, :, None]
        zero = (pw == 0)[:, :, None]
        ure, uim = np.where(zero, dtype(0), vre / nrm).astype(dtype), np.where(zero, dtype(0), vim / nrm).astype(dtype)
        M = np.array([lags(n, lag_prop) for n in range(E + 1)])[N]
        R = []
        for m in range(1, int(M.max()) + 1 if len(M) else 1):
            C = _ordered_sum(ure[:, :E - m] * ure[:, m:] + uim[:, :E - m] * uim[:, m:], 2, dtype, order)      # C(i, i + m) [P, E - m]
            pair = np.arange(E - m)[None, :] + m < N[:, None]
            tot = _ordered_sum(np.where(pair, C, dtype(0)), 1, dtype, order)
            R.append(np.where(m <= M, tot / np.maximum(N - m, 1).astype(dtype), dtype(0)).astype(dtype))
        y = np.zeros(P_, dtype)
        for r in (R if order == 0 else R[::-1]):
            y = y + r
    return y, M


def _cf(vre, vim, N, gamma, dtype, order):
    """one transmission: v [P, E, 1] -> (S_re w, S_im w [P], sum_k |v_k| [P])"""
    vre, vim = vre[:, :, 0], vim[:, :, 0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        sre, sim = _ordered_sum(vre, 1, dtype, order), _ordered_sum(vim, 1, dtype, order)
        q = _ordered_sum(vre * vre + vim * vim, 1, dtype, order)
        cf = np.where(q == 0, dtype(0), (sre * sre + sim * sim) / (np.maximum(N, 1).astype(dtype) * q)).astype(dtype)
        wgt = np.ones_like(cf) if gamma == 0 else cf if gamma == 1 else np.power(cf, dtype(gamma))
        mag = np.sqrt(vre.astype(np.float64) ** 2 + vim.astype(np.float64) ** 2).sum(axis=1)
        return (wgt * sre).astype(dtype), (wgt * sim).astype(dtype), mag


def coherence(iq, tx, elem, x, z, fs, c, f_d, kind="slsc", lag_prop=0.3, half_kernel=1, gamma=1.0, t0=0.0, f_number=1.0,
              interpolation="linear", compound="sum", dtype=np.float64, order=0):
    """iq [A, E, T] complex at the rate fs -> (image [nx, nz], B [nx, nz], edge [nx, nz] bool, (before, past)).  The header's
    definition: SLSC float64 image clamped at 0 (NaN kept), CF complex128."""
    A = np.shape(iq)[0]
    nx, nz = len(np.ravel(x)), len(np.ravel(z))
    H = int(half_kernel) if kind == "slsc" else 0
    acc_re, acc_im, B = np.zeros(nx * nz, dtype), np.zeros(nx * nz, dtype), np.zeros(nx * nz)
    edge, before, past = np.zeros(nx * nz, bool), 0, 0
    for vre, vim, N, (ca, sa), e, (b_, p_) in rows(iq, tx, elem, x, z, fs, c, f_d, H, t0, f_number, interpolation, dtype):
        edge |= e
        before, past = before + b_, past + p_
        if kind == "slsc":
            y, M = _slsc(vre, vim, N, lag_prop, dtype, order)
            acc_re = acc_re + y
            B += M
        else:
            wre, wim, mag = _cf(vre, vim, N, gamma, dtype, order)
            with np.errstate(invalid="ignore"):
                yre, yim = (ca * wre - sa * wim).astype(dtype), (ca * wim + sa * wre).astype(dtype)
            acc_re = acc_re + np.where(N > 0, yre, dtype(0))                  # (a transmission with N = 0 is skipped)
            acc_im = acc_im + np.where(N > 0, yim, dtype(0))
            B += mag
    if compound == "mean":
        acc_re, acc_im, B = acc_re / dtype(A), acc_im / dtype(A), B / A
    if kind == "slsc":
        img = np.where((acc_re > 0) | np.isnan(acc_re), acc_re, 0.0).astype(np.float64)
    else:
        img = iu._complex(acc_re.astype(np.float64), acc_im.astype(np.float64))
    return img.reshape(nx, nz), B.reshape(nx, nz), edge.reshape(nx, nz), (before, past)


# ---- on the walk cases -----------------------------------------------------------------------------------------------------------------
def settings_kw(setting):
    """('slsc', lag_prop, H) or ('cf', gamma) -> the keywords of coherence / coherence_beamform"""
    return dict(kind="slsc", lag_prop=setting[1], half_kernel=setting[2]) if setting[0] == "slsc" else dict(kind="cf", gamma=setting[1])


@functools.lru_cache(maxsize=None)
def restated(name, which, f_d, setting, f32=False, order=0):
    g = geometry(name)
    out = coherence(ku.case_data(name, which), g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, f_d,
                    dtype=np.float32 if f32 else np.float64, order=order, **settings_kw(setting), **g["kw"])
    for a in out[:3]:
        a.setflags(write=False)
    return out


def floor_of(name, which, f_d, setting, used):
    """the float32 floor of a case: the larger of the two orders' largest |f32 - f64| / B over the pixels `used`"""
    ref, B = restated(name, which, f_d, setting)[:2]
    return max(float((np.abs(restated(name, which, f_d, setting, True, o)[0] - ref)[used] / B[used]).max()) for o in (0, 1))


def near_bad(g, sites, H, t0=0.0):
    """[nx, nz]: pixels with a pair whose position lies within das_util.EDGE_SAMPLES of a whole (linear) or half (nearest) sample and
    whose kernel, moved by one sample either way, reaches a bad sample (sites: [(a, e, t)]): nlbf_util.near_bad with the kernel's reach"""
    kw = g["kw"]
    out = np.zeros(g["left_out"].shape, bool)
    for a, (_, _, _, wlo, whi) in enumerate(nu.sample_reads(g["tx"], g["elem"], g["x"], g["z"], T, g["fs"], C0, t0=t0,
                                                            f_number=kw["f_number"], interpolation=kw["interpolation"])):
        for sa, e, t in sites:
            if sa == a:
                out |= (wlo[e] <= whi[e]) & (wlo[e] - H <= t) & (t <= whi[e] + H)
    return out
