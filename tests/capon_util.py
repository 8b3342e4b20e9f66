"""Capon (minimum-variance) beamforming on I/Q data (include/pbrt_hip.h "Capon") restated in NumPy for
test_capon_restatement.py (CPU) and test_gpu_capon.py (GPU): written from the header's formulas and sharing no text with the kernel.

  lm            the subarray length L and the number of subarrays M of an aperture of N elements
  chol_ones     u with R u = 1 for a batch of Hermitian positive-definite matrices, by a hand-written Cholesky
  capon         the image -> (image [nx, nz] complex, B [nx, nz]),  B = sum_a sum_k |v_k|
  case_data     the two input families of the GPU test on a walk case;  restated: capon on a walk case, cached

The delayed samples, the elements a pixel uses and the positions are nlbf_util's (delayed, _positions), the rotations iq_util's (_unit).
Everything runs in float64, or with dtype=np.float32 in one of two orders of every sum (order 0: ascending, 1: descending): the float32
runs set the floor the device is compared on.  The pixels of all transmissions are taken together in groups of one L, so that no loop
runs over pixels."""
import functools

import numpy as np

import iq_util as iu
import nlbf_util as nu
from walk_cases import C0, T, geometry

MAX_L, MAX_E = 32, 256


def lm(N, l_prop):
    """(L, M): L = min(max(1, floor(l_prop N)), 32) with the product in float32, M = N - L + 1 (0 for N = 0)"""
    L = min(max(1, int(np.floor(np.float32(l_prop) * np.float32(N)))), MAX_L)
    return L, (N - L + 1 if N else 0)


def _seq(n, order):
    return range(n) if order == 0 else range(n - 1, -1, -1)


def chol_ones(R, dtype=np.float64, order=0):
    """R [P, L, L] Hermitian positive definite -> u [P, L] with R u = 1: R = G G^H column by column, G y = 1, G^H u = y"""
    ct = np.complex64 if dtype is np.float32 else np.complex128
    R = np.asarray(R, ct)
    P, L, _ = R.shape
    G = np.zeros((P, L, L), ct)
    diag = np.zeros((P, L), dtype)
    for j in range(L):
        s = R[:, j, j].real.astype(dtype)
        t = R[:, j + 1:, j].copy()
        for k in _seq(j, order):
            s = s - (G[:, j, k].real ** 2 + G[:, j, k].imag ** 2).astype(dtype)
            t = t - G[:, j + 1:, k] * np.conj(G[:, j, k])[:, None]
        diag[:, j] = np.sqrt(s)
        G[:, j + 1:, j] = t / diag[:, j, None]
    y = np.zeros((P, L), ct)
    for i in range(L):
        t = np.ones(P, ct)
        for k in _seq(i, order):
            t = t - G[:, i, k] * y[:, k]
        y[:, i] = t / diag[:, i]
    u = np.zeros((P, L), ct)
    for i in range(L - 1, -1, -1):
        t = y[:, i].copy()
        for k in (range(i + 1, L) if order == 0 else range(L - 1, i, -1)):
            t = t - np.conj(G[:, k, i]) * u[:, k]
        u[:, i] = t / diag[:, i]
    return u


def _group(V, N, L, l_prop, delta_l, dtype, order):
    """the pixels of one subarray length L: V [P, Nmax] (zero beyond N), N [P] -> y [P]"""
    ct = np.complex64 if dtype is np.float32 else np.complex128
    P = len(N)
    M = N - L + 1
    R = np.zeros((P, L, L), ct)
    xbar = np.zeros((P, L), ct)
    for l in _seq(int(M.max()), order):
        on = (l < M)[:, None]
        x = np.where(on, V[:, l:l + L], ct(0))                 # x_l, and nothing from the pixels that have fewer subarrays
        R = R + x[:, :, None] * np.conj(x)[:, None, :]
        xbar = xbar + x
    tr = np.zeros(P, dtype)
    for i in _seq(L, order):
        tr = tr + R[:, i, i].real
    live = ~(tr == 0)
    y = np.zeros(P, ct)
    if not live.any():
        return y
    R, xbar, tr, N, M = R[live], xbar[live], tr[live], N[live], M[live]
    eps = (dtype(delta_l) * tr / dtype(L)).astype(dtype)
    idx = np.arange(L)
    R[:, idx, idx] = (R[:, idx, idx].real + eps[:, None]).astype(ct)
    u = chol_ones(R, dtype, order)
    num, den = np.zeros(len(N), ct), np.zeros(len(N), dtype)
    for i in _seq(L, order):
        num = num + np.conj(u[:, i]) * xbar[:, i]
        den = den + u[:, i].real
    y[live] = ((N.astype(dtype) / M.astype(dtype)) * num / den).astype(ct)
    return y


def capon(iq, tx, elem, x, z, fs, c, f_d, l_prop=0.5, delta_l=0.01, t0=0.0, f_number=1.0, interpolation="linear", compound="sum",
          dtype=np.float64, order=0):
    """iq [A, E, T] complex at the rate fs -> (image [nx, nz] complex128, B [nx, nz]).  Per pixel and transmission a, over the elements
    U(a) in index order: v_k = rot_e s_{a,e}; L, M = lm(N); R = sum_l x_l x_l^H, xbar = sum_l x_l over the subarrays x_l = v[l : l + L];
    tr = trace R; y_a = 0 when N = 0 or tr == 0, else R' = R + delta_l tr / L I, R' u = 1, y_a = (N / M) u^H xbar / sum_i Re u_i;
    image = sum_a rot_a y_a (/ A for 'mean'); B = sum_a sum_k |v_k| (likewise)."""
    iq = np.asarray(iq, np.complex64)
    A, E, _ = iq.shape
    ct = np.complex64 if dtype is np.float32 else np.complex128
    fs64, fd64, t064 = iu._f32(fs), iu._f32(f_d), iu._f32(t0)
    kw = dict(t0=t0, f_number=f_number, interpolation=interpolation, dtype=dtype)
    re_it = nu.delayed(iq.real, tx, elem, x, z, fs, c, **kw)
    im_it = nu.delayed(iq.imag, tx, elem, x, z, fs, c, **kw)
    pos_it = nu._positions(tx, elem, x, z, fs, c, t0, f_number)
    nx, nz = len(np.ravel(x)), len(np.ravel(z))
    V, N, rot = [], [], []
    B = np.zeros((nx, nz))
    for (sr, ok), (si, _), (_, _, s_tx, s_rx) in zip(re_it, im_it, pos_it):
        ce, se = iu._unit(fd64 * (s_rx / fs64), dtype)
        ca, sa = iu._unit(fd64 * (s_tx / fs64 + t064), dtype)
        v = np.empty(sr.shape, ct)
        v.real, v.imag = (ce * sr - se * si).astype(dtype), (ce * si + se * sr).astype(dtype)
        v, ok = v.reshape(E, -1).T, ok.reshape(E, -1).T                     # [pixels, E]
        B += np.where(ok, np.abs(v.astype(np.complex128)), 0.0).sum(axis=1).reshape(nx, nz)
        # the elements in use, in index order, at the front of every row (a stable sort of the flags)
        front = np.argsort(~ok, axis=1, kind="stable")
        n = ok.sum(axis=1)
        packed = np.where(np.arange(E)[None, :] < n[:, None], np.take_along_axis(v, front, axis=1), ct(0))
        V.append(packed)
        N.append(n)
        r = np.empty(nx * nz, ct)
        r.real, r.imag = ca.ravel(), sa.ravel()
        rot.append(r)
    V, N, rot = np.concatenate(V), np.concatenate(N), np.concatenate(rot)
    V = np.concatenate([V, np.zeros((len(V), MAX_L), ct)], axis=1)           # (a subarray window never leaves the row)
    Ls = np.array([lm(int(n), l_prop)[0] for n in range(E + 1)])[N]
    y = np.zeros(len(N), ct)
    for L in np.unique(Ls[N > 0]):
        sel = (Ls == L) & (N > 0)
        y[sel] = _group(V[sel], N[sel], int(L), l_prop, delta_l, dtype, order)
    terms = (rot * y).astype(ct).reshape(A, nx, nz)
    img = np.zeros((nx, nz), ct)
    for a in range(A):
        img = img + terms[a]
    if compound == "mean":
        img, B = img / dtype(A), B / A
    return img.astype(np.complex128), B


# ---- the inputs of the GPU test on the walk cases ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_data(name, which):
    """'noise': complex normal; 'coherent': (0.75 + 0.3j) + 0.05 noise -- with demod_freq = 0 every v_k of a pixel is nearly one value
    and the condition number of R' is near L / delta_l"""
    g = geometry(name)
    rng = np.random.default_rng(sum(map(ord, name)) * 11 + len(which))
    shape = (g["A"], g["E"], T)
    noise = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    data = noise if which == "noise" else (0.75 + 0.3j) + 0.05 * noise
    data = data.astype(np.complex64)
    data.setflags(write=False)
    return data


@functools.lru_cache(maxsize=None)
def restated(name, which, f_d, l_prop, delta_l, f32=False, order=0):
    g = geometry(name)
    img, B = capon(case_data(name, which), g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, f_d, l_prop, delta_l,
                   dtype=np.float32 if f32 else np.float64, order=order, **g["kw"])
    img.setflags(write=False)
    B.setflags(write=False)
    return img, B


def floor_of(name, which, f_d, l_prop, delta_l, used):
    """the float32 floor of a case: the larger of the two orders' largest |f32 - f64| / B over the pixels `used`"""
    ref, B = restated(name, which, f_d, l_prop, delta_l)
    return max(float((np.abs(restated(name, which, f_d, l_prop, delta_l, True, o)[0] - ref)[used] / B[used]).max()) for o in (0, 1))


def width(prof, level=0.5):
    """-6 dB width (in pixels, edges interpolated) of a profile around its maximum; inf where it never falls to the level"""
    prof = np.asarray(prof, np.float64)
    k = int(np.argmax(prof))
    thr = level * prof[k]

    def reach(step):
        i = k
        while 0 <= i + step < len(prof) and prof[i + step] >= thr:
            i += step
        j = i + step
        if not 0 <= j < len(prof):
            return float("inf")
        return abs(i - k) + (prof[i] - thr) / (prof[i] - prof[j])

    return reach(-1) + reach(+1)


@functools.lru_cache(maxsize=None)
def baseband_scatterer(A):
    """nlbf_util.point_scatterer brought to baseband analytically: per (transmission, element) the Gaussian envelope of the pulse
    times exp(-2 pi i f0 tau), tau the scatterer's own delay, noise free; the scan is the three depths around the scatterer.
    -> dict(iq, tx, ex, x, z, fs, c, f0)"""
    d = nu.point_scatterer(A=A)
    ex, tx = d["ex"].astype(np.float64), d["tx"].astype(np.float64)
    depth = float(d["z"][d["iz"]])
    dist = np.sqrt(ex ** 2 + depth ** 2)
    tau = np.min(tx + dist[None] / d["c"], axis=1)[:, None] + dist[None] / d["c"]
    t = np.arange(d["data"].shape[2])[None, None, :] / d["fs"] - tau[:, :, None]
    sigma = 1.5 / (2 * d["f0"])
    iq = (np.exp(-(t / sigma) ** 2) * np.exp(-2j * np.pi * d["f0"] * tau[:, :, None])).astype(np.complex64)
    return dict(iq=iq, tx=d["tx"], ex=d["ex"], x=d["x"], z=d["z"][d["iz"] - 1:d["iz"] + 2], fs=d["fs"], c=d["c"], f0=d["f0"])


def assert_capon_narrows_the_scatterer(beamform_das, beamform_capon):
    """the point-scatterer inequality, A = 1 and 3, f-number 0 and 1, l_prop 0.5, delta_l 0.01: the -6 dB lateral width of |Capon| is
    under a quarter of delay-and-sum's and the peak within 1 % of it.  beamform_*(s, f_number) -> complex image [nx, 3]."""
    for A in (1, 3):
        s = baseband_scatterer(A)
        for fn in (0.0, 1.0):
            das, cap = np.abs(beamform_das(s, fn))[:, 1], np.abs(beamform_capon(s, fn))[:, 1]
            w_das, w_cap, peak = width(das), width(cap), float(cap.max() / das.max())
            print(f"\nA={A} f#={fn}: width DAS {w_das:.2f} px, Capon {w_cap:.2f} px, peak ratio {peak:.4f}")
            assert w_cap < 0.25 * w_das, (A, fn, w_cap, w_das)
            assert abs(peak - 1.0) <= 0.01, (A, fn, peak)
