"""p-DAS and F-DMAS (include/pbrt_hip.h) restated in NumPy for test_nlbf_restatement.py (CPU) and test_gpu_nlbf.py
(GPU): the definitions, written from the papers' formulas and sharing no text with the kernel.

  delayed          the delayed samples s_e of every transmission and the elements U(a) a pixel uses -- positions, range and aperture
                   rules of oracle/beamform.py as das_util / convex_util state them (line of elements [E], or element table [E, 4])
  beamform         p-DAS / F-DMAS / DAS of those samples -> (image, B), B the per-pixel scale the device is compared on; in float64,
                   or with every sample, root, sum and power in np.float32 (the float32 floor of the GPU test)
  fdmas_pairwise   the O(E^2) sum over pairs F-DMAS is defined by
  margins          the pixels das_util leaves out (range and aperture edges, rounding ties)
  fir              the axial FIR by np.convolve
  point_scatterer  channel data of one scatterer, and the -6 dB lateral width of an image's envelope through it
"""
import numpy as np

import convex_util as cu
import das_util as du
from oracle import beamform as obf


def _table(elem):
    return np.ndim(elem) == 2 and np.shape(elem)[1] == 4


def _positions(tx, elem, x, z, fs, c, t0, f_number):
    """for every transmission: (s [E, nx, nz] sample positions in f64, use [E, nx, nz] the receive aperture, and the two parts of s:
    the transmit part (t_tx - t0) fs [nx, nz] and the receive part dist / c fs [E, nx, nz])"""
    fn = float(np.float32(f_number or 0.0))
    c64, fs64, t064 = float(np.float32(c)), float(np.float32(fs)), float(np.float32(t0))
    if not _table(elem):
        z64 = du.f64(z).ravel()[None, None, :]
        t_tx = du.first_arrival(tx, elem, x, z, c)
        for a, (s, dx) in enumerate(du.positions(np.atleast_2d(tx), elem, x, z, fs, c, t0)):
            use = np.abs(dx) <= z64 / (2.0 * fn) if fn > 0 else np.ones(s.shape, bool)
            yield s, use, (t_tx[a] - t064) * fs64, np.sqrt(dx * dx + z64 * z64) / c64 * fs64
        return
    tx, el, gx, gz = du.f64(np.atleast_2d(tx)), du.f64(elem).reshape(-1, 4), du.f64(x).ravel(), du.f64(z).ravel()
    X, Z = np.meshgrid(gx, gz, indexing="ij")
    dx, dz = X[None] - el[:, 0, None, None], Z[None] - el[:, 1, None, None]
    dist = np.sqrt(dx * dx + dz * dz)
    dn = dx * el[:, 2, None, None] + dz * el[:, 3, None, None]
    dt = dx * el[:, 3, None, None] - dz * el[:, 2, None, None]
    use = (dn > 0) & (2.0 * fn * np.abs(dt) <= dn) if fn > 0 else np.ones(dist.shape, bool)
    for a in range(tx.shape[0]):
        t_tx = np.min(tx[a][:, None, None] + dist / c64, axis=0)
        yield (t_tx[None] + dist / c64 - t064) * fs64, use, (t_tx - t064) * fs64, dist / c64 * fs64


def _split(s):
    """a float64 position as whole samples and a float32 fraction in [0, 1) -- the format the header gives the positions of a sum"""
    whole = np.floor(s)
    frac = (s - whole).astype(np.float32)
    up = frac >= 1.0
    return whole + up, np.where(up, np.float32(0), frac)


def delayed(data, tx, elem, x, z, fs, c, t0=0.0, f_number=1.0, interpolation="linear", dtype=np.float64):
    """for every transmission a: (s_e [E, nx, nz] in `dtype`, ok [E, nx, nz]: e in U(a)).  The sample POSITION is evaluated in float64
    in either case; with dtype float32 its transmit and receive parts are then each split into whole samples and a float32 fraction,
    the fractions are added in float32 (include/pbrt_hip.h: "kept as whole samples plus an f32 fraction"), and the interpolation runs
    in float32.  Which elements a pixel uses is decided by the float64 position in both."""
    data = np.asarray(data, np.float32).astype(dtype)
    A, E, T = data.shape
    ee = np.arange(E)[:, None, None]
    for a, (s, use, s_tx, s_rx) in enumerate(_positions(tx, elem, x, z, fs, c, t0, f_number)):
        if interpolation == "nearest":
            r = np.rint(s)
            ok = (r >= 0) & (r <= T - 1) & use
            val = data[a][ee, np.clip(r, 0, T - 1).astype(int)]
        else:
            f = np.floor(s)
            ok = (((f >= 0) & (f < T - 1)) | (s == T - 1)) & use
            if dtype is np.float32:
                (ti, tf), (ri, rf) = _split(s_tx), _split(s_rx)
                fr = tf[None] + rf                       # float32, [0, 2)
                carry = np.floor(fr)
                f, w = ti[None] + ri + carry, fr - carry
            else:
                w = (s - f).astype(np.float32).astype(dtype)   # the weight is a float32 in the f64 statement too (oracle/beamform.py)
            i0 = np.clip(f, 0, T - 1).astype(int)
            i1 = np.clip(i0 + 1, 0, T - 1)
            v0, v1 = data[a][ee, i0], data[a][ee, i1]
            val = v0 + w * (v1 - v0)
        yield val.astype(dtype), ok


def signed_root(v, p, dtype=np.float64):
    v = np.asarray(v, dtype)
    r = np.sqrt(np.abs(v)) if p == 2 else np.power(np.abs(v), dtype(1) / dtype(p))
    return (np.sign(v) * r).astype(dtype)


def signed_power(q, p, dtype=np.float64):
    q = np.asarray(q, dtype)
    m = np.abs(q)
    return (np.sign(q) * (m * m if p == 2 else np.power(m, dtype(p)))).astype(dtype)


def beamform(method, data, tx, elem, x, z, fs, c, p=2.0, t0=0.0, f_number=1.0, interpolation="linear", compound="sum",
             dtype=np.float64):
    """method 'das' | 'pdas' | 'fdmas' -> (image [nx, nz], B [nx, nz]).  Per transmission a, over the elements U(a) of the pixel:
         pdas   r_e = sgn(s_e) |s_e|^(1/p), q = sum r_e, y = sgn(q) |q|^p                       B_a = (sum |r_e|)^p
         fdmas  r_e = sgn(s_e) sqrt|s_e|,   y = ((sum r_e)^2 - sum |s_e|) / 2                    B_a = ((sum |r_e|)^2 + sum |s_e|) / 2
         das    y = sum s_e                                                                    B_a = sum |s_e|
       image = sum_a y_a (/ A for 'mean'), B = sum_a B_a (likewise): the size of what is added up, which does not cancel."""
    A = np.shape(data)[0]
    img = B = None
    for val, ok in delayed(data, tx, elem, x, z, fs, c, t0, f_number, interpolation, dtype):
        val = np.where(ok, val, dtype(0))
        mag = np.abs(val).sum(axis=0, dtype=dtype)
        if method == "das":
            y, b = val.sum(axis=0, dtype=dtype), mag
        else:
            pp = 2 if method == "fdmas" else p
            r = signed_root(val, pp, dtype)
            q, qa = r.sum(axis=0, dtype=dtype), np.abs(r).sum(axis=0, dtype=dtype)
            if method == "fdmas":
                y, b = dtype(0.5) * (q * q - mag), dtype(0.5) * (qa * qa + mag)
            else:
                y, b = signed_power(q, pp, dtype), signed_power(qa, pp, dtype)
        img = y if img is None else img + y
        B = b if B is None else B + b
    if compound == "mean":
        img, B = img / dtype(A), B / dtype(A)
    return img, B


def fdmas_pairwise(s):
    """sum_{i < j} r_i r_j, r = sgn(s) sqrt|s|, pair by pair (Matrone et al. 2015, eq. 3 - 4)"""
    r = np.sign(s) * np.sqrt(np.abs(s))
    return sum(r[i] * r[j] for i in range(len(r)) for j in range(i + 1, len(r)))


def fdmas_closed(s):
    r = np.sign(s) * np.sqrt(np.abs(s))
    return 0.5 * (np.sum(r) ** 2 - np.sum(np.abs(s)))


def margins(tx, elem, x, z, T, fs, c, t0=0.0, f_number=1.0, interpolation="linear"):
    """-> (left_out [nx, nz], n_terms per transmission [A, nx, nz]): pixels with a pair within das_util's edge margins (`excluded`,
    and `ties` for nearest), and N_a, the elements a pixel uses per transmission"""
    tx = np.atleast_2d(tx)
    A, E = tx.shape
    kw = dict(t0=t0, f_number=f_number, interpolation=interpolation)
    n_a = []
    if _table(elem):
        _, _, excluded, ties = cu.das(np.ones((A, E, T), np.float32), tx, elem, x, z, fs, c, **kw)
    else:
        _, excluded, ties = du.contributions(tx, elem, x, z, T, fs, c, **kw)
    for _, ok in delayed(np.ones((A, E, T), np.float32), tx, elem, x, z, fs, c, **kw):
        n_a.append(ok.sum(axis=0))
    return excluded | ties, np.stack(n_a).astype(np.float64)


def fir(img, taps):
    """out[ix, n] = sum_k taps[K + k] img[ix, n - k], zero outside the column, in f64: np.convolve, cut to the column (mode 'same'
    for a column no shorter than the taps; 'same' keeps the LONGER operand's length, so the cut is written out)"""
    x, h = np.atleast_2d(np.asarray(img, np.float64)), np.asarray(taps, np.float64).ravel()
    K = len(h) // 2
    return np.stack([np.convolve(row, h, mode="full")[K:K + x.shape[1]] for row in x])


# ---- a point scatterer -------------------------------------------------------------------------------------------------
def point_scatterer(E=32, A=3, nx=41, nz=96, f0=3.0e6, c=1540.0, fs=40.0e6, depth=6.0e-3, cycles=1.5):
    """Channel data of one scatterer at (0, depth) under a line of E elements at lambda / 2 pitch: per (transmission, element) one
    Gaussian-windowed pulse cos(2 pi f0 (t - tau)) exp(-((t - tau) / sigma)^2), tau the scatterer's own delay (first arrival +
    return path), sigma = cycles / (2 f0).  The scan is nx x nz pixels at lambda / 16 centred on the scatterer.
    -> dict(data, tx, ex, x, z, fs, c, f0, ix, iz); x and z stay float64 (a float32 axis is not uniform to 1e-6 of this step)"""
    lam = c / f0
    ex = (np.arange(E) - (E - 1) / 2) * (lam / 2)
    angles = np.deg2rad(np.linspace(-6.0, 6.0, A)) if A > 1 else np.zeros(1)
    tx = ex[None, :] * np.sin(angles)[:, None] / c
    step = lam / 16
    x = (np.arange(nx) - nx // 2) * step
    z = depth + (np.arange(nz) - nz // 2) * step
    dist = np.sqrt(ex ** 2 + depth ** 2)
    t_tx = np.min(tx + dist[None] / c, axis=1)
    tau = t_tx[:, None] + dist[None] / c                    # [A, E]
    T = int(np.ceil(tau.max() * fs)) + 64
    t = np.arange(T)[None, None, :] / fs - tau[:, :, None]
    sigma = cycles / (2.0 * f0)
    data = (np.cos(2 * np.pi * f0 * t) * np.exp(-(t / sigma) ** 2)).astype(np.float32)
    return dict(data=data, tx=tx.astype(np.float32), ex=ex.astype(np.float32), x=x, z=z, fs=fs,
                c=c, f0=f0, ix=nx // 2, iz=nz // 2)


def lateral_width(rf, iz, level=0.5):
    """-6 dB width (in pixels, edges interpolated) of the envelope's lateral profile at depth index iz, around its maximum"""
    prof = obf.envelope(rf)[:, iz]
    k = int(np.argmax(prof))
    thr = level * prof[k]

    def reach(step):
        i = k
        while 0 <= i + step < len(prof) and prof[i + step] >= thr:
            i += step
        j = i + step
        if not 0 <= j < len(prof):
            return float("inf")       # the profile never falls to the level inside the scan
        return abs(i - k) + (prof[i] - thr) / (prof[i] - prof[j])

    return reach(-1) + reach(+1)


# ---- non-finite samples (test_imgform_nonfinite_restatement.py on the CPU, test_gpu_imgform_nonfinite.py on the GPU) --------------
FINITE, NAN, POS_INF, NEG_INF = 0, 1, 2, 3


def classes(img):
    """the class of every value -- FINITE, NAN, POS_INF or NEG_INF; a complex image gives [..., 2], its real and imaginary parts"""
    img = np.asarray(img)
    if np.iscomplexobj(img):
        return np.stack([classes(img.real), classes(img.imag)], axis=-1)
    out = np.full(img.shape, FINITE, np.uint8)
    out[np.isnan(img)] = NAN
    out[img == np.inf] = POS_INF
    out[img == -np.inf] = NEG_INF
    return out


def sample_reads(tx, elem, x, z, T, fs, c, t0=0.0, f_number=1.0, interpolation="linear"):
    """for every transmission a: (lo, hi, ok, wlo, whi), each [E, nx, nz].  Where ok, the pair (a, e) of the pixel reads the samples
    lo .. hi of its trace (the float64 position's window: floor(s) and the next sample, or the rounded one).  A position within
    das_util.EDGE_SAMPLES of a whole sample (linear) or of a half sample (nearest) may take the neighbouring window in another order
    of operations, or meet a weight of exactly 0 there: a bad sample in wlo .. whi leaves the pixel's class open (wlo > whi: none)"""
    for s, use, _, _ in _positions(tx, elem, x, z, fs, c, t0, f_number):
        fl = np.floor(s)
        if interpolation == "nearest":
            r = np.rint(s)
            ok = (r >= 0) & (r <= T - 1) & use
            lo = hi = r
            near = np.abs(s - fl - 0.5) < du.EDGE_SAMPLES
            wlo, whi = fl, fl + 1
        else:
            ok = (((fl >= 0) & (fl < T - 1)) | (s == T - 1)) & use
            lo, hi = fl, np.minimum(fl + 1, T - 1)
            n = np.rint(s)
            near = np.abs(s - n) < du.EDGE_SAMPLES
            wlo, whi = n - 1, n + 1
        near &= use
        yield (np.clip(lo, 0, T - 1).astype(int), np.clip(hi, 0, T - 1).astype(int), ok,
               np.where(near, wlo, 1).astype(int), np.where(near, whi, 0).astype(int))


def read_mask(g, T, c):
    """[A, E, T]: the samples that at least one kept pixel of the case g (walk_cases.geometry) reads"""
    keep = ~g["left_out"]
    kw = g["kw"]
    M = np.zeros((g["A"], g["E"], T), bool)
    ee = np.broadcast_to(np.arange(g["E"])[:, None, None], (g["E"],) + keep.shape)
    for a, (lo, hi, ok, _, _) in enumerate(sample_reads(g["tx"], g["elem"], g["x"], g["z"], T, g["fs"], c, f_number=kw["f_number"],
                                                        interpolation=kw["interpolation"])):
        sel = ok & keep[None]
        M[a][ee[sel], lo[sel]] = True
        M[a][ee[sel], hi[sel]] = True
    return M


def bad_sites(g, T, c, n, seed):
    """n sites (a, e, t) that kept pixels read -- spread over the transmissions (every trip of angles) and over the elements in use, the
    first and the last of them included (every block of 64) -- and, where some trace lies outside every kept pixel's aperture, one site
    in such a trace, which must change nothing.  -> (sites [(a, e, t)], idle: the site no pixel reaches, or None)"""
    M = read_mask(g, T, c)
    rng = np.random.default_rng(seed)
    A = g["A"]
    sites = []
    for k in range(n):
        a = (k * A) // n if k < n - 1 else A - 1
        used = np.flatnonzero(M[a].any(axis=1))
        e = int(used[int(round(k / max(n - 1, 1) * (len(used) - 1)))])
        sites.append((int(a), e, int(rng.choice(np.flatnonzero(M[a, e])))))
    idle = None
    unused = np.flatnonzero(~M.any(axis=(0, 2)))
    if len(unused):
        idle = (A // 2, int(unused[len(unused) // 2]), T // 2)
        sites.append(idle)
    return sites, idle


def near_bad(g, T, c, sites):
    """[nx, nz]: pixels with a pair whose interpolation window lies next to a bad sample and whose position lies within
    das_util.EDGE_SAMPLES of a whole sample (linear) or of a half sample (nearest): left out, like the pixels of `margins`"""
    kw = g["kw"]
    out = np.zeros(g["left_out"].shape, bool)
    for a, (_, _, _, wlo, whi) in enumerate(sample_reads(g["tx"], g["elem"], g["x"], g["z"], T, g["fs"], c, f_number=kw["f_number"],
                                                         interpolation=kw["interpolation"])):
        for sa, e, t in sites:
            if sa == a:
                out |= (wlo[e] <= t) & (t <= whi[e])
    return out


def with_bad(data, sites, value):
    """a copy of the channel data with `value` at every site"""
    out = np.array(data, copy=True)
    for a, e, t in sites:
        out[a, e, t] = value
    return out


def fir_bad_mask(nz, K, j):
    """the outputs of a column of nz that a bad sample at index j reaches: |n - j| <= K"""
    return np.abs(np.arange(nz) - j) <= K


def bad_reads(bad, tx, elem, x, z, fs, c, t0=0.0, f_number=1.0, interpolation="linear"):
    """bad [A, E, T]: the non-finite samples of some channel data -> (sure, open), each [nx, nz].  sure: a pair of the pixel reads a
    bad sample and its position lies clear of every whole (linear) or half (nearest) sample; open: a pair within
    das_util.EDGE_SAMPLES of one has a bad sample in the window it may take.  A pixel that is open and not sure has a class that rests
    on such pairs alone."""
    bad = np.asarray(bad, bool)
    A, E, T = bad.shape
    count = np.concatenate([np.zeros((A, E, 1), np.int64), np.cumsum(bad, axis=2)], axis=2)      # count[..., k]: bad samples below k
    ee = np.arange(E)[:, None, None]
    sure = open_ = None
    for a, (lo, hi, ok, wlo, whi) in enumerate(sample_reads(tx, elem, x, z, T, fs, c, t0, f_number, interpolation)):
        near = wlo <= whi
        hit = ok & ~near & (count[a][ee, hi + 1] - count[a][ee, lo] > 0)
        w0, w1 = np.clip(wlo, 0, T), np.clip(whi + 1, 0, T)
        maybe = near & (w1 > w0) & (count[a][ee, np.maximum(w1, w0)] - count[a][ee, w0] > 0)
        sure = hit.any(axis=0) if sure is None else sure | hit.any(axis=0)
        open_ = maybe.any(axis=0) if open_ is None else open_ | maybe.any(axis=0)
    return sure, open_
