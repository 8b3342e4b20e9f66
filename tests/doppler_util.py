"""Colour and power Doppler (include/pbrt_hip.h) restated in NumPy for test_doppler_restatement.py (CPU) and
test_gpu_doppler.py (GPU), and for their non-finite and rescaled cases (test_doppler_nonfinite_restatement.py, test_gpu_doppler_edges.py): the slow-time autocorrelation with its polynomial regression (wall) filter and the maps made of it, written
from the header's formulas and sharing no text with the kernels.

  basis     the orthonormal polynomial basis on N slow-time points, float64 (Gram-Schmidt; the package's wall_basis is held to it)
  weights   a smoothing window as the library makes it: float64, normalised, rounded once to float32
  autocorr  frames [N, nx, nz] complex, q [d + 1, N] or None -> (acf [3, nx, nz], B [3, nx, nz])
  smooth    acf, B -> the smoothed planes and their B
  maps      acf -> a dict: planes, B, velocity, amplitude, B_amp

Both steps run in float64, or with dtype=np.float32 modelling the stated order and precisions (float32 products and sums in the order
of the header; a fused multiply-add is modelled by a product and a sum, as iq_util does: the float32 runs set the floor the device is
compared on).  B per pixel and plane is the sum of the absolute values of everything added up, through filter, correlation and
smoothing: with X_n = |x_n| per component (|x_n| + |x_0| under a wall filter, which works on x_n - x_0), Y_n = X_n + sum_k |q[k][n]|
sum_m |q[k][m]| X_m bounds the filtered sample, and
  B(Re R1) = sum_n (Yr_n Yr_{n-1} + Yi_n Yi_{n-1}),  B(Im R1) = sum_n (Yi_n Yr_{n-1} + Yr_n Yi_{n-1}),  B(R0) = sum_n (Yr_n^2 + Yi_n^2) / N;
the smoothing, whose weights are positive, is applied to B as it is to the planes.  plate_scene and plate_frames are the moving-plate
experiment of DESIGN D24 on the CPU oracle's acquisition."""
import math

import numpy as np

import iq_util as iu

F32_EPS = 2.0 ** -24


def basis(N, d):
    """[d + 1, N] float64: Gram-Schmidt on 1, t, t^2, ... over the centred points, leading coefficients positive"""
    t = (np.arange(N, dtype=np.float64) - (N - 1) / 2.0) / ((N - 1) / 2.0)
    rows = []
    for k in range(d + 1):
        v = t ** k
        for _ in range(2):   # (twice: the second pass removes what rounding left of the first)
            for r in rows:
                v = v - np.dot(r, v) * r
        rows.append(v / np.sqrt(np.dot(v, v)))
    return np.stack(rows)


def weights(window, k):
    """the k-point window of pbrt_doppler_maps as float64 values of its float32 weights"""
    h = [0.54 - 0.46 * math.cos(2.0 * math.pi * i / (k - 1)) if window == "hamming" and k > 1 else 1.0 for i in range(k)]
    s = 0.0
    for v in h:
        s += v
    return np.array([v / s for v in h], np.float64).astype(np.float32).astype(np.float64)


def autocorr(frames, q=None, dtype=np.float64):
    """frames [N, nx, nz] complex (read as complex64), q [d + 1, N] (read as float32) or None -> (acf [3, nx, nz] float64, B)"""
    x = np.asarray(frames, np.complex64)
    N = x.shape[0]
    xr, xi = x.real.astype(dtype), x.imag.astype(dtype)
    Xr, Xi = np.abs(x.real.astype(np.float64)), np.abs(x.imag.astype(np.float64))
    yr, yi, Yr, Yi = xr.copy(), xi.copy(), Xr.copy(), Xi.copy()
    if q is not None:
        q = np.asarray(q, np.float32)
        qd, qa = q.astype(dtype), np.abs(q.astype(np.float64))
        xr, xi = xr - xr[0], xi - xi[0]           # the filter works on u_n = x_n - x_0 (one subtraction in `dtype`)
        Xr, Xi = Xr + Xr[0], Xi + Xi[0]
        yr, yi, Yr, Yi = xr.copy(), xi.copy(), Xr.copy(), Xi.copy()
        for k in range(q.shape[0]):
            cr, ci = np.zeros(x.shape[1:], dtype), np.zeros(x.shape[1:], dtype)
            for n in range(N):          # the coefficients from the UNfiltered samples, n ascending
                cr = cr + qd[k, n] * xr[n]
                ci = ci + qd[k, n] * xi[n]
            for n in range(N):          # k ascending per frame: this loop nest subtracts row k from every frame before row k + 1
                yr[n] = yr[n] - qd[k, n] * cr
                yi[n] = yi[n] - qd[k, n] * ci
            Cr, Ci = np.tensordot(qa[k], Xr, 1), np.tensordot(qa[k], Xi, 1)
            Yr += qa[k][:, None, None] * Cr[None]
            Yi += qa[k][:, None, None] * Ci[None]
    r0 = np.zeros(x.shape[1:], dtype)
    re, im = r0.copy(), r0.copy()
    for n in range(N):
        r0 = (r0 + yi[n] * yi[n]) + yr[n] * yr[n]
        if n:
            re = (re + yi[n] * yi[n - 1]) + yr[n] * yr[n - 1]
            im = (im - yr[n] * yi[n - 1]) + yi[n] * yr[n - 1]
    acf = np.stack([re, im, r0 / dtype(N)]).astype(np.float64)
    B = np.stack([(Yr[1:] * Yr[:-1] + Yi[1:] * Yi[:-1]).sum(0), (Yi[1:] * Yr[:-1] + Yr[1:] * Yi[:-1]).sum(0), (Yr * Yr + Yi * Yi).sum(0) / N])
    return acf, B


def _along(a, w, axis, dtype):
    """sum_j w[j] a[.. i + j - h ..] along `axis`, zero outside, j ascending.  The sum starts from -0.0, as the header states: then its
    first term is the product itself, the sign of a zero included, and a 1-point window is the identity on -0.0 too"""
    k, h = len(w), len(w) // 2
    a = np.moveaxis(np.asarray(a, dtype), axis, -1)
    n = a.shape[-1]
    pad = np.concatenate([np.zeros(a.shape[:-1] + (h,), dtype), a, np.zeros(a.shape[:-1] + (h,), dtype)], axis=-1)
    acc = np.full(a.shape, -0.0, dtype)
    for j in range(k):
        acc = acc + dtype(w[j]) * pad[..., j:j + n]
    return np.moveaxis(acc, -1, axis)


def smooth(planes, window, kernel, dtype=np.float64):
    """planes [.., nx, nz] -> the same, smoothed along z first and then along x"""
    kx, kz = kernel
    return _along(_along(planes, weights(window, kz), -1, dtype), weights(window, kx), -2, dtype).astype(np.float64)


def maps(acf, nyquist_velocity, window="hamming", kernel=(1, 1), dtype=np.float64, B=None):
    """acf [3, nx, nz] (read as float32; B: its bound, default |acf|) -> dict(planes, B, velocity, amplitude, B_amp)"""
    a = np.asarray(acf, np.float32)
    s = smooth(a, window, kernel, dtype)
    Bs = smooth(np.abs(a.astype(np.float64)) if B is None else B, window, kernel)
    if dtype is np.float32:
        scale = np.float32(float(np.float32(nyquist_velocity)) / math.pi)
        vel = (scale * np.arctan2(s[1], s[0]).astype(np.float32)).astype(np.float64)
        amp = np.sqrt(s[2].astype(np.float32)).astype(np.float64)
    else:
        vel = float(np.float32(nyquist_velocity)) / math.pi * np.arctan2(s[1], s[0])
        amp = np.sqrt(s[2])
    vel = np.where((s[0] == 0) & (s[1] == 0), 0.0, vel)
    return dict(planes=s, B=Bs, velocity=vel, amplitude=amp, B_amp=np.sqrt(Bs[2]))


def floor_of(f32, f64, B):
    """the float32 floor of a case: the largest |float32 restatement - float64| / B (pixels with B == 0 hold exact zeros)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(B > 0, np.abs(f32 - f64) / B, 0.0)
    return float(r.max())


def ratio_of(dev, f64, B):
    """the device's largest |device - float64| / B; a pixel with B == 0 must be exact"""
    dev = np.asarray(dev, np.float64)
    assert np.all(dev[B == 0] == f64[B == 0])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(B > 0, np.abs(dev - f64) / B, 0.0)
    return float(r.max())


def velocity_bound(m64, nyquist_velocity, floor):
    """(bound [nx, nz], kept [nx, nz]) of the velocity rule: |device - float64| <= (nyq / pi) (4 floor B_R1 / |R1| + 8 2^-24 pi) on the
    pixels with |R1 smoothed| >= 1e-3 B_R1; B_R1 = B(Re R1) + B(Im R1), which bounds the error of both components (a pixel whose
    R1 is exactly zero has velocity exactly 0 on both sides: the second term alone)"""
    s, B = m64["planes"], m64["B"]
    r1, b1 = np.hypot(s[0], s[1]), B[0] + B[1]
    kept = r1 >= 1e-3 * b1
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = float(np.float32(nyquist_velocity)) / math.pi * (np.where(r1 > 0, 4.0 * floor * b1 / r1, 0.0) + 8.0 * F32_EPS * math.pi)
    return bound, kept


def ensemble(rng, N, shape, d=None, clutter=1e3):
    """random complex frames [N, *shape] complex64, plus (d is not None) a clutter polynomial of degree d in n, `clutter` times stronger"""
    x = rng.normal(size=(N,) + shape) + 1j * rng.normal(size=(N,) + shape)
    if d is not None:
        t = (np.arange(N) - (N - 1) / 2.0) / ((N - 1) / 2.0)
        for k in range(d + 1):
            x = x + clutter * (rng.normal(size=shape) + 1j * rng.normal(size=shape))[None] * (t ** k)[:, None, None]
    return x.astype(np.complex64)


def tone(rng, N, shape, noise=0.1):
    """a pure-tone ensemble A exp(i phi n), A and phi per pixel, plus `noise` of complex noise"""
    A = rng.uniform(0.5, 2.0, shape) * np.exp(2j * np.pi * rng.uniform(size=shape))
    phi = rng.uniform(-0.9 * np.pi, 0.9 * np.pi, shape)
    x = A[None] * np.exp(1j * phi[None] * np.arange(N)[:, None, None])
    return (x + noise * (rng.normal(size=x.shape) + 1j * rng.normal(size=x.shape)) / np.sqrt(2)).astype(np.complex64)


# ---- the moving plate of DESIGN D24: 32 elements, one 0 degree transmission, 8 pulses, the plate moved by dz between pulses ----------
PLATE = dict(n_elements=32, pitch=2e-4, fs=40e6, f=4e6, c=1500.0, T=1400, ppr=256, seed=3, pulses=8)
LAM = PLATE["c"] / PLATE["f"]
PLATE_X = np.linspace(-2e-3, 2e-3, 5)
PLATE_Z = np.arange(18.5e-3, 22e-3, LAM / 2)


def plate_scene(mi, z_plate, pulse_model="gaussian"):
    """us_util.phantom("plate") with the plate at depth z_plate, max_depth 2 and the pulse model asked for"""
    T = mi.ScalarTransform4f
    p = PLATE
    return mi.load_dict({
        "type": "scene",
        "integrator": {"type": "ultrasound_integrator", "max_depth": 2, "sampling_rate": p["fs"], "frequency": p["f"], "sound_speed": p["c"],
                       "attenuation": 0.3, "main_beam_angle": 20, "cutoff_angle": 35, "n_elements": p["n_elements"], "pitch": p["pitch"],
                       "time_samples": p["T"], "angles": np.asarray([0.0], np.float32), "paths_per_ray": p["ppr"], "seed": p["seed"],
                       "primary_rays": "element", "pulse_model": pulse_model},
        "sensor": {"type": "ultrasound_sensor", "to_world": T().look_at([0, 0, 0], [0, 0, 0.03], [0, 1, 0])},
        "p": {"type": "rectangle", "to_world": T().translate([0, 0, float(z_plate)]) @ T().rotate([0, 1, 0], 4) @ T().rotate([1, 0, 0], 180)
              @ T().scale([0.03, 0.03, 1]), "bsdf": {"type": "ultrasound_bsdf", "impedance": 7.8, "roughness": 0.8}}})


def plate_scenes(mi, dz, pulse_model="gaussian"):
    return [plate_scene(mi, 0.02 + n * dz, pulse_model) for n in range(PLATE["pulses"])]


def plate_frames(mi, ob, obf, dz, pulse_model="gaussian"):
    """the eight beamformed I/Q frames [8, 5, 19] of the plate moved by dz per pulse, by the reference chain: the CPU oracle's
    acquisition, oracle/beamform.py apply_pulse (gaussian), iq_util.rf2iq and iq_util.iq_beamform, in float64"""
    p = PLATE
    frames = []
    for sc in plate_scenes(mi, dz, pulse_model):
        ui = sc.integrator()
        buf, tx = ob.OracleScene.from_scene(sc).us_acquire(ui.us_params(sc), ui.seed, p["ppr"])
        buf = np.asarray(buf, np.float64).reshape(1, p["n_elements"], p["T"])
        if pulse_model == "gaussian":
            buf = obf.apply_pulse(buf, p["fs"], p["f"], ui.pulse_sigma)
        taps = mi.lowpass_taps(p["f"] / 2, p["fs"])
        iq, _ = iu.rf2iq(buf.reshape(p["n_elements"], p["T"]), p["fs"], 0.0, p["f"], 1, taps)
        elem = p["pitch"] * (np.arange(p["n_elements"]) - (p["n_elements"] - 1) / 2)
        img, _ = iu.iq_beamform(iq.reshape(1, p["n_elements"], -1), np.asarray(tx, np.float64).reshape(1, -1), elem, PLATE_X, PLATE_Z,
                                p["fs"], p["c"], p["f"])
        frames.append(img)
    return np.stack(frames)


def phase_over_pi(frames, q=None):
    """(median of arg R1 / pi over the pixels with R0 >= 0.1 max, their number, min |R1| / ((N - 1) R0) there)"""
    acf, _ = autocorr(frames, q)
    keep = acf[2] >= 0.1 * acf[2].max()
    arg = np.arctan2(acf[1], acf[0])[keep] / np.pi
    coh = (np.hypot(acf[0], acf[1]) / ((len(frames) - 1) * acf[2]))[keep]
    return float(np.median(arg)), int(keep.sum()), float(coh.min())
