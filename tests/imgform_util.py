"""Shared by the image-formation tests (test_imgform_bound.py on the CPU, test_gpu_imgform_shapes.py on the GPU): per-sample bounds
that the float32 kernels k_hilbert_env / k_hilbert_env_even, k_env_max + k_log_compress and k_apply_pulse (csrc/kernels_beamform.h)
are held to against the f64 restatement of oracle/beamform.py, and numpy emulations of their float32 arithmetic in their own order.

u = 2^-24 is the unit roundoff of float32; "k ulp" of a float32 result x is at most 2 k u |x|.  Each bound is derived in the
docstring of the function that computes it."""
import numpy as np

from oracle import beamform as obf

U32 = 2.0 ** -24
K_ENV = 4.0        # envelope: taps rounded to f32 (1) and slack for the second-order terms
C_ENV = 4.0        # envelope: y * y, the fma with x * x and the sqrt (2 u env), doubled
EPS_FFT = 1e-13    # f64 FFT noise of the restatement, per unit of sum |x| of the column
LOG10F_ULP = 3.0   # log10f: the OpenCL single-precision limit (device library); glibc's log10f is within 2 ulp of the true value
C_SUM_PULSE = 2.0  # pulse: the tap product rounding and the second-order terms of the fma chain
C_TAP = 16.0       # pulse: sinpif and expf (<= 4 ulp each on the device, <= 1 ulp in the emulation) and the product of the two


# ---- envelope ---------------------------------------------------------------------------------------------------------------
def hilbert_taps(N):
    """h[k], 0 <= k < N: the discrete Hilbert kernel of the FFT definition (kernels_beamform.h: 2/N cot(pi k/N) for even N and odd k,
    0 for even k; -1/N tan(pi k/2N) (k even) and 1/N cot(pi k/2N) (k odd) for odd N), in f64; h[N - k] = -h[k]"""
    k = np.arange(N, dtype=np.float64)
    h = np.zeros(N)
    if N % 2 == 0:
        odd = k % 2 == 1
        h[odd] = 2.0 / N / np.tan(np.pi * k[odd] / N)
    else:
        ev = (k % 2 == 0) & (k > 0)
        od = k % 2 == 1
        h[ev] = -np.tan(0.5 * np.pi * k[ev] / N) / N
        h[od] = 1.0 / np.tan(0.5 * np.pi * k[od] / N) / N
    return h


def circulant(h):
    """A[n, m] = h[(n - m) mod N]: y = A @ x is the circular convolution, summed directly (no FFT)"""
    N = len(h)
    idx = (np.arange(N)[:, None] - np.arange(N)[None, :]) % N
    return h[idx]


def nonzero_taps(N):
    """terms of the fma chain of one output that are not exactly 0: every tap for odd N, the odd ones for even N"""
    return N // 2 if N % 2 == 0 else max(N - 1, 0)


class EnvBound:
    """Per-sample bound of a float32 envelope against obf.envelope, for columns of length N.  The kernels form the imaginary part
    y_n = sum_m x_m g[(n - m)], g the f64 taps rounded to f32 (|g - h| <= u |h|), as an fma chain over m in increasing order
    (k_hilbert_env: every m; k_hilbert_env_even: the m of the other parity -- a zero tap leaves the accumulator as it is), and
    env_n = sqrt(fma(x_n, x_n, y_n * y_n)).
      - the chain: each of its n_t roundings is <= u times a partial sum, so |y - sum x g| <= n_t u sum |x g|;
      - the taps: |sum x g - sum x h| <= u S_n, S_n = sum_m |x_m| |h[(n - m) mod N]| (f64, direct circular convolution: an FFT's
        rounding is relative to the column's maximum, not to S_n, and a spike column has S_n = 0 at half of its samples);
      - d env / d y = y / env lies in [-1, 1], so the error of y passes on at most as it is;
      - y * y (u y^2), the fma (u env^2) and the sqrt (u env / 2): <= 2 u env;
      - the restatement's own f64 FFT: EPS_FFT sum |x| per column covers it (where S_n = 0 the kernel's result is exact).
    bound_n = (n_t + K_ENV) u S_n + C_ENV u ref_n + EPS_FFT sum_m |x_m|,   n_t = nonzero_taps(N)."""

    def __init__(self, N):
        self.N = N
        self.h = hilbert_taps(N)
        self.absA = np.abs(circulant(self.h))   # made once per N, used for every column

    def S(self, rf):
        x = np.abs(np.asarray(rf, np.float32).astype(np.float64)).reshape(-1, self.N)
        return x @ self.absA.T

    def __call__(self, rf, ref=None):
        x = np.asarray(rf, np.float32).reshape(-1, self.N)
        if ref is None:
            ref = obf.envelope(x)
        S = self.S(x)
        col = np.abs(x.astype(np.float64)).sum(axis=1, keepdims=True)
        return (nonzero_taps(self.N) + K_ENV) * U32 * S + C_ENV * U32 * np.abs(ref) + EPS_FFT * col, ref


def f32_fma(a, b, c):
    """float32 fma: the product of two float32 is exact in float64, the sum rounds once there and once more to float32 (a double
    rounding that may differ from the single one of the hardware by one ulp in rare ties: far below every bound here)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def emulate_env(rf, parity_sums=False):
    """k_hilbert_env's float32 arithmetic: taps g = f32(h), the column read in quads (the last, partial one zero-padded), one
    fma chain per output over m = 0 .. Np - 1, then sqrtf(fma(x, x, y * y)).  parity_sums: k_hilbert_env_even's two sums -- an
    output of parity s runs its chain over the inputs of parity 1 - s only, in increasing order"""
    x = np.asarray(rf, np.float32)
    x = x.reshape(-1, x.shape[-1])
    C, N = x.shape
    Np = (N + 3) // 4 * 4
    xp = np.zeros((C, Np), np.float32)
    xp[:, :N] = x
    g = hilbert_taps(N).astype(np.float32)
    n = np.arange(N)
    acc = np.zeros((C, N), np.float32)
    for m in range(Np):
        k = n - m
        tap = np.where((np.abs(k) < N) & (np.abs(k) > 0), np.sign(k) * g[np.abs(k) % N], 0).astype(np.float32)
        if parity_sums:
            use = (n % 2) != (m % 2)
            acc[:, use] = f32_fma(xp[:, m:m + 1], tap[use][None, :], acc[:, use])
        else:
            acc = f32_fma(xp[:, m:m + 1], tap[None, :], acc)
    return np.sqrt(f32_fma(x, x, acc * acc)).astype(np.float32)


# ---- log compression --------------------------------------------------------------------------------------------------------
def log_bound(env, dr):
    """Per-pixel bound of k_env_max + k_log_compress against obf.log_compress.  The kernel computes, in float32,
    db = 20 log10f(e + 1e-12f), max_db the same of the maximum (exact: a maximum of float32 values), min_db = max_db - dr,
    out = (clamp(db, min_db, max_db) - min_db) / dr.
      - e + 1e-12f: the constant is within u of 1e-12 relative, the sum rounds: a relative error <= 2 u of its argument, i.e.
        <= 2 u / ln 10 in log10 and A = 40 / ln 10 u dB after the factor 20;
      - log10f: LOG10F_ULP ulp <= 2 LOG10F_ULP u |log10|, and the product by 20 one more rounding: B = 2 LOG10F_ULP + 1 times u |db|;
      - so |d db| <= (A + B |db|) u, and the same for max_db; min_db adds u |min_db| <= u (|max_db| + dr);
      - the clamp is 1-Lipschitz in db and in its limits (pixels near either edge need no special case);
      - db - min_db rounds (u dr after the clamp), the division by dr (exact in float32 here) rounds: u |out|.
    bound = u (2 A + (B + 1) (|db| + |max_db|) + 2 dr) / dr + u |out|, db and max_db of the f64 restatement."""
    e = np.asarray(env, np.float32).astype(np.float64)
    db = 20.0 * np.log10(e + 1e-12)
    mx = db.max()
    ref = obf.log_compress(np.asarray(env, np.float32), dr)
    A = 40.0 / np.log(10.0)
    B = 2.0 * LOG10F_ULP + 1.0
    bound = U32 * (2.0 * A + (B + 1.0) * (np.abs(db) + abs(mx)) + 2.0 * dr) / dr + U32 * np.abs(ref)
    return bound, ref


def emulate_log(env, dr):
    """k_env_max + k_log_compress in float32 (numpy's float32 log10 for log10f)"""
    e = np.asarray(env, np.float32)
    f20, eps, d = np.float32(20.0), np.float32(1e-12), np.float32(dr)
    gm = max(np.float32(e.max()), np.float32(0.0))
    max_db = f20 * np.log10(gm + eps)
    min_db = np.float32(max_db - d)
    db = f20 * np.log10(e + eps)
    db = np.minimum(np.maximum(db, min_db), max_db)
    return ((db - min_db) / d).astype(np.float32)


# ---- pulse ------------------------------------------------------------------------------------------------------------------
def pulse_tap_error(fs, fc, sigma):
    """-> (h, K, err): the f64 taps of obf.pulse_taps and a bound on |tap_f32 - h| per tap.  k_apply_pulse forms
    t = f32((i - K) / fs) (relative error u), the phase 2 fc t in float32 (2 fc exact, the product rounds: |d phase| <= 2 u |2 fc t|
    to first order) and sinpif of it: the phase error is ABSOLUTE in sin(pi phase), pi |d phase| <= pi 2^-23 |2 fc t| -- taken
    as pi 2^-22 |2 fc t| gauss, twice that.  The Gaussian exp(-(t t) / (sigma sigma)): t t, sigma sigma, the division -- 5 u of
    its argument a = t^2 / sigma^2, i.e. 5 u a gauss absolute -- and expf.  sinpif, expf (<= 4 ulp each on the device) and the
    product: C_TAP u |h|.
    err_k = pi 2^-22 |2 fc t_k| gauss_k + (C_TAP + 5 a_k) u |h_k|"""
    h, K = obf.pulse_taps(fs, fc, sigma)
    fs, fc, sg = float(np.float32(fs)), float(np.float32(fc)), float(np.float32(sigma))
    t = np.arange(-K, K + 1) / fs
    a = t * t / (sg * sg)
    gauss = np.exp(-a)
    err = np.pi * 2.0 ** -22 * np.abs(2.0 * fc * t) * gauss + (C_TAP + 5.0 * a) * U32 * np.abs(h)
    return h, K, err


def pulse_bound(traces, fs, fc, sigma):
    """Per-sample bound of k_apply_pulse against obf.apply_pulse: out[n] = sum_{|k| <= K} x[n - k] h_k as an fma chain of 2K + 1
    terms in float32 over the float32 taps:
      - the chain: (2 K + 1) u sum |x h|, and C_SUM_PULSE u sum |x h| for the second-order terms;
      - the taps: sum_k |x[n - k]| err_k (pulse_tap_error), a term of its own because the tap error is absolute in the phase.
    bound_n = (2 K + 1 + C_SUM_PULSE) u sum_k |x[n - k]| |h_k| + sum_k |x[n - k]| err_k  (f64 direct convolutions)"""
    x = np.abs(np.asarray(traces, np.float32).astype(np.float64))
    h, K, err = pulse_tap_error(fs, fc, sigma)
    flat = x.reshape(-1, x.shape[-1])
    T = x.shape[-1]
    ah = np.abs(h)
    out = np.stack([(2 * K + 1 + C_SUM_PULSE) * U32 * np.convolve(r, ah)[K:K + T] + np.convolve(r, err)[K:K + T] for r in flat])
    return out.reshape(x.shape)


def emulate_pulse_taps(fs, fc, sigma):
    """k_apply_pulse's taps in float32, with the exact sine of the float32 phase and the exact exponential of the float32 argument"""
    K = obf.pulse_taps(fs, fc, sigma)[1]
    fs32, fc32, sg32 = np.float32(fs), np.float32(fc), np.float32(sigma)
    i = np.arange(2 * K + 1)
    t = ((i.astype(np.float32) - np.float32(K)) / fs32).astype(np.float32)
    ph = (np.float32(2.0) * fc32 * t).astype(np.float32)
    s = np.sin(np.pi * ph.astype(np.float64)).astype(np.float32)
    arg = (-(t * t) / (sg32 * sg32)).astype(np.float32)
    return (s * np.exp(arg.astype(np.float64)).astype(np.float32)).astype(np.float32), K


def emulate_pulse(traces, fs, fc, sigma):
    """k_apply_pulse: acc = fma(in[n - k], h_k, acc) for k = -K .. K in this order, inputs outside the trace read as 0"""
    x = np.asarray(traces, np.float32)
    flat = x.reshape(-1, x.shape[-1])
    T = flat.shape[1]
    h, K = emulate_pulse_taps(fs, fc, sigma)
    pad = np.zeros((flat.shape[0], T + 2 * K), np.float32)
    pad[:, K:K + T] = flat
    acc = np.zeros(flat.shape, np.float32)
    for j in range(2 * K + 1):          # k = j - K: in[n - k] = pad[n + K - k] = pad[n + 2K - j]
        acc = f32_fma(pad[:, 2 * K - j:2 * K - j + T], h[j], acc)
    return acc.reshape(x.shape)


def excess(got, ref, bound):
    """|got - ref| / bound per sample: 0 where they are equal (the bound 0 included), inf where the bound is 0 and they differ,
    and inf where either is NaN or infinite -- a NaN written where the restatement is finite is a failure, not a skipped sample"""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / bound)
    return np.where(np.isfinite(got) & np.isfinite(ref) & ~np.isnan(r), r, np.inf)


def worst_ratio(got, ref, bound):
    """the largest excess (np.max, not np.nanmax: a NaN sample must fail)"""
    r = excess(got, ref, bound)
    return float(np.max(r)) if r.size else 0.0
