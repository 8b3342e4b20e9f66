"""The per-sample bounds of tests/imgform_util.py on the CPU: numpy emulations of the float32 arithmetic of k_hilbert_env,
k_hilbert_env_even, k_env_max + k_log_compress and k_apply_pulse, in their summation order, stay within them at the sizes the GPU
tests use (so the bounds are not too tight), and numpy mutants that model kernel bugs are flagged at nearly every sample they touch
(so they are not too loose).  No GPU: the mutants are never built as kernels."""
import numpy as np
import pytest

import imgform_util as iu
from oracle import beamform as obf

FLAG_MIN = 0.97
# At N = 637 / 638 the bound is ~640 u S_n: two of the mutants move a sample by less than that wherever the input sample they
# scale, or the share y / env of the imaginary part, is small -- up to a quarter of the samples -- and the linear kernel misses
# 3 % at N = 637.  At N = 61 / 62 every mutant is flagged at >= 98 % of the samples it touches.
FLAG_MIN_LONG = {"partial_quad_zero": 0.75, "one_tap_1e-3": 0.7, "linear_kernel": 0.95}


def columns(N, rng, n_random=1):
    """random columns, a spike column (half of its outputs are exactly 0 for even N) and a column with a quiet tail (the last
    third 1e-4 of the rest)"""
    cols = [rng.normal(size=N) for _ in range(n_random)]
    spike = np.zeros(N)
    spike[N // 3] = 3.0
    cols.append(spike)
    tail = rng.normal(size=N)
    tail[2 * N // 3:] *= 1e-4
    cols.append(tail)
    return np.stack(cols).astype(np.float32)


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 637, 638, 1023, 1024, 1025, 2047, 2048, 4093, 4096])
def test_envelope_emulation_is_within_the_bound(N):
    rf = columns(N, np.random.default_rng(N))
    bound, ref = iu.EnvBound(N)(rf)
    got = iu.emulate_env(rf)
    r = iu.worst_ratio(got, ref, bound)
    print(f"N={N}: k_hilbert_env emulation at {r:.3f} of the bound")
    assert r <= 1.0
    if N % 2 == 0:      # k_hilbert_env_even's two parity sums: the same chains without the zero taps, the same bits
        assert np.array_equal(iu.emulate_env(rf, parity_sums=True).view(np.uint32), got.view(np.uint32))
        same = ((np.arange(N) - N // 3) % 2 == 0) & (np.arange(N) != N // 3)
        assert np.all(got[1, same] == 0.0)                  # the spike: exact zeros at the other samples of its parity


def test_a_non_finite_sample_where_the_restatement_is_finite_fails_the_bound():
    """a kernel that writes NaN (or inf) into some samples of finite input must fail worst_ratio, not have them skipped: one whole
    column NaN, the last partial quad of another NaN, one sample inf"""
    rf = np.random.default_rng(2).normal(size=(1040, 638)).astype(np.float32)
    bound, ref = iu.EnvBound(638)(rf)
    good = ref.astype(np.float32)
    assert iu.worst_ratio(good, ref, bound) <= 1.0
    for cols, samples, v in ((5, slice(None), np.nan), (9, slice(636, 638), np.nan), (11, slice(100, 101), np.inf)):
        bad = good.copy()
        bad[cols, samples] = v
        assert iu.worst_ratio(bad, ref, bound) == np.inf
        assert np.all(iu.excess(bad, ref, bound)[cols, samples] == np.inf)


def test_envelope_bound_is_tight_enough_to_see_one_ulp_per_term():
    """a sample's bound is a few hundred ulp of its S_n at N = 638, and a single-ulp error of the whole envelope is inside it"""
    rf = columns(638, np.random.default_rng(1), n_random=3)
    bound, ref = iu.EnvBound(638)(rf)
    assert iu.worst_ratio(ref.astype(np.float32) * np.float32(1 + 2 ** -23), ref, bound) <= 1.0
    assert np.median(bound / np.maximum(ref, 1e-30)) < 1e-4


def _env_mutants(x, N):
    """f64 models of kernel bugs on columns x [C, N] -> {name: envelope}"""
    x = x.astype(np.float64)
    h = iu.hilbert_taps(N)
    n = np.arange(N)

    def env(xr, y):
        return np.sqrt(xr * xr + y * y)

    def conv(taps_of_k, xr=x):
        k = n[:, None] - n[None, :]                        # [output, input]
        return xr @ taps_of_k(k).T

    def table(hh):                                         # the kernel's tap table g[C + k] of a length len(hh)
        L = len(hh)
        return lambda k: np.where(np.abs(k) < L, np.sign(k) * hh[np.minimum(np.abs(k), L - 1)], 0.0)

    m = {}
    kinf = lambda k: np.where(k % 2 != 0, 2.0 / (np.pi * np.where(k == 0, 1, k)), 0.0)
    m["linear_kernel"] = env(x, conv(kinf))
    xq = x.copy()
    xq[:, N & ~3:] = 0.0
    m["partial_quad_zero"] = env(xq, conv(table(h), xq))
    m["taps_N_plus_1"] = env(x, conv(table(iu.hilbert_taps(N + 1))))
    m["taps_N_minus_1"] = env(x, conv(table(iu.hilbert_taps(N - 1))))
    y = conv(table(h))
    if N % 2 == 0:
        ysh = conv(lambda k: table(h)(k + 2))
        m["parity_offset"] = env(x, np.where(n % 2 == 0, ysh, y))
    m["no_real_part"] = np.abs(y)
    yt = y.copy()
    yt[:, 1:] += 1e-3 * h[1] * x[:, :-1]
    m["one_tap_1e-3"] = env(x, yt)
    return m


@pytest.fixture(scope="module")
def env_cases():
    out = {}
    for N in (61, 62, 637, 638):     # (N % 4 = 1, 2: a partial last quad of one and of two samples)
        rng = np.random.default_rng(N + 7)
        rf = (rng.uniform(0.5, 1.0, size=(8, N)) * rng.choice([-1, 1], size=(8, N))).astype(np.float32)
        bound, ref = iu.EnvBound(N)(rf)
        out[N] = (rf, bound, ref, _env_mutants(rf, N))
    return out


ENV_MUTANTS = ["linear_kernel", "partial_quad_zero", "taps_N_plus_1", "taps_N_minus_1", "no_real_part", "one_tap_1e-3"]


@pytest.mark.parametrize("N,name", [(N, m) for N in (61, 62, 637, 638) for m in ENV_MUTANTS] + [(62, "parity_offset"),
                                                                                                (638, "parity_offset")])
def test_the_envelope_bound_flags_kernel_bug_mutants(env_cases, N, name):
    """(the parity offset is a bug of the even kernel only: odd N never runs it)"""
    rf, bound, ref, muts = env_cases[N]
    mut = muts[name]
    noise = iu.EPS_FFT * np.abs(rf.astype(np.float64)).sum(axis=1, keepdims=True)
    touched = np.abs(mut - ref) > noise
    assert touched.sum() >= 100
    flagged = (iu.excess(mut, ref, bound) > 1.0) & touched
    frac = flagged.sum() / touched.sum()
    print(f"envelope N={N} {name}: {frac:.4f} of {int(touched.sum())} samples flagged")
    need = FLAG_MIN_LONG.get(name, FLAG_MIN) if N > 100 else FLAG_MIN
    assert frac >= need, f"{name}: only {frac:.4f} of the {int(touched.sum())} samples it touches are flagged"
    assert iu.worst_ratio(iu.emulate_env(rf), ref, bound) <= 1.0


@pytest.mark.parametrize("n,dr", [(1, 60.0), (257, 1.0), (5000, 40.0), (70001, 60.0), (262145, 300.0)])
def test_log_compress_emulation_is_within_the_bound(n, dr):
    rng = np.random.default_rng(n)
    env = (np.abs(rng.normal(size=n)) ** 4 * 10.0 ** rng.uniform(-6, 0, size=n)).astype(np.float32)
    env[n // 2] = 0.0
    bound, ref = iu.log_bound(env, dr)
    got = iu.emulate_log(env, dr)
    r = iu.worst_ratio(got, ref, bound)
    print(f"log n={n} dr={dr}: emulation at {r:.3f} of the bound")
    assert r <= 1.0
    z = np.zeros(max(n, 1), np.float32)
    bz, rz = iu.log_bound(z, dr)
    assert np.all(rz == 1.0) and iu.worst_ratio(iu.emulate_log(z, dr), rz, bz) <= 1.0


def test_the_log_bound_flags_a_maximum_of_the_first_block_only():
    rng = np.random.default_rng(4)
    env = (np.abs(rng.normal(size=20000)) ** 2).astype(np.float32)
    env[15000] = 40.0                                         # the maximum outside the first block's 1024 values
    for dr in (1.0, 40.0, 60.0, 300.0):
        bound, ref = iu.log_bound(env, dr)
        e = env.astype(np.float64)
        db = 20 * np.log10(e + 1e-12)
        mx = 20 * np.log10(e[:1024].max() + 1e-12)
        mut = (np.clip(db, mx - dr, mx) - (mx - dr)) / dr
        touched = mut != ref
        frac = ((iu.excess(mut, ref, bound) > 1.0) & touched).sum() / touched.sum()
        print(f"log dr={dr} max_of_first_block: {frac:.4f} of {int(touched.sum())} pixels flagged")
        assert touched.sum() >= 20 and frac >= FLAG_MIN


PULSES = [(50e6, 3e6, 1.5 / 50e6), (50e6, 5e6, 31.5 / (2.5 * 50e6)), (50e6, 22.5e6, 255.5 / (2.5 * 50e6)),
          (50e6, 22.5e6, 1023.5 / (2.5 * 50e6)), (20e6, 1e6, 1023.9 / (2.5 * 20e6))]


@pytest.mark.parametrize("fs,fc,sigma", PULSES)
def test_pulse_emulation_is_within_the_bound(fs, fc, sigma):
    K = obf.pulse_taps(fs, fc, sigma)[1]
    assert K <= 1024
    rng = np.random.default_rng(K)
    T = 2600
    x = np.zeros((3, T), np.float32)
    x[0] = rng.normal(size=T)
    idx = rng.integers(0, T, size=40)
    x[1, idx] = rng.uniform(0.5, 1.0, size=40) * rng.choice([-1, 1], size=40)
    x[2, [0, 255, 256, T - 1]] = 1.0                          # at the ends and a block edge
    ref = obf.apply_pulse(x, fs, fc, sigma)
    bound = iu.pulse_bound(x, fs, fc, sigma)
    got = iu.emulate_pulse(x, fs, fc, sigma)
    r = iu.worst_ratio(got, ref, bound)
    print(f"pulse K={K} fc/fs={fc / fs:.2f}: emulation at {r:.3f} of the bound")
    assert r <= 1.0


@pytest.mark.parametrize("K_target,fc_frac", [(32, 0.06), (1024, 0.45)])
def test_the_pulse_tap_term_covers_the_phase_error_without_hiding_it(K_target, fc_frac):
    """the float32 phase error of the taps, emulated with the exact sine of the float32 phase, against its own term: inside it, and
    not by a loose constant (at K ~ 1000 near Nyquist it is a sizeable part of it)"""
    fs = 50e6
    sigma = (K_target - 0.5) / (2.5 * fs)
    h, K, err = iu.pulse_tap_error(fs, fc_frac * fs, sigma)
    assert K == K_target
    g = iu.emulate_pulse_taps(fs, fc_frac * fs, sigma)[0].astype(np.float64)
    d = np.abs(g - h)
    r = iu.excess(g, h, err)
    print(f"pulse taps K={K}: error {d.max() / np.abs(h).max():.2e} of the peak tap, at most {r.max():.3f} of its term")
    assert r.max() <= 1.0
    if K >= 1000:
        assert r.max() >= 0.05 and d.max() / np.abs(h).max() > 1e-5


def test_the_pulse_bound_flags_kernel_bug_mutants():
    fs, fc = 50e6, 2.8125e6
    sigma = 39.5 / (2.5 * fs)
    h, K = obf.pulse_taps(fs, fc, sigma)
    assert K == 40 and abs(np.sin(2 * np.pi * fc * K / fs)) > 0.99
    rng = np.random.default_rng(8)
    T = 3000
    x = np.zeros((4, T), np.float32)
    for r in range(4):
        idx = rng.choice(T, size=30, replace=False)
        x[r, idx] = rng.uniform(0.5, 1.0, size=30) * rng.choice([-1, 1], size=30)
    x[0, [256 - 5, 512 + 3, 768]] = 1.0                       # near block edges
    ref = obf.apply_pulse(x, fs, fc, sigma)
    bound = iu.pulse_bound(x, fs, fc, sigma)
    x64 = x.astype(np.float64)
    hk = h.copy()
    hk[[0, -1]] = 0.0
    muts = {"taps_K_minus_1": np.stack([np.convolve(r, hk)[K:K + T] for r in x64])}
    halo = np.zeros_like(ref)
    for b0 in range(0, T, 256):
        blk = np.zeros_like(x64)
        blk[:, b0:b0 + 256] = x64[:, b0:b0 + 256]
        halo[:, b0:b0 + 256] = np.stack([np.convolve(r, h)[K:K + T] for r in blk])[:, b0:b0 + 256]
    muts["halo_dropped"] = halo
    for name, mut in muts.items():
        touched = mut != ref
        frac = ((iu.excess(mut, ref, bound) > 1.0) & touched).sum() / touched.sum()
        print(f"pulse {name}: {frac:.4f} of {int(touched.sum())} samples flagged")
        assert touched.sum() >= 50 and frac >= FLAG_MIN, name
