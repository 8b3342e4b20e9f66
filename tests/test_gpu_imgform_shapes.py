"""k_hilbert_env / k_hilbert_env_even, k_env_max + k_log_compress and k_apply_pulse (csrc/kernels_beamform.h) held to the
per-sample bounds of tests/imgform_util.py against the f64 restatement of oracle/beamform.py, at the shapes where the kernels
change path: every column length mod 4 and mod 8 around 256, 638, 1024, 2048 and 4096, one to 20 000 columns per call; images
around k_env_max's grid stride and up to 4e6 pixels, at an unaligned pointer; pulse half-widths up to PULSE_MAX_K and traces around
the 256-sample blocks.  Then non-finite input (a column with a NaN or an infinity is NaN, a NaN anywhere makes the display NaN, as
in the restatement and USMain.py:213-218, end to end on the D12 scene) and the context's envelope tap table across column lengths,
pbrt_ctx_trim and a replayed us_render."""
import numpy as np
import pytest

import imgform_util as iu
from conftest import scene_path
from oracle import beamform as obf

pytestmark = pytest.mark.gpu

ENV_N = [1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 637, 638, 1023, 1024, 1025, 2047, 2048, 2049, 4093, 4094, 4095, 4096]
WORST = {}      # kernel -> largest error-to-bound ratio seen in this module


def _note(kernel, r):
    WORST[kernel] = max(WORST.get(kernel, 0.0), r)
    print(f"worst error / bound so far: {kernel} {WORST[kernel]:.4f}")


def _columns(N, nx, rng):
    """random columns, spike columns and quiet-tail columns (the last third 1e-4 of the rest) in turn"""
    rf = rng.normal(size=(nx, N))
    rf[1::3] = 0.0
    for i in range(1, nx, 3):
        rf[i, (7 * i) % N] = 3.0
    rf[2::3, 2 * N // 3:] *= 1e-4
    return rf.astype(np.float32)


def _envelope_both(mi, rf, monkeypatch, even):
    """-> the envelope by the default kernel; with even N also by k_hilbert_env (PBRT_ENV_GENERAL=1), which must give the same bits"""
    got = mi.envelope(rf)
    if even:
        monkeypatch.setenv("PBRT_ENV_GENERAL", "1")
        gen = mi.envelope(rf)
        monkeypatch.delenv("PBRT_ENV_GENERAL")
        assert np.array_equal(gen.view(np.uint32), got.view(np.uint32))
    return got


@pytest.mark.parametrize("N", ENV_N)
def test_envelope_is_within_its_per_sample_bound(mi, monkeypatch, N):
    cx = mi.default_context()
    rng = np.random.default_rng(1000 + N)
    eb = iu.EnvBound(N)
    for nx in (1, 2, 1040):
        rf = _columns(N, nx, rng)
        got = _envelope_both(mi, rf, monkeypatch, N % 2 == 0)
        bound, ref = eb(rf)
        r = iu.worst_ratio(got, ref, bound)
        _note("k_hilbert_env(_even)", r)
        assert got.shape == rf.shape and r <= 1.0, (N, nx, r)
        d = mi.DeviceBuffer.from_host(cx, rf)
        assert np.array_equal(mi.envelope(d).numpy().view(np.uint32), got.view(np.uint32))
        d.close()


@pytest.mark.parametrize("N", [8, 9])
def test_envelope_of_twenty_thousand_short_columns(mi, monkeypatch, N):
    rf = _columns(N, 20000, np.random.default_rng(N))
    got = _envelope_both(mi, rf, monkeypatch, N % 2 == 0)
    bound, ref = iu.EnvBound(N)(rf)
    r = iu.worst_ratio(got, ref, bound)
    _note("k_hilbert_env(_even)", r)
    assert r <= 1.0


LOG_N = [1, 255, 256, 257, 1024, 1025, 262143, 262144, 262145, 663520, 4000003]


def _log_dev(mi, cx, vals, n, off, dr):
    buf = mi.DeviceBuffer.from_host(cx, vals)
    out = mi.DeviceBuffer(cx, (n,))
    cx.check(cx.lib.pbrt_log_compress_dev(cx.handle, n, buf.ptr + 4 * off, float(dr), out.ptr), "pbrt_log_compress_dev")
    got = out.numpy()
    buf.close()
    out.close()
    return got


def _max_places(n):
    """where the maximum goes: first, last, in the scalar tail of the 16-byte loop, beyond k_env_max's first grid stride"""
    nb = max(1, min(-(-n // 1024), 256))
    places = {"first": 0, "last": n - 1, "tail": (n // 4) * 4 if n % 4 else n - 1}
    if 4 * nb * 256 < n:
        places["past_stride"] = min(4 * nb * 256 + 5, n - 1)
    return places


@pytest.mark.parametrize("n", LOG_N)
def test_log_compress_is_within_its_per_pixel_bound(mi, n):
    cx = mi.default_context()
    rng = np.random.default_rng(n)
    base = (np.abs(rng.normal(size=n + 1)) ** 3).astype(np.float32)
    drs = (1.0, 40.0, 60.0, 300.0)
    for (where, at), dr in ((p, dr) for p in _max_places(n).items() for dr in drs):
        vals = base.copy()
        vals[at] = 50.0
        got = mi.log_compress(vals[:n], dr)
        bound, ref = iu.log_bound(vals[:n], dr)
        r = iu.worst_ratio(got, ref, bound)
        _note("k_env_max + k_log_compress", r)
        assert r <= 1.0, (n, where, dr, r)
        if dr == 300.0:                                     # (e + 1e-12 >= 1e-12: 274 dB at most, nothing clips)
            assert 0.0 < got.min() and ref.min() > 0.0
        for off in ((0, 1) if n >= 262144 else (0,)):       # (off = 1: the pointer 4 bytes past a 16-byte boundary)
            v = vals if off == 0 else np.concatenate([[0.0], vals[:n]]).astype(np.float32)
            d = _log_dev(mi, cx, v, n, off, dr)
            assert np.array_equal(d.view(np.uint32), got.view(np.uint32)), (n, where, off)
    for dr in drs:                                          # an all-zero envelope: all ones, as in the restatement
        z = np.zeros(n, np.float32)
        got = mi.log_compress(z, dr)
        bound, ref = iu.log_bound(z, dr)
        assert np.all(ref == 1.0) and iu.worst_ratio(got, ref, bound) <= 1.0


PULSE_T = [255, 256, 257, 511, 513, 10000]
PULSE_K = [1, 2, 255, 256, 257, 1023, 1024]


def _sigma_for(K, fs):
    sigma = (K - 0.5) / (2.5 * fs)
    assert obf.pulse_taps(fs, 1e6, sigma)[1] == K
    return sigma


@pytest.mark.parametrize("K", PULSE_K)
def test_pulse_is_within_its_per_sample_bound(mi, K):
    fs = 50e6
    sigma = _sigma_for(K, fs)
    fc = (0.45 if K >= 1000 else (0.05, 0.2, 0.45)[K % 3]) * fs    # (K ~ 1000 near Nyquist: the largest f32 tap-phase error)
    rng = np.random.default_rng(K)
    for T in PULSE_T:
        x = np.zeros((3, T), np.float32)
        x[0] = rng.normal(size=T)
        spikes = [p for b0 in range(0, T, 256) for p in (b0 - K, b0 + K, b0 + 255 - K, b0 + 255 + K, b0) if 0 <= p < T]
        x[1, spikes] = rng.uniform(0.5, 1.0, size=len(spikes)) * rng.choice([-1, 1], size=len(spikes))
        x[2, :T // 3] = rng.normal(size=T // 3)            # a trace that falls silent: the error of its tail is its own
        got = mi.apply_pulse(x, fs, fc, sigma)
        ref = obf.apply_pulse(x, fs, fc, sigma)
        bound = iu.pulse_bound(x, fs, fc, sigma)
        r = iu.worst_ratio(got, ref, bound)
        _note("k_apply_pulse", r)
        assert got.shape == x.shape and r <= 1.0, (K, T, r)
        assert np.all(got[2, T // 3 + K:] == 0.0)


def test_pulse_half_width_and_trace_count_limits(mi):
    fs = 50e6
    x = np.ones((2, 300), np.float32)
    mi.apply_pulse(x, fs, 5e6, _sigma_for(1024, fs))
    sigma_1025 = 1024.5 / (2.5 * fs)
    assert obf.pulse_taps(fs, 5e6, sigma_1025)[1] == 1025
    with pytest.raises(RuntimeError):
        mi.apply_pulse(x, fs, 5e6, sigma_1025)              # K = 1025 > PULSE_MAX_K
    sigma = _sigma_for(2, fs)
    T = 3
    x = np.random.default_rng(3).normal(size=(65535, T)).astype(np.float32)
    got = mi.apply_pulse(x, fs, 7e6, sigma)                # 65 535 traces: the largest grid.y
    h, K = obf.pulse_taps(fs, 7e6, sigma)
    _, _, err = iu.pulse_tap_error(fs, 7e6, sigma)
    n = np.arange(T)
    k = n[:, None] - n[None, :]                             # out[n] = sum_m x[m] h[n - m]
    inside = np.abs(k) <= K
    M, Ma, Me = (np.where(inside, v[np.clip(k + K, 0, 2 * K)], 0.0) for v in (h, np.abs(h), err))
    x64 = x.astype(np.float64)
    ref = x64 @ M.T
    bound = (2 * K + 1 + iu.C_SUM_PULSE) * iu.U32 * (np.abs(x64) @ Ma.T) + np.abs(x64) @ Me.T
    r = iu.worst_ratio(got, ref, bound)
    _note("k_apply_pulse", r)
    assert r <= 1.0
    with pytest.raises(RuntimeError):
        mi.apply_pulse(np.zeros((65536, T), np.float32), fs, 7e6, sigma)


# ---- non-finite input -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [9, 637, 638, 4096])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_sample_makes_its_column_nan_in_both_kernels(mi, monkeypatch, N, bad):
    rng = np.random.default_rng(N)
    clean = rng.normal(size=(5, N)).astype(np.float32)
    for at in sorted({0, N // 2, N - 1}):
        rf = clean.copy()
        rf[2, at] = bad
        assert np.isnan(obf.envelope(rf)[2]).all() and not np.isnan(obf.envelope(rf)[[0, 1, 3, 4]]).any()
        envs = {"default": None}
        if N % 2 == 0:
            envs["general"] = "1"
        for name, flag in envs.items():
            if flag:
                monkeypatch.setenv("PBRT_ENV_GENERAL", flag)
            ref = mi.envelope(clean)
            got = mi.envelope(rf)
            if flag:
                monkeypatch.delenv("PBRT_ENV_GENERAL")
            assert np.isnan(got[2]).all(), (N, at, name)
            keep = [0, 1, 3, 4]
            assert np.array_equal(got[keep].view(np.uint32), ref[keep].view(np.uint32)), (N, at, name)


@pytest.mark.parametrize("n", [1, 1000, 262145, 663520])
@pytest.mark.parametrize("bad", [np.nan, -1e-10, -np.inf, np.inf])
def test_a_nan_or_negative_envelope_makes_the_display_nan(mi, n, bad):
    cx = mi.default_context()
    base = (np.abs(np.random.default_rng(n).normal(size=n + 1)) ** 2).astype(np.float32)
    for where, at in _max_places(n).items():
        vals = base.copy()
        vals[at] = bad
        assert np.isnan(obf.log_compress(vals[:n], 60.0)).all()            # np.max propagates NaN (USMain.py:213-216)
        got = mi.log_compress(vals[:n], 60.0)
        assert np.isnan(got).all(), (n, where, bad)
        if n >= 262144:
            v = np.concatenate([[0.0], vals[:n]]).astype(np.float32)
            assert np.isnan(_log_dev(mi, cx, v, n, 1, 60.0)).all(), (n, where, bad)
    small = base[:n].copy()
    small[0] = -1e-13                                       # inside (-1e-12, 0): log10 of a positive number on both sides
    assert np.isfinite(mi.log_compress(small, 60.0)).all()


def test_d12_nan_echoes_reach_the_display_as_in_the_f64_chain(mi):
    """the 0-degree plane wave on a plate facing the probe exactly gives NaN echoes (quirks = None, the reference's
    arithmetic).  us_render's envelope is NaN in exactly the columns where the f64 chain (DAS -> envelope of oracle/beamform.py on
    the GPU's own channel buffer) is NaN, and the display is all NaN, as np.max makes it in USMain.py:213-218."""
    T = mi.ScalarTransform4f
    sc = mi.load_dict({
        "type": "scene",
        "integrator": {"type": "ultrasound_integrator", "max_depth": 4, "sampling_rate": 40e6, "frequency": 4e6, "sound_speed": 1500,
                       "attenuation": 0.1, "main_beam_angle": 20, "cutoff_angle": 35, "n_elements": 32, "pitch": 2e-4,
                       "time_samples": 4000, "angles": [-5.0, 0.0, 5.0], "paths_per_ray": 50, "seed": 9},
        "sensor": {"type": "ultrasound_sensor", "to_world": T().look_at([0, 0, 0], [0, 0, 0.03], [0, 1, 0])},
        "p": {"type": "rectangle", "to_world": T().translate([0, 0, 0.015]) @ T().rotate([1, 0, 0], 180) @ T().scale([0.03, 0.03, 1]),
              "bsdf": {"type": "ultrasound_bsdf", "impedance": 7.8, "roughness": 0.9}}})
    ui = sc.integrator()
    display, bmode, (xs, zs) = mi.us_render(sc, x_range=(-0.003, 0.003), z_range=(0.005, 0.03))
    chan = np.asarray(ui.channel_buf, np.float32).reshape(3, 32, 4000)
    assert np.isnan(chan[1]).any() and not np.isnan(chan[[0, 2]]).any()
    ex = mi.build_probe("linear", 32, ui.pitch, ui.frequency, 70).geometry[0]
    tx = np.asarray(ui.transmission_delays_buf, np.float32).reshape(3, 32)
    env_ref = obf.envelope(obf.das_beamform(chan, tx, ex, xs, zs, ui.fs, ui.sound_speed))
    nan_cols = np.isnan(env_ref).any(axis=1)
    assert nan_cols.any() and np.array_equal(np.isnan(env_ref).all(axis=1), nan_cols)
    assert np.array_equal(np.isnan(bmode).any(axis=1), nan_cols) and np.array_equal(np.isnan(bmode).all(axis=1), nan_cols)
    assert np.isnan(obf.log_compress(env_ref, 60.0)).all() and np.isnan(display).all()


# ---- the context's tap table ------------------------------------------------------------------------------------------------
def _env_on(mi, cx, rf):
    d = mi.DeviceBuffer.from_host(cx, rf)
    out = mi.envelope(d).numpy()
    d.close()
    return out


def test_the_tap_table_follows_the_column_length(mi, capi):
    """envelopes of lengths 638, 637, 638, 4096, 8 in turn on one context equal a fresh context's, bit for bit; then the same with
    pbrt_ctx_trim between the calls (a log compression first, so that the trim takes the tap table)"""
    lengths = [638, 637, 638, 4096, 8]
    rfs = {N: _columns(N, 6, np.random.default_rng(N)) for N in set(lengths)}
    fresh = {}
    for N in rfs:
        cf = capi.Context(0)
        fresh[N] = _env_on(mi, cf, rfs[N])
        cf.close()
    cx = capi.Context(0)
    for trim in (False, True):
        for N in lengths:
            got = _env_on(mi, cx, rfs[N])
            assert np.array_equal(got.view(np.uint32), fresh[N].view(np.uint32)), (N, trim)
            if trim:
                d = mi.DeviceBuffer.from_host(cx, np.ones(64, np.float32))
                mi.log_compress(d, 60.0).numpy()
                d.close()
                cx.trim()
    cx.close()


def test_a_replayed_us_render_after_an_envelope_of_another_length(mi):
    """us_render replays its recording from the third call on; an envelope of another column length on the same context replaces
    the tap table, and the next us_render must not replay the stale recording: its image equals graph=False's at the tolerance
    of test_us_render_replays_its_chain_from_the_third_call_on"""
    sc = mi.load_file(scene_path("us_plate.xml"), paths_per_ray=16, seed=5)
    kw = dict(x_range=(-0.012, 0.012), z_range=(0.03, 0.07), return_bmode=True)
    flags = []
    for _ in range(3):
        tm = {}
        b = mi.us_render(sc, timing=tm, **kw)[1]
        flags.append(tm["replayed"])
    assert flags == [False, False, True]
    cx = sc.device().ctx
    other = b.shape[1] + 1
    _env_on(mi, cx, np.random.default_rng(0).normal(size=(3, other)).astype(np.float32))
    after = mi.us_render(sc, **kw)[1]
    plain = mi.us_render(sc, graph=False, **kw)[1]
    assert np.allclose(after, plain, rtol=0, atol=2e-5 * plain.max())
    assert np.allclose(b, plain, rtol=0, atol=2e-5 * plain.max())
