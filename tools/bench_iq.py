"""Device time of the RF chain against the I/Q chain (DESIGN D20) at the acquisition of the reference's us_render (USMain.py:26-90:
5 x 64 x 10000 channel buffer, +-40 mm lateral): RF delay-and-sum + Hilbert envelope on the lambda / 4 grid; rf2iq + I/Q delay-and-sum +
modulus on the same grid at decimation 1 and 4; the I/Q chain on a lambda / 2 axial grid.  Beamformer and envelope by HIP events on the
library's stream (pbrt_ctx_set_profiling), N = 10, without and with the first-arrival table.  rf2iq has no event slot in
pbrt_image_stats (ABI 5 stays as it is): it is timed by wall clock over a queue of 50 launches, so the chain totals add two kinds of
time and say so.  A last block times rf2iq alone at D = 1, 2, 4, 8: its LDS reads are D words apart from lane to lane.
--apodization {boxcar,tukey,hann,hamming} [--alpha A]: the receive window of both beamformers (DESIGN D22; boxcar: today's kernels)."""
import os, sys, time
import argparse
_ap = argparse.ArgumentParser()
_ap.add_argument("--apodization", choices=("boxcar", "tukey", "hann", "hamming"), default="boxcar")   # the receive window (DESIGN D22)
_ap.add_argument("--alpha", type=float, default=0.5)
_a = _ap.parse_args()
WIN = dict(rx_apodization=_a.apodization, rx_apodization_alpha=_a.alpha) if _a.apodization != "boxcar" else {}
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pbrt_amd as mi
rng = np.random.default_rng(0)
A, E, T, c, fs, pitch, fc = 5, 64, 10000, 1540.0, 50e6, 1.2e-4, 5e6
data = rng.normal(size=(A, E, T)).astype(np.float32)
ex = (pitch * (np.arange(E, dtype=np.float32) - (E - 1) / 2)).astype(np.float32)
tx = (ex[None, :].astype(np.float64) * np.sin(np.deg2rad([-15, -7.5, 0, 7.5, 15]))[:, None] / c).astype(np.float32)
lam = c / fc
cx = mi.default_context()
up = lambda v: mi.DeviceBuffer.from_host(cx, np.asarray(v, np.float32))  # noqa: E731
d_data, d_tx, d_ex = up(data), up(tx), up(ex)
N = 10


def events(call):
    """(beamformer us, envelope us) of call(), mean of N by HIP events"""
    call()
    cx.synchronize()
    cx.set_profiling(True)
    das = env = 0.0
    for _ in range(N):
        call()
        st = cx.image_stats()
        das += st["das_ms"] / N
        env += st["envelope_ms"] / N
    cx.set_profiling(False)
    return das * 1e3, env * 1e3


def wall(call, n=50):
    call()
    cx.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    cx.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def grid(step_z):
    x, z = np.arange(-0.04, 0.04 + lam / 4, lam / 4), np.arange(0.001, 0.05 + step_z, step_z)
    d_x, d_z = up(x), up(z)
    return x, z, d_x, d_z, mi.das_first_arrival(d_tx, d_ex, d_x, d_z, c)


def rf_chain(step_z, name):
    x, z, d_x, d_z, tab = grid(step_z)
    bf, env = mi.DeviceBuffer(cx, (len(x), len(z))), mi.DeviceBuffer(cx, (len(x), len(z)))
    for label, t in (("", None), (", first-arrival table", tab)):
        das, e = events(lambda: (mi.das_beamform(d_data, d_tx, d_ex, d_x, d_z, fs, c, out=bf, table=t, **WIN), mi.envelope(bf, out=env)))
        print(f"RF  {name} {len(x)} x {len(z)}{label}: DAS {das:7.1f} us + Hilbert envelope {e:6.1f} us = {das + e:7.1f} us", flush=True)


def iq_chain(step_z, name, D):
    x, z, d_x, d_z, tab = grid(step_z)
    taps = up(mi.lowpass_taps(fc / 2, fs))
    iq = mi.rf2iq(d_data, fc, fs, decimation=D, taps=taps)
    t_demod = wall(lambda: mi.rf2iq(d_data, fc, fs, decimation=D, taps=taps, out=iq))
    bf, env = mi.DeviceBuffer(cx, (len(x), len(z)), np.complex64), mi.DeviceBuffer(cx, (len(x), len(z)))
    for label, t in (("", None), (", first-arrival table", tab)):
        das, e = events(lambda: (mi.iq_beamform(iq, d_tx, d_ex, d_x, d_z, fs / D, c, fc, out=bf, table=t, **WIN), mi.iq_envelope(bf, out=env)))
        print(f"I/Q {name} {len(x)} x {len(z)} D = {D}{label}: rf2iq (K = {taps.shape[0] // 2}, wall clock) {t_demod:6.1f} us + I/Q DAS {das:7.1f} us "
              f"+ modulus {e:5.1f} us = {t_demod + das + e:7.1f} us (events + wall clock)", flush=True)


print(f"receive window: {_a.apodization}" + (f" alpha = {_a.alpha:g}" if _a.apodization == "tukey" else ""), flush=True)
rf_chain(lam / 4, "lambda/4")
for D in (1, 4):
    iq_chain(lam / 4, "lambda/4", D)
for D in (1, 4):
    iq_chain(lam / 2, "lambda/2", D)

# the demodulator alone: (2K + 1) multiply-adds per output and plane, T / D outputs per trace -- without bank conflicts the time falls as 1 / D
taps = up(mi.lowpass_taps(fc / 2, fs))
for D in (1, 2, 4, 8):
    iq = mi.rf2iq(d_data, fc, fs, decimation=D, taps=taps)
    t = wall(lambda: mi.rf2iq(d_data, fc, fs, decimation=D, taps=taps, out=iq))
    print(f"rf2iq alone D = {D}: {t:6.1f} us (wall clock over 50 queued launches), {t * D:6.1f} us x D", flush=True)
