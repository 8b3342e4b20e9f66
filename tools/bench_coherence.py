"""Device time of the spatial-coherence beamformers (DESIGN D26) at the scan of profiles/capon.md section 1: linear probe, 5 angles, 64
elements at 120 um, I/Q data 5 x 64 x 2500 at 12.5 MHz (complex normal noise) demodulated at 5 MHz, 261 x 391 pixels at lambda / 2
(x +-20 mm, z 20 - 80 mm), the first-arrival table made once.  Per call: three warm-up calls, then 7 repetitions of synchronise, queue n
calls, synchronise, wall clock / n; median (smallest - largest) in us.  Beside SLSC at (lag_prop, half_kernel) = (0.3, 1) and (1.0, 4) and
CF at gamma 1: pbrt_iq_beamform_table_dev and pbrt_capon_beamform_table_dev at l_prop 0 -- the same gather with nothing behind it.
    python tools/bench_coherence.py [--f-number F]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pbrt_amd as mi

ap = argparse.ArgumentParser()
ap.add_argument("--f-number", type=float, default=1.0)
args = ap.parse_args()
rng = np.random.default_rng(0)
A, E, T, c, fs, pitch, fc = 5, 64, 2500, 1540.0, 12.5e6, 1.2e-4, 5e6
iq = (rng.normal(size=(A, E, T)) + 1j * rng.normal(size=(A, E, T))).astype(np.complex64)
ex = (pitch * (np.arange(E, dtype=np.float32) - (E - 1) / 2)).astype(np.float32)
tx = (ex[None, :].astype(np.float64) * np.sin(np.deg2rad([-15, -7.5, 0, 7.5, 15]))[:, None] / c).astype(np.float32)
lam = c / fc
x, z = np.arange(-0.02, 0.02 + lam / 2, lam / 2), np.arange(0.02, 0.08 + lam / 2, lam / 2)
cx = mi.default_context()
d_iq = mi.DeviceBuffer.from_host(cx, iq)
d_tx, d_ex, d_x, d_z = (mi.DeviceBuffer.from_host(cx, np.asarray(v, np.float32)) for v in (tx, ex, x, z))
table = mi.das_first_arrival(d_tx, d_ex, d_x, d_z, c)
out_c = mi.DeviceBuffer(cx, (len(x), len(z)), np.complex64)
out_r = mi.DeviceBuffer(cx, (len(x), len(z)), np.float32)
common = dict(f_number=args.f_number, table=table)
pos = (d_iq, d_tx, d_ex, d_x, d_z, fs, c, fc)


def timed(call, n):
    for _ in range(3):
        call()
    cx.synchronize()
    reps = []
    for _ in range(7):
        cx.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            call()
        cx.synchronize()
        reps.append((time.perf_counter() - t0) / n * 1e6)
    return np.median(reps), min(reps), max(reps)


print(f"{len(x)} x {len(z)} pixels, {A} x {E} x {T} I/Q samples, f-number {args.f_number:g}", flush=True)
rows = (("pbrt_iq_beamform_table_dev", 50, lambda: mi.iq_beamform(*pos, out=out_c, **common)),
        ("pbrt_capon_beamform_table_dev l_prop 0", 10, lambda: mi.capon_beamform(*pos, l_prop=0.0, delta_l=0.01, out=out_c, **common)),
        ("pbrt_coherence_beamform_table_dev CF gamma 1", 10, lambda: mi.coherence_beamform(*pos, kind="cf", gamma=1.0, out=out_c, **common)),
        ("... SLSC lag_prop 0.3 half_kernel 0", 10,
         lambda: mi.coherence_beamform(*pos, kind="slsc", lag_prop=0.3, half_kernel=0, out=out_r, **common)),
        ("... SLSC lag_prop 0.3 half_kernel 1", 10,
         lambda: mi.coherence_beamform(*pos, kind="slsc", lag_prop=0.3, half_kernel=1, out=out_r, **common)),
        ("... SLSC lag_prop 1.0 half_kernel 4", 5,
         lambda: mi.coherence_beamform(*pos, kind="slsc", lag_prop=1.0, half_kernel=4, out=out_r, **common)))
for name, n, call in rows:
    med, lo, hi = timed(call, n)
    print(f"{name:55s} {med:9.1f} ({lo:.1f} - {hi:.1f}) us", flush=True)
