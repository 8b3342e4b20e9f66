"""Device time of the two Doppler steps (DESIGN D24): pbrt_doppler_autocorr_dev at N = 8, 16, 64 frames without a wall filter, under
mean removal and under degree 3, and pbrt_doppler_maps_dev under 1 x 1, 3 x 3, 5 x 5 and 15 x 15 Hamming windows -- on the lambda / 2
grid of examples/us_bmode.py --iq (+-20 mm x 20 - 80 mm at 5 MHz: 261 x 391) and on 1040 x 638, the lambda / 4 grid of the reference's
us_render.  The steps have no event slot in pbrt_image_stats (ABI 5 stays as it is): wall clock over a queue of 50 launches, as
tools/bench_iq.py times rf2iq, so a launch's share of queueing is in the figure.  Beside each time the bytes the step must move (8 N per
pixel in and 12 out; then 12 in and 8 out) and the rate that makes, to set beside the copy rate of the device."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pbrt_amd as mi

cx = mi.default_context()
rng = np.random.default_rng(0)


def wall(call, n=50):
    call()
    cx.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    cx.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


lam = 1540.0 / 5e6
GRIDS = (("us_bmode --iq, lambda/2", len(np.arange(-0.02, 0.02 + lam / 2, lam / 2)), len(np.arange(0.02, 0.08 + lam / 2, lam / 2))),
         ("us_render, lambda/4", 1040, 638))
for name, nx, nz in GRIDS:
    P = nx * nz
    d_acf, d_vel, d_amp = mi.DeviceBuffer(cx, (3, nx, nz)), mi.DeviceBuffer(cx, (nx, nz)), mi.DeviceBuffer(cx, (nx, nz))
    for N in (8, 16, 64):
        frame = (rng.normal(size=(nx, nz)) + 1j * rng.normal(size=(nx, nz))).astype(np.complex64)
        d_frames = mi.DeviceBuffer(cx, (N, nx, nz), np.complex64)
        for n in range(N):   # (one frame on the host at a time: a moving tone)
            d_frames.view(n * P, (nx, nz)).upload(frame * np.complex64(np.exp(0.3j * n)))
        for wf, degree in (("none", 0), ("mean", 0), ("poly", 3)):
            t = wall(lambda: mi.doppler_autocorr(d_frames, wf, degree, out=d_acf))
            moved = P * (8 * N + 12)
            print(f"{name} {nx} x {nz}, N = {N:2d}, wall {wf}{degree if wf == 'poly' else ''}: autocorr {t:7.1f} us, "
                  f"{moved / 1e6:7.1f} MB must move = {moved / t / 1e6:5.2f} TB/s", flush=True)
        d_frames.close()
    for kernel in ((1, 1), (3, 3), (5, 5), (15, 15)):
        t = wall(lambda: mi.doppler_maps(d_acf, 0.3, "hamming", kernel, out=(d_vel, d_amp)))
        print(f"{name} {nx} x {nz}, hamming {kernel[0]} x {kernel[1]}: maps {t:7.1f} us, {P * 20 / 1e6:6.1f} MB must move = {P * 20 / t / 1e6:5.2f} TB/s",
              flush=True)
