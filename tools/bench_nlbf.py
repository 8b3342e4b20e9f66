"""Device time of the beamformers at the acquisition of the reference's us_render (USMain.py:26-90: 5 x 64 x 10000 channel buffer,
+-40 mm lateral at lambda / 4) on the axial grid the non-linear beamformers need (lambda / 16: DESIGN D19): DAS, p-DAS (p = 2 and
p = 1.5) and F-DMAS, without and with the first-arrival table, HIP events on the library's stream (pbrt_ctx_set_profiling); the axial
FIR of F-DMAS's default band by wall clock over a queue of launches.
--apodization {boxcar,tukey,hann,hamming} [--alpha A]: the receive window of all four (DESIGN D22; boxcar: today's kernels)."""
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
x = np.arange(-0.04, 0.04 + lam / 4, lam / 4); z = np.arange(0.001, 0.05 + lam / 16, lam / 16)
cx = mi.default_context()
d = {k: mi.DeviceBuffer.from_host(cx, v.astype(np.float32)) for k, v in dict(data=data, tx=tx, ex=ex, x=x, z=z).items()}
out = mi.DeviceBuffer(cx, (len(x), len(z)))
tab = mi.das_first_arrival(d["tx"], d["ex"], d["x"], d["z"], c)
N = 10
def run(name, call):
    res = []
    for table in (None, tab):
        call(table)
        cx.synchronize()
        cx.set_profiling(True)
        ms = 0.0
        for _ in range(N):
            call(table)
            ms += cx.image_stats()["das_ms"] / N
        cx.set_profiling(False)
        res.append(ms * 1e3)
    print(f"{name:14s} {len(x)} x {len(z)}: {res[0]:8.1f} us, with the first-arrival table {res[1]:8.1f} us", flush=True)
args = (d["data"], d["tx"], d["ex"], d["x"], d["z"], fs, c)
print(f"receive window: {_a.apodization}" + (f" alpha = {_a.alpha:g}" if _a.apodization == "tukey" else ""), flush=True)
run("DAS", lambda t: mi.das_beamform(*args, out=out, table=t, **WIN))
run("p-DAS p=2", lambda t: mi.nonlinear_beamform(*args, method="pdas", p=2.0, out=out, table=t, **WIN))
run("p-DAS p=1.5", lambda t: mi.nonlinear_beamform(*args, method="pdas", p=1.5, out=out, table=t, **WIN))
run("F-DMAS", lambda t: mi.nonlinear_beamform(*args, method="fdmas", out=out, table=t, **WIN))
h = mi.bandpass_taps(2 * fc * 0.65, 2 * fc * 1.35, mi.beamform.axial_rate(z, c))
d_h, flt = mi.DeviceBuffer.from_host(cx, h), mi.DeviceBuffer(cx, out.shape)
mi.axial_fir(out, d_h, out=flt)
cx.synchronize()
t0 = time.perf_counter()
for _ in range(50):
    mi.axial_fir(out, d_h, out=flt)
cx.synchronize()
print(f"axial FIR K = {len(h) // 2}: {(time.perf_counter() - t0) / 50 * 1e6:.1f} us per image (wall clock over 50 queued launches)")
