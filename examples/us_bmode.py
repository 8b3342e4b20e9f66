#!/usr/bin/env python3
"""The reference's ultrasound driver flow on this library: scene dict -> acquisition -> delay-and-sum -> envelope ->
log compression -> finite-difference roughness loop (what USMain.py does at :26-90, :93-224, :257-289), without the
plotting.  Writes the B-mode image and the channel buffer as .npy.
    python examples/us_bmode.py [--convex] [--beamformer {das,pdas,fdmas,capon,slsc,cf}] [--p P] [--l-prop X] [--delta-l D]
                                  [--lag-prop Q] [--half-kernel H] [--gamma G]
                                  [--iq [--decimation D]] [--polar] [--apodization {boxcar,tukey,hann,hamming} [--alpha A]] [out_dir]
--convex: the same flow under a curved (abdominal) array -- 64 elements on a 40 mm arc of 40 degrees (DESIGN D18); the sensor
transform puts the apex where the linear array sits, and the scan is given in the sensor's frame, whose origin is the centre of
curvature.
--beamformer: delay-and-sum (default), p-DAS (--p, default 2) or F-DMAS (DESIGN D19).  The non-linear beamformers band-pass their
image along z, around the carrier (p-DAS) or twice the carrier (F-DMAS): the reference's lambda / 4 grid puts the axial Nyquist
frequency AT the carrier, so the example picks lambda / 8 for p-DAS and lambda / 16 for F-DMAS itself and says so.
--beamformer capon: the minimum-variance beamformer (DESIGN D23) with subarrays of --l-prop (default 0.5) of the elements a pixel uses
and a diagonal loading of --delta-l (default 0.01).  It works on I/Q data, so it implies --iq, and it makes its own weights: no
--apodization.
--beamformer slsc / cf: the spatial-coherence beamformers (DESIGN D26; not ultraspy's).  slsc is the short-lag spatial coherence -- the
image is the correlation between neighbouring elements, summed over the lags up to --lag-prop (default 0.3) of the elements a pixel uses,
over an axial kernel of 2 x --half-kernel + 1 samples (default 1; 0 .. 4); it is a detection image already, so there is no envelope step.
cf is delay-and-sum weighted by the coherence factor to the power --gamma (default 1; 0 is delay-and-sum).  Like capon both work on I/Q
data, so they imply --iq and a lambda / 2 step, and take no --apodization.
--iq: the I/Q chain (DESIGN D20) -- the channel data are demodulated at the carrier and decimated by --decimation (default 4: 50 MHz ->
12.5 MHz), delay-and-sum runs on complex samples and the envelope is the modulus of each pixel, which needs no carrier on the grid: the
example then scans at lambda / 2 axially.  Delay-and-sum only.
--polar: the beamformer runs on a sector (PolarScan, DESIGN D21) -- rays over the opening angle of the curved array, or over the x-range
seen from the deepest z under the linear one -- the envelope is taken along the rays, and the scan conversion brings it onto the Cartesian
grid of the other runs.  Combines with every option above.
--apodization: the receive window on the f-number aperture of every pixel (DESIGN D22) -- boxcar (default), tukey (--alpha, default 0.5),
hann or hamming: lower side lobes around the specular plate for a wider main lobe.  Combines with every option above.  --profile prints the device time of each step (HIP events)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pbrt_amd as mi                       # was: import mitsuba as mi
import pbrt_amd.drjit_compat as dr          # was: import drjit as dr

mi.set_variant("llvm_ad_mono")              # accepted; the one backend is HIP on gfx950
ap = argparse.ArgumentParser()
ap.add_argument("--convex", action="store_true")
ap.add_argument("--beamformer", choices=("das", "pdas", "fdmas", "capon", "slsc", "cf"), default="das")
ap.add_argument("--p", type=float, default=2.0)
ap.add_argument("--l-prop", type=float, default=0.5)
ap.add_argument("--delta-l", type=float, default=0.01)
ap.add_argument("--lag-prop", type=float, default=0.3)
ap.add_argument("--half-kernel", type=int, default=1)
ap.add_argument("--gamma", type=float, default=1.0)
ap.add_argument("--iq", action="store_true")
ap.add_argument("--decimation", type=int, default=4)
ap.add_argument("--polar", action="store_true")
ap.add_argument("--apodization", choices=("boxcar", "tukey", "hann", "hamming"), default="boxcar")
ap.add_argument("--alpha", type=float, default=0.5)
ap.add_argument("--profile", action="store_true")
ap.add_argument("out_dir", nargs="?", default=".")
args = ap.parse_args()
if args.beamformer == "capon":
    if args.apodization != "boxcar":
        ap.error("--beamformer capon makes its own weights: no --apodization (DESIGN D23)")
    args.iq = True
if args.beamformer in ("slsc", "cf"):
    if args.apodization != "boxcar":
        ap.error(f"--beamformer {args.beamformer} takes no receive window: no --apodization (DESIGN D26)")
    args.iq = True
if args.iq and args.beamformer not in ("das", "capon", "slsc", "cf"):
    ap.error("--iq takes delay-and-sum, Capon, SLSC or CF: the non-linear beamformers are defined on RF data (DESIGN D19)")
convex, out_dir = args.convex, args.out_dir
T = mi.ScalarTransform4f
RADIUS = 0.04 if convex else 0.0            # centre of curvature RADIUS behind the apex; the scan's z is measured from it
Z_RANGE = (RADIUS + 0.02, RADIUS + 0.08)

scene = mi.load_dict({
    "type": "scene",
    "integrator": {"type": "ultrasound_integrator", "max_depth": 10, "sampling_rate": 50e6, "frequency": 5e6,
                   "sound_speed": 1540, "attenuation": 0.2, "wave_cycles": 5, "main_beam_angle": 24, "cutoff_angle": 30,
                   "n_elements": 64, "pitch": 1.2e-4, "time_samples": 10000, "angles": dr.linspace(mi.Float, -15, 15, 5),
                   "paths_per_ray": 4096, "seed": 1, **({"radius": RADIUS, "opening_angle": 40.0} if convex else {})},
    "sensor": {"type": "ultrasound_sensor", "num_elements_lateral": 1280, "elements_width": 0.003, "elements_height": 0.01,
               "pitch": 0.0003, "center_frequency": 5e6, "sound_speed": 1540, "directivity": 1.0,
               "to_world": T().look_at(origin=[0, 0, -RADIUS], target=[0, 0, 0.03], up=[0, 1, 0])},
    "flat_plate": {"type": "rectangle",
                   "to_world": T().translate([0, 0, 0.05]) @ T().rotate([0, 1, 0], 45) @ T().scale([0.17, 0.17, 0.14]),
                   "bsdf": {"type": "ultrasound_bsdf", "impedance": 7.8, "roughness": 0.7}},
    "wall_back": {"type": "rectangle",
                  "to_world": T().translate([0, 0, 1]) @ T().rotate([0, 1, 0], 180) @ T().scale([0.05, 0.05, 1]),
                  "bsdf": {"type": "ultrasound_bsdf", "impedance": 7.8, "roughness": 0.7}},
})

integ = scene.integrator()
lam = integ.sound_speed / integ.frequency
window = dict(rx_apodization=args.apodization, rx_apodization_alpha=args.alpha)
beamformer = {"das": lambda: mi.DelayAndSum(**window), "pdas": lambda: mi.PDelayAndSum(p=args.p, **window),
              "fdmas": lambda: mi.FilteredDelayMultiplyAndSum(**window),
              "capon": lambda: mi.Capon(l_prop=args.l_prop, delta_l=args.delta_l),
              "slsc": lambda: mi.ShortLagSpatialCoherence(lag_prop=args.lag_prop, half_kernel=args.half_kernel),
              "cf": lambda: mi.CoherenceFactor(gamma=args.gamma)}[args.beamformer]()
step = {"das": lam / 4, "pdas": lam / 8, "fdmas": lam / 16, "capon": lam / 2, "slsc": lam / 2, "cf": lam / 2}[args.beamformer]
RENDER = dict(x_range=(-0.02, 0.02), z_range=Z_RANGE, step=step, beamformer=beamformer)
if args.iq:
    RENDER.update(iq=True, decimation=args.decimation, step=lam / 2)
    print(f"I/Q chain: demodulated at {integ.frequency / 1e6:.1f} MHz, {integ.fs / 1e6:.0f} -> {integ.fs / args.decimation / 1e6:.2f} MHz, "
          f"scan step lambda / 2 = {lam / 2 * 1e6:.0f} um (the Hilbert envelope of the RF chain needs lambda / 4 or finer)")
if args.polar:
    RENDER.update(scan="polar")
if args.beamformer in ("pdas", "fdmas"):
    f_lo, f_hi = beamformer.band(mi.build_probe("linear", 64, 1.2e-4, integ.frequency, 70))
    print(f"{beamformer}: band {f_lo / 1e6:.2f} - {f_hi / 1e6:.2f} MHz needs an axial rate c / (2 step) above {2 * f_hi / 1e6:.2f} MHz; "
          f"scan step lambda / {lam / step:.0f} = {step * 1e6:.1f} um gives {integ.sound_speed / (2 * step) / 1e6:.2f} MHz "
          f"(the reference's lambda / 4: {integ.sound_speed / (2 * lam / 4) / 1e6:.2f} MHz)")

t = time.perf_counter()
display, bmode, (x_scan, z_scan) = mi.us_render(scene, **RENDER)
print(f"B-mode {display.shape[0]} x {display.shape[1]} pixels in {(time.perf_counter() - t) * 1e3:.1f} ms; "
      f"channel_buf sum {float(np.sum(scene.integrator().channel_buf)):.4g}, max {float(np.max(scene.integrator().channel_buf)):.4g}")
if args.polar:
    sector = integ._render_plan.d_bf.shape
    print(f"sector {sector[0]} rays x {sector[1]} samples = {sector[0] * sector[1]} pixels beamformed, "
          f"{len(x_scan)} x {len(z_scan)} = {len(x_scan) * len(z_scan)} on the grid")
if args.profile:   # per step, by HIP events on the library's stream (a context that profiles queues the chain call by call)
    cx = scene.device().ctx
    cx.set_profiling(True)
    acc, N = {}, 10
    for _ in range(N):
        mi.us_render(scene, **RENDER)
        for k, v in cx.image_stats().items():
            if k.endswith("_ms"):
                acc[k] = acc.get(k, 0.0) + v / N
    cx.set_profiling(False)
    print("device time per step: " + ", ".join(f"{k[:-3]} {v * 1e3:.1f} us" for k, v in acc.items()))
np.save(os.path.join(out_dir, "bmode_display.npy"), display)
np.save(os.path.join(out_dir, "channel_buf.npy"), np.asarray(scene.integrator().channel_buf))

# the finite-difference loop of USMain.py:257-289; every forward run uses the same seed (common random numbers)
params = mi.traverse(scene)
key = [k for k in params.keys() if k.endswith("flat_plate.bsdf.roughness")][0]
target = bmode.astype(np.float64)


def forward(rough):
    params[key] = rough
    params.update()
    return mi.us_render(scene, **RENDER)[1].astype(np.float64)


rough, eps = 0.5, 1e-2
scale = float(np.mean(target ** 2))
for it in range(5):
    f0 = float(np.mean((forward(rough) - target) ** 2)) / scale
    f1 = float(np.mean((forward(rough + eps) - target) ** 2)) / scale
    grad = (f1 - f0) / eps
    rough = float(np.clip(rough - 0.05 * np.sign(grad), 1e-4, 1.0))
    print(f"iter {it}: relative loss {f0:.4g}, d loss / d roughness {grad:.4g}, roughness -> {rough:.3f}")
