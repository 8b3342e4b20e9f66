#!/usr/bin/env python3
"""Colour and power Doppler of a moving target (DESIGN D24): the steel box of tests/scenes/us_sphere_box.xml with its sphere moving
along z at --speed (m/s, positive = away from the probe) under the pulse repetition frequency --prf.  One scene per pulse -- geometry
cannot be updated in place -- every pulse with the same seed, the Gaussian pulse model (the impulse model ties the carrier to absolute
time and shows no Doppler shift), the I/Q chain, then doppler_render: wall filter, lag-one autocorrelation, smoothing, maps.  Writes
doppler_velocity.npy and doppler_power.npy (and doppler.png when matplotlib is there) and prints the median velocity inside the
sphere's outline beside the speed asked for.  The colour map is NEGATIVE for motion away from the probe.
    python examples/us_doppler.py [--speed V] [--prf F] [--pulses N] [--wall {none,mean,poly}] [--degree D] [--kernel KX KZ]
                                    [--paths P] [out_dir]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pbrt_amd as mi
from pbrt_amd.xml_loader import load_xml_to_dict

ap = argparse.ArgumentParser()
ap.add_argument("--speed", type=float, default=0.05)
ap.add_argument("--prf", type=float, default=2000.0)
ap.add_argument("--pulses", type=int, default=8)
ap.add_argument("--wall", choices=("none", "mean", "poly"), default="none")
ap.add_argument("--degree", type=int, default=1)
ap.add_argument("--kernel", type=int, nargs=2, default=(3, 3))
ap.add_argument("--paths", type=int, default=256)
ap.add_argument("out_dir", nargs="?", default=".")
args = ap.parse_args()

XML = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "scenes", "us_sphere_box.xml")
T = mi.ScalarTransform4f
Z0, R = 0.08, 0.06


def pulse(n):
    """the scene at pulse n: the sphere n * speed / prf further along z"""
    d = load_xml_to_dict(XML, paths_per_ray=args.paths, seed=1)
    d["integrator"].update(pulse_model="gaussian", angles=np.asarray([0.0], np.float32))
    d["sphere"]["to_world"] = T().translate([0, 0, Z0 + n * args.speed / args.prf]) @ T().scale([R, R, R])
    return mi.load_dict(d)


scenes = [pulse(n) for n in range(args.pulses)]
integ = scenes[0].integrator()
lam = integ.sound_speed / integ.frequency
nyq = mi.nyquist_velocity(integ.sound_speed, args.prf, integ.frequency)
print(f"{args.pulses} pulses at {args.prf:.0f} Hz, sphere at {args.speed:+.4f} m/s = {args.speed / args.prf / lam:+.4f} lambda per pulse; "
      f"Nyquist velocity {nyq:.4f} m/s" + ("  (ALIASED: |speed| exceeds it)" if abs(args.speed) >= nyq else ""))
t = time.perf_counter()
velocity, power, (x, z) = mi.doppler_render(scenes, args.prf, x_range=(-0.01, 0.01), z_range=(0.01, 0.04), decimation=4,
                                            wall_filter=args.wall, degree=args.degree, kernel=tuple(args.kernel), dynamic_range=40.0)
print(f"maps of {velocity.shape[0]} x {velocity.shape[1]} pixels in {(time.perf_counter() - t) * 1e3:.1f} ms")
np.save(os.path.join(args.out_dir, "doppler_velocity.npy"), velocity)
np.save(os.path.join(args.out_dir, "doppler_power.npy"), power)

# inside the sphere's outline, where the power display is within 20 dB (the upper half of a 40 dB range) of its maximum
zz, xx = np.meshgrid(z, x, indexing="ij")
inside = (xx ** 2 + (zz - Z0) ** 2 <= R ** 2) & (power >= 0.5)
if inside.any():
    print(f"median velocity on {int(inside.sum())} pixels inside the sphere's outline: {float(np.median(velocity[inside])):+.4f} m/s; "
          f"asked for {args.speed:+.4f} m/s away from the probe, which the map shows as {-args.speed:+.4f}")
else:
    print("no pixel inside the sphere's outline reaches the upper half of the display range")
try:
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig, axes = plt.subplots(1, 2, figsize=(9, 4))
    ext = (x[0] * 1e3, x[-1] * 1e3, z[-1] * 1e3, z[0] * 1e3)
    axes[0].imshow(velocity, extent=ext, cmap="seismic", vmin=-nyq, vmax=nyq, aspect="auto")
    axes[0].set_title("velocity (m/s, negative: away)")
    axes[1].imshow(power, extent=ext, cmap="hot", aspect="auto")
    axes[1].set_title("power Doppler (40 dB)")
    fig.savefig(os.path.join(args.out_dir, "doppler.png"), dpi=120)
except ImportError:
    pass
