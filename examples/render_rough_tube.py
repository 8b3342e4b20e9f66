#!/usr/bin/env python3
"""Radiance mode: the scene of the reference's first prototype -- one `cylinder` whose BSDF is a GGX `roughconductor` -- with the
light the prototype lacks (it has no emitter and renders black).
    python examples/render_rough_tube.py [res] [spp] [alpha] [out.npy]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pbrt_amd as mi

res = int(sys.argv[1]) if len(sys.argv) > 1 else 512
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 256
alpha = float(sys.argv[3]) if len(sys.argv) > 3 else 0.1
out = sys.argv[4] if len(sys.argv) > 4 else "rough_tube.npy"
scene = mi.load_dict({
    "type": "scene",
    "integrator": {"type": "path"},
    "cylinder": {"type": "cylinder", "radius": 0.2, "p0": [0, -0.5, 0], "p1": [0, 0.5, 0],
                 "bsdf": {"type": "roughconductor", "alpha": alpha, "distribution": "ggx"}},
    "lamp": {"type": "point", "position": [0.5, 0.5, 2.0], "intensity": {"type": "rgb", "value": [3.0, 3.0, 3.0]}},
    "sensor": {"type": "perspective",
               "to_world": mi.ScalarTransform4f().look_at(origin=[0, 0, 2], target=[0, 0, 0], up=[0, 1, 0]),
               "film": {"type": "hdrfilm", "width": res, "height": res, "rfilter": {"type": "box"}},
               "sampler": {"type": "independent", "sample_count": spp}}})
mi.render(scene, seed=0)                                                                     # warm-up: upload, first launch
t = time.perf_counter()
img = mi.render(scene, seed=0)
dt = time.perf_counter() - t
st = mi.default_context().stats()
print(f"{res} x {res} x {spp} spp, alpha {alpha}: {dt * 1e3:.2f} ms wall, {st['kernel_ms']:.2f} ms on the GPU = "
      f"{res * res * spp / st['kernel_ms'] / 1e3:.0f} Msamples/s; mean radiance {img.mean():.4f}")
np.save(out, img)

# roughness is a scene parameter: params.update() overwrites the material record on the device, no rebuild
params = mi.traverse(scene)
params["cylinder.bsdf.alpha"] = 4 * alpha
params.update()
print(f"alpha {4 * alpha}: mean radiance {mi.render(scene, seed=0).mean():.4f}")
