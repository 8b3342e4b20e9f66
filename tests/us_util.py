"""Shared by the acquisition tests (test_us_bound.py on the CPU, test_gpu_ultrasound.py and test_gpu_us_shapes.py on the GPU): the
per-bin tolerance a float32 acquisition kernel is held to against the CPU oracle (oracle/oracle.cpp oracle_us_acquire).

The oracle reports, per channel bin, what the bin is a sum of (OracleScene.us_acquire(..., bounds=True)): abs_sum = sum |p| over
the echoes p deposited there, count = how many, ramp_sum = sum |p / D| over those whose directivity angle lies on the ramp of the
directivity weight D, all scaled by 1 / norm_paths like the buffer.  The bound is

    |got - ref| <= (count + c) u abs_sum + K_D u ramp_sum + u |ref|,      u = 2^-24,
    c = 22 + 14 max_depth,      K_D = 10 ac / (ac - am) + 4.

Derivation.  Write "k ulp" for an error of k units in the last place of a float32 result x: at most 2 k u |x|.

1. The echo.  The device (kernels_us.h k_us_bounce / k_us_first, kernels_us_wavefront.h k_us_shade) and the oracle evaluate each
   echo with the same float32 operations in the same order: IEEE round-to-nearest, no contraction, every fma spelled out, / and
   sqrtf correctly rounded on both sides ("Numeric contract"); the first-bounce tables are the same statements run once
   per (ray, receiver).  The hit, the receiver draw, the visibility, the total time, its bin tf and the phase are therefore the same
   bits on both sides -- the assertion that the non-zero bins are identical relies on exactly this, and a bin whose time index or
   visibility differs is a finding, not something this bound absorbs.  The pressure p = ((atten amp) D w_o) carrier [w_ray] takes
   three factors from library routines that differ between the device (ocml) and the host (glibc):
   - carrier = sinf(phase): ocml within 4 ulp (the OpenCL single-precision limit), glibc within 1 ulp: they differ by <= 5 ulp
     = 10 u |carrier|;
   - atten *= expf(katt d / 8.686) once per bounce: <= 3 + 1 ulp = 8 u per factor.  The roulette then divides atten by
     rr = min(|atten amp|, 1): for rr < 1 that cancels the difference carried so far (rr carries it too), for rr = 1 it carries on;
     either way a bounce adds at most 8 u plus 2 u for each of the three roundings (atten e, atten amp, atten / rr) that now act on
     operands that differ: 14 u per bounce, <= max_depth bounces up to an echo;
   - D = (ac - alpha) / (ac - am) with alpha = |acosf(.)|, on the ramp am < alpha <= ac (1 below it, 0 beyond it; continuous at
     both ends, so a threshold taken on one side only changes D as much as the ramp does): acosf <= 4 + 1 ulp = 10 u alpha, plus
     2 u (ac - alpha) for the subtraction and 2 u D for the division: |dD| <= (10 ac / (ac - am) + 4) u = K_D u.  This is an
     absolute error of D, not a relative one -- an echo near the cutoff has D -> 0 and keeps it -- so it weighs |p / D|; ramp_sum
     sums exactly the echoes within 2^-16 ac of the ramp, far wider than any acosf error.
   The four products after the perturbed factors (atten amp, x D w_o, x carrier, x w_ray) and D w_o itself round operands that
   differ: 2 u each, 10 u.  Everything else (amp, w_o, w_ray: the emitter's sin / cos are the fixed polynomial of omath.h
   sincos_pi4 up to 45 degrees on both sides) is the same bits.  Per echo: |p_dev - p_ref| <= (20 + 14 max_depth) u |p_ref|
   + K_D u |p_ref / D| [on the ramp].
2. The sum.  The device adds a bin's echoes in float32 in an order it does not fix: within a workgroup ds_add_f32 into the bin of
   the LDS echo table that the channel index claimed (or a global atomic when another index holds the bin), then one global
   atomic per table bin at the flush, in any order of workgroups.  That is a summation tree of count terms: error
   <= (count - 1) u sum |p_dev|.  The oracle sums in float64 in path order and rounds once: <= u |ref| (its float64 error,
   count 2^-53 abs_sum, is below the slack of the next point).
3. The scale.  k_scale multiplies the float32 sum by fl(1 / norm_paths): 1 u for the reciprocal, 1 u for the product, on
   |sum| <= abs_sum: 2 u abs_sum.  The oracle scales in float64 before its one rounding (point 2).
Adding up: (count - 1) + 2 + 20 + 14 max_depth = count + 21 + 14 max_depth; one more u abs_sum covers the second-order terms
(sum |p_dev| against sum |p_ref|, the 1 / (1 - count u) of the summation bound): c = 22 + 14 max_depth.  A bin without
echoes (count = 0) must be exactly 0 on the device.
"""
import numpy as np

U32 = 2.0 ** -24          # unit roundoff of float32
C_BASE = 22.0             # sinf (10), the products after the perturbed factors (10), k_scale (2), minus 1 of (count - 1), plus 1
C_PER_BOUNCE = 14.0       # expf (8) and three roundings on perturbed operands (6) per bounce


def ramp_gain(p):
    """K_D of the module docstring from the acquisition's parameters (pbrt_us_params: degrees, as the kernels convert them)"""
    am = float(np.float32(p.main_beam_angle) * np.float32(np.pi / 180.0))
    ac = float(np.float32(p.cutoff_angle) * np.float32(np.pi / 180.0))
    return 10.0 * ac / (ac - am) + 4.0


def tolerance(ref, extra, p):
    """per-bin tolerance of a float32 acquisition against the oracle's channel buffer ref; extra: the third value of
    OracleScene.us_acquire(..., bounds=True); p: the pbrt_us_params of the acquisition"""
    c = C_BASE + C_PER_BOUNCE * float(p.max_depth)
    cnt = extra["count"].astype(np.float64)
    tol = (cnt + c) * U32 * extra["abs_sum"].astype(np.float64) + ramp_gain(p) * U32 * extra["ramp_sum"].astype(np.float64)
    return tol + U32 * np.abs(np.asarray(ref, np.float64))


def excess(got, ref, tol):
    """|got - ref| / tol per bin (0 where both are exactly 0; inf where tol is 0 and they differ)"""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / tol)
    return np.where(np.isnan(r), np.inf, r)


def worst_ratio(got, ref, tol):
    """the largest |got - ref| / tol over the buffer"""
    return float(excess(got, ref, tol).max())


def acquire_ref(ob, sc, ui, seed, ppr, quirks=None, **kw):
    """the oracle's (ref, tx, tol) for the integrator ui of scene sc"""
    p = ui.us_params(sc, quirks)
    ref, tx, extra = ob.OracleScene.from_scene(sc).us_acquire(p, seed, ppr, bounds=True, **kw)
    return ref, tx, tolerance(ref, extra, p)


def phantom(mi, kind, n_elements, angles, time_samples, ppr, seed, max_depth=4, quirks=None, emitter=False, pitch=2e-4):
    """cheap phantoms in front of a linear probe at the origin looking along +z, by load_dict:
    "plate": one steel plate at 20 mm, tilted by 4 degrees (brute force; at exactly normal incidence the reference's GGX frame
             divides 0 by 0);
    "few":   two spheres and three plates between 15 and 55 mm, echoes over bins ~800 - 3000 (brute force, fused k_us_bounce);
    "bvh":   "few" and 36 small plates more: > 32 primitives, the BVH streams (k_trace + k_us_shade)
    "cone":  "few" and one analytic cone between 21 and 28 mm, its base turned half towards the probe: at 128 elements the rays of
             about 18 elements meet its base and those of 18 more its lateral surface (brute force, the _BIG instances of k_us_bounce)
    emitter=True adds an ultrasound_emitter with the probe's elements and primary_rays="emitter" (the EMIT instances)"""
    T = mi.ScalarTransform4f
    rng = np.random.default_rng(seed)
    bsdf = lambda z, r: {"type": "ultrasound_bsdf", "impedance": z, "roughness": r}   # noqa: E731
    d = {"type": "scene",
         "integrator": {"type": "ultrasound_integrator", "max_depth": max_depth, "sampling_rate": 40e6, "frequency": 4e6,
                        "sound_speed": 1500.0, "attenuation": 0.3, "main_beam_angle": 20, "cutoff_angle": 35, "n_elements": n_elements,
                        "pitch": pitch, "time_samples": time_samples, "angles": np.asarray(angles, np.float32), "paths_per_ray": ppr,
                        "seed": seed, "primary_rays": "emitter" if emitter else "element", **({} if quirks is None else {"quirks": quirks})},
         "sensor": {"type": "ultrasound_sensor", "to_world": T().look_at([0, 0, 0], [0, 0, 0.03], [0, 1, 0])}}
    if emitter:
        d["emitter"] = {"type": "ultrasound_emitter", "number_of_elements": n_elements, "pitch": pitch, "element_width": 1e-4,
                        "element_height": 4e-4, "speed_of_sound": 1500.0, "steering_angle_min": -12.0, "steering_angle_max": 12.0}
    if kind == "plate":
        d["p"] = {"type": "rectangle", "to_world": T().translate([0, 0, 0.02]) @ T().rotate([0, 1, 0], 4) @ T().rotate([1, 0, 0], 180)
                  @ T().scale([0.03, 0.03, 1]), "bsdf": bsdf(7.8, 0.8)}
        return mi.load_dict(d)
    for i, (x, z, r) in enumerate([(-0.00413, 0.025, 0.004), (0.00517, 0.04, 0.006)]):
        d[f"s{i}"] = {"type": "sphere", "center": [x, 0.0, z], "radius": r, "bsdf": bsdf(5.0, 0.6)}
    for i, (x, z, tilt) in enumerate([(0.0, 0.015, 6.0), (-0.008, 0.035, -20.0), (0.002, 0.055, 10.0)]):
        d[f"p{i}"] = {"type": "rectangle", "to_world": T().translate([x, 0, z]) @ T().rotate([0, 1, 0], tilt) @ T().rotate([1, 0, 0], 180)
                      @ T().scale([0.004 + 0.004 * i, 0.008, 1]), "bsdf": bsdf(7.8, 0.9)}
    if kind == "bvh":
        for i in range(36):
            tw = T().translate([float(rng.uniform(-0.015, 0.015)), float(rng.uniform(-0.004, 0.004)), float(rng.uniform(0.03, 0.06))]) @ \
                T().rotate([0, 1, 0], float(rng.uniform(-40, 40))) @ T().rotate([1, 0, 0], float(rng.uniform(150, 210))) @ \
                T().scale([float(rng.uniform(0.001, 0.003)), float(rng.uniform(0.002, 0.005)), 1])
            d[f"q{i}"] = {"type": "rectangle", "to_world": tw, "bsdf": bsdf(float(rng.uniform(2, 8)), float(rng.uniform(0.3, 0.9)))}
    if kind == "cone":     # the closed unit cone (apex (0, 0, 1), base disc of radius 1 at z = 0) under to_world
        d["c"] = {"type": "cone", "to_world": T().translate([0.0065, 0.0005, 0.024]) @ T().rotate([1, 0, 0], 10) @ T().rotate([0, 1, 0], 60)
                  @ T().scale([0.0035, 0.0035, 0.007]), "bsdf": bsdf(6.0, 0.7)}
    sc = mi.load_dict(d)
    P = sc.flatten()["prims"]
    assert (len(P) > 32) == (kind == "bvh")
    assert bool(np.any(P["type"] == mi._capi.PRIM_CONE)) == (kind == "cone")
    return sc
