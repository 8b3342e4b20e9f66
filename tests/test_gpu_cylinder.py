"""The analytic cylinder on the DEVICE.  The CPU oracle does not know PBRT_PRIM_CYLINDER, so these checks are closed
forms, the float64 restatement of tests/cylinder_util.py, and agreement between the library's own kernel families: the brute-force
kernels, the BVH in LDS and in global memory, the fused ultrasound bounce against the BVH streams, with and without the
first-bounce tables."""
import math

import numpy as np
import pytest

import cylinder_util as cu
from conftest import scene_path

pytestmark = pytest.mark.gpu


def _accel(capi, name):
    return {"brute": capi.ACCEL_BRUTE, "bvh": capi.ACCEL_BVH, "bvh_global": capi.ACCEL_BVH_GLOBAL}[name]


def _skewed(mi):
    """rotated, mirrored (det < 0), non-uniformly scaled, translated"""
    T = mi.ScalarTransform4f
    return T().translate([0.2, -0.1, 0.3]) @ T().rotate([0.3, 1.0, -0.4], 28.0) @ T().scale([-1.2, 0.7, 1.1])


def _rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(np.asarray(b, np.float64)), 1e-30))


# ---- 1. hand-computed hits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("frame", ["plain", "skewed"])
def test_hand_computed_hits(mi, capi, flip, frame):
    """rays written in the tube's object space (radius 1, 0 <= z <= 1) and mapped to the world: outside -> near wall, inside -> far
    wall, through an open end, parallel to the axis inside and outside, tangent (and 1e-3 inside / outside of it)"""
    tw = _skewed(mi) if frame == "skewed" else None
    kw = dict(p0=[0.0, 0.0, -0.5], p1=[0.0, 0.0, 1.5], radius=0.5) if frame == "plain" else \
        dict(p0=[0.1, -0.2, 0.0], p1=[0.3, 0.9, 0.4], radius=0.3, to_world=tw)
    sc = mi.load_dict({"type": "scene", "c": {"type": "cylinder", "flip_normals": flip, **kw}})
    sc.accel = capi.ACCEL_BRUTE
    O = cu.object_to_world(kw["p0"], kw["p1"], kw["radius"], None if tw is None else tw.matrix)
    #        origin (object)        direction (object)   t (object units of d)  hit point (object) or None
    cases = [((3.0, 0.0, 0.5), (-1.0, 0.0, 0.0), 2.0, (1.0, 0.0, 0.5)),      # outside -> near wall
             ((0.2, 0.0, 0.5), (1.0, 0.0, 0.0), 0.8, (1.0, 0.0, 0.5)),       # inside -> far wall
             ((0.0, -0.3, 0.3), (0.0, -1.0, 0.0), 0.7, (0.0, -1.0, 0.3)),    # inside, other side
             ((0.0, 0.0, -1.0), (0.3, 0.0, 1.0), None, None),                # through the open end z = 0 (and out at z = 1)
             ((0.5, 0.0, -1.0), (0.0, 0.0, 1.0), None, None),                # parallel to the axis, inside
             ((2.0, 0.0, -1.0), (0.0, 0.0, 1.0), None, None),                # parallel to the axis, outside
             ((0.999, -2.0, 0.5), (0.0, 1.0, 0.0), 2.0 - math.sqrt(1 - 0.999 ** 2), None),  # just inside the tangent: hit
             ((1.001, -2.0, 0.5), (0.0, 1.0, 0.0), None, None)]              # just outside: miss
    oo = np.array([c[0] for c in cases])
    do = np.array([c[1] for c in cases])
    o = oo @ O[:3, :3].T + O[:3, 3]
    dw = do @ O[:3, :3].T
    scale = np.linalg.norm(dw, axis=1)
    d = dw / scale[:, None]
    r = sc.ray_intersect(o, d)
    for i, (_, _, t_obj, q) in enumerate(cases):
        if t_obj is None:
            assert not r["valid"][i], i
            continue
        assert r["valid"][i] and r["prim"][i] == 0 and r["u"][i] == 0 and r["v"][i] == 0, i
        assert r["t"][i] == pytest.approx(t_obj * scale[i], rel=1e-5), i
        if q is None:
            continue
        pw = O[:3, :3] @ np.array(q) + O[:3, 3]
        assert np.allclose(r["p"][i], pw, atol=2e-6 * (1 + np.abs(pw).max())), i
        nw = np.linalg.inv(O[:3, :3]).T @ np.array([q[0], q[1], 0.0])     # outward: the gradient of x^2 + y^2 to the world
        nw = nw / np.linalg.norm(nw) * (-1.0 if flip else 1.0)
        assert np.allclose(r["n"][i], nw, atol=2e-4), i
    # exactly tangent (plain frame: exact arithmetic, disc = 0): a hit if any at the touching point
    t1 = sc.ray_intersect(O[:3, :3] @ np.array([1.0, -2.0, 0.5]) + O[:3, 3], O[:3, :3] @ np.array([0.0, 1.0, 0.0]) /
                          np.linalg.norm(O[:3, :3] @ np.array([0.0, 1.0, 0.0])))
    if t1["valid"][0]:
        assert np.allclose(t1["p"][0], O[:3, :3] @ np.array([1.0, 0.0, 0.5]) + O[:3, 3], atol=1e-3)
    elif frame == "plain":
        pytest.fail("the exactly tangent ray of the plain frame has disc = 0 and touches the tube")


def test_c_abi_refusals(mi, capi):
    """a singular or non-finite record is PBRT_E_INVALID, an area light on a cylinder PBRT_E_UNSUPPORTED"""
    f = mi.load_dict({"type": "scene", "c": {"type": "cylinder"}}).flatten()
    ctx = capi.default_context()
    empty_e = np.zeros(0, dtype=capi.EMITTER_DTYPE)
    for g in (np.zeros(12), np.r_[np.eye(3, 4).ravel()[:11], np.nan], np.r_[1.0, 0, 0, 0, 0, 1.0, 0, 0, 1.0, 1.0, 0, 0]):
        P = f["prims"].copy()
        P["g"][0] = g
        with pytest.raises(RuntimeError, match="rc=-1"):
            capi.DeviceScene(ctx, P, f["materials"], empty_e, np.zeros(0, np.uint32), np.zeros(0, np.float32))
    e = np.zeros(1, dtype=capi.EMITTER_DTYPE)
    e["type"], e["count"], e["area"] = capi.EMIT_AREA, 1, 1.0
    P = f["prims"].copy()
    P["emitter"] = 0
    with pytest.raises(RuntimeError, match="rc=-4"):
        capi.DeviceScene(ctx, P, f["materials"], e, np.zeros(1, np.uint32), np.ones(1, np.float32))
    capi.DeviceScene(ctx, f["prims"], f["materials"], empty_e, np.zeros(0, np.uint32), np.zeros(0, np.float32)).close()


# ---- 2. random rays against the float64 restatement --------------------------------------------------------------------------------
def _random_rays(O, n, rng):
    """built in the tube's object space (radius 1, 0 <= z <= 1) and mapped to the world: origins in a box around the tube, a fifth
    of them inside it, aimed at points scattered about the surface (some beyond the open ends)"""
    oo = rng.uniform([-3.0, -3.0, -1.0], [3.0, 3.0, 2.0], (n, 3))
    inside = rng.random(n) < 0.2
    rr, ph = 0.8 * np.sqrt(rng.random(inside.sum())), rng.uniform(0, 2 * np.pi, inside.sum())
    oo[inside] = np.stack([rr * np.cos(ph), rr * np.sin(ph), rng.uniform(0.05, 0.95, inside.sum())], axis=1)
    ph = rng.uniform(0, 2 * np.pi, n)
    tgt = np.stack([np.cos(ph), np.sin(ph), rng.uniform(-0.3, 1.3, n)], axis=1) + rng.normal(0, 0.3, (n, 3))
    o = oo @ O[:3, :3].T + O[:3, 3]
    d = (tgt - oo) @ O[:3, :3].T
    return o.astype(np.float32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _cyl_kw(mi):
    return dict(p0=[0.1, -0.3, 0.2], p1=[-0.2, 0.6, 0.5], radius=0.25, to_world=_skewed(mi))


def test_random_rays_against_the_restatement(mi, capi):
    """one cylinder, brute force: hit / miss, t (rel. 1e-5), normals (2e-4) against the float64 definition away from the rims and
    the silhouette; ray_test equals `valid` under a finite tmax"""
    kw = _cyl_kw(mi)
    sc = mi.load_dict({"type": "scene", "c": {"type": "cylinder", **kw}})
    sc.accel = capi.ACCEL_BRUTE
    W = cu.record_matrix(sc.flatten()["prims"][0])
    O = cu.object_to_world(kw["p0"], kw["p1"], kw["radius"], kw["to_world"].matrix)
    rng = np.random.default_rng(11)
    o, d = _random_rays(O, 20000, rng)
    ref = cu.intersect(W, o, d)
    r = sc.ray_intersect(o, d)
    sure = ref["margin"] > 1e-4
    assert sure.mean() > 0.95 and ref["valid"][sure].mean() > 0.3
    assert np.array_equal(r["valid"][sure], ref["valid"][sure])
    # (t of a near-tangent root carries the float32 error of sqrt(disc), the near root of an origin close to the wall that of C)
    h = sure & ref["valid"] & (ref["chord"] > 0.1) & (ref["gap"] > 0.1)
    assert h.sum() > 5000
    assert np.allclose(r["t"][h], ref["t"][h], rtol=1e-5, atol=0)
    assert np.abs(r["n"][h] - ref["n"][h]).max() < 2e-4
    assert np.all(r["prim"][r["valid"]] == 0)
    tm = np.where(rng.random(len(o)) < 0.5, ref["t"] * rng.uniform(0.5, 1.5, len(o)), rng.uniform(0.1, 3.0, len(o))).astype(np.float32)
    tm = np.where(np.isfinite(tm), tm, 1.0).astype(np.float32)
    assert np.array_equal(sc.ray_test(o, d, tm), sc.ray_intersect(o, d, tm)["valid"])


def test_beside_triangles_all_accelerators_agree(mi, capi):
    """the same cylinder beside a 64-triangle mesh (a tessellated cone crossing it): brute force (the _BIG kernels), the BVH in
    LDS and in global memory give array_equal t and prim, ray_test equals `valid`; a sure cylinder hit of the restatement is
    reported as the cylinder at its t, or as a triangle in front of it"""
    T = mi.ScalarTransform4f
    kw = _cyl_kw(mi)
    d_ = {"type": "scene", "c": {"type": "cylinder", **kw},
          "m": {"type": "cone", "tessellate": True, "segments": 16, "rings": 2,
                "to_world": T().translate([0.1, 0.1, 0.2]) @ T().rotate([1, 0, 0], 70) @ T().scale([0.3, 0.3, 0.8])}}
    O = cu.object_to_world(kw["p0"], kw["p1"], kw["radius"], kw["to_world"].matrix)
    rng = np.random.default_rng(12)
    o, d = _random_rays(O, 20000, rng)
    tm = rng.uniform(0.2, 3.0, len(o)).astype(np.float32)
    res = {}
    for name in ("brute", "bvh", "bvh_global"):
        sc = mi.load_dict(d_)
        P = sc.flatten()["prims"]
        assert len(P) >= 41 and P["type"][0] == capi.PRIM_CYLINDER
        sc.accel = _accel(capi, name)
        res[name] = sc.ray_intersect(o, d)
        assert np.array_equal(sc.ray_test(o, d, tm), sc.ray_intersect(o, d, tm)["valid"]), name
    W = cu.record_matrix(P[0])
    ref = cu.intersect(W, o, d)
    for name in ("bvh", "bvh_global"):
        assert np.array_equal(res[name]["prim"], res["brute"]["prim"]), name
        assert np.array_equal(res[name]["t"], res["brute"]["t"]), name
    r = res["brute"]
    assert (r["prim"] == 0).sum() > 2000 and ((r["prim"] > 0) & r["valid"]).sum() > 2000
    sure = (ref["margin"] > 1e-4) & ref["valid"]
    on_cyl = sure & (r["prim"] == 0) & (ref["chord"] > 0.1) & (ref["gap"] > 0.1)
    assert np.allclose(r["t"][on_cyl], ref["t"][on_cyl], rtol=1e-5, atol=0)
    assert np.abs(r["n"][on_cyl] - ref["n"][on_cyl]).max() < 2e-4
    other = sure & (r["prim"] != 0)
    assert np.all(r["valid"][other]) and np.all(r["t"][other] <= ref["t"][other] * (1 + 1e-5))
    cyl_hits = r["valid"] & (r["prim"] == 0)
    assert np.all(ref["valid"][cyl_hits] | (ref["margin"][cyl_hits] <= 1e-4))


# ---- 3. radiance closed form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", ["path", "direct"])
@pytest.mark.parametrize("accel", ["brute", "bvh", "bvh_global"])
def test_emitting_box_around_a_diffuse_tube(mi, capi, integrator, accel):
    """six walls emitting Le with reflectance 0 around a diffuse tube of albedo rho (axis along y, its ends out of view): the
    background is Le (exactly at max_depth 1); the tube, convex from outside, sees only the walls, so a pixel fully on it is rho Le in expectation
    (and exactly 0 at max_depth 1); the covered columns are the projected width of the tube within one"""
    T = mi.ScalarTransform4f
    rho, Le, res, fov, R, D = 0.6, 0.8, 32, 40.0, 0.25, 0.95
    black = {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.0, 0.0, 0.0]}}
    walls = {
        "zp": T().translate([0, 0, 1]).rotate([0, 1, 0], 180), "zn": T().translate([0, 0, -1]),
        "xp": T().translate([1, 0, 0]).rotate([0, 1, 0], -90), "xn": T().translate([-1, 0, 0]).rotate([0, 1, 0], 90),
        "yp": T().translate([0, 1, 0]).rotate([1, 0, 0], 90), "yn": T().translate([0, -1, 0]).rotate([1, 0, 0], -90)}

    def scene(max_depth):
        d = {"type": "scene", "integrator": {"type": integrator, "max_depth": max_depth} if integrator == "path" else {"type": "direct"},
             "sensor": {"type": "perspective", "fov": fov, "near_clip": 1e-3, "far_clip": 100.0,
                        "to_world": T().look_at([0, 0, -D], [0, 0, 0], [0, 1, 0]),
                        "sampler": {"type": "independent", "sample_count": 64},
                        "film": {"type": "hdrfilm", "width": res, "height": res, "rfilter": {"type": "box"}}},
             "tube": {"type": "cylinder", "p0": [0, -0.97, 0], "p1": [0, 0.97, 0], "radius": R,
                      "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [rho] * 3}}}}
        for k, t in walls.items():
            d[k] = {"type": "rectangle", "to_world": t, "bsdf": black, "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [Le] * 3}}}
        sc = mi.load_dict(d)
        sc.accel = _accel(capi, accel)
        return sc

    img = mi.render(scene(4), seed=2, spp=64)
    assert img.shape == (res, res, 3) and np.isfinite(img).all()
    # image-plane x of the silhouette: tan(asin(R / D)); a column of width 2 tan(fov / 2) / res
    xs = math.tan(math.asin(R / D)) / (2 * math.tan(math.radians(fov / 2)) / res)
    edges = np.arange(res + 1) - res / 2
    full = (edges[:-1] >= -xs + 0.05) & (edges[1:] <= xs - 0.05)
    free = (edges[1:] <= -xs - 0.05) | (edges[:-1] >= xs + 0.05)
    assert full.sum() >= 10 and free.sum() >= 4
    assert np.allclose(img[:, free], Le, rtol=1e-6, atol=0)      # (64 samples of Le summed and divided in float32)
    tube = img[:, full]
    assert tube.mean() == pytest.approx(rho * Le, rel=2e-2)
    assert np.abs(tube.mean(axis=(0, 2)) - rho * Le).max() < 0.1 * rho * Le
    # a column counts as covered when the tube fills most of it (its mean is nearer rho Le than Le)
    covered = np.abs(img.mean(axis=(0, 2)) - rho * Le) < np.abs(img.mean(axis=(0, 2)) - Le)
    assert abs(int(covered.sum()) - 2 * xs) <= 1
    if integrator == "path":
        img1 = mi.render(scene(1), seed=3, spp=4)
        assert np.all(img1[:, full] == 0) and np.all(img1[:, free] == np.float32(Le))


# ---- 4. echo arrival bins -------------------------------------------------------------------------------------------------------
V_D, V_R, V_C, V_FS, V_N, V_PITCH, V_T = 0.03, 0.004, 1540.0, 50e6, 15, 3e-4, 3000    # the vessel scene: depth, radius, c, fs, elements


def _vessel_scene(mi, max_depth=1, attenuation=0.0, emitter=False, x0=0.0):
    """a vessel whose axis lies along the probe's elevation direction at x = x0, unsteered, an odd element count (one element on the
    axis when x0 = 0);
    emitter=True adds an ultrasound_emitter without jitter: point elements, one steering angle of 0 degrees, three rays per element
    (every one the integrator's own ray, weight 1 / (N * 3)); the integrator keeps its own rays until primary_rays is set"""
    T = mi.ScalarTransform4f
    d = {"type": "scene",
         "integrator": {"type": "ultrasound_integrator", "max_depth": max_depth, "sampling_rate": V_FS, "frequency": 5e6, "sound_speed": V_C,
                        "attenuation": attenuation, "main_beam_angle": 80, "cutoff_angle": 85, "n_elements": V_N, "pitch": V_PITCH,
                        "time_samples": V_T, "angles": np.array([0.0], np.float32)},
         "sensor": {"type": "ultrasound_sensor", "to_world": T().look_at([0, 0, 0], [0, 0, 0.03], [0, 1, 0])},
         "vessel": {"type": "cylinder", "p0": [x0, -0.05, V_D], "p1": [x0, 0.05, V_D], "radius": V_R,
                    "bsdf": {"type": "ultrasound_bsdf", "impedance": 7.8, "roughness": 0.7}}}
    if emitter:
        d["emitter"] = {"type": "ultrasound_emitter", "number_of_elements": V_N, "pitch": V_PITCH, "element_width": 0.0, "element_height": 0.0,
                        "number_of_rays_per_element": 3, "speed_of_sound": V_C, "steering_angle_min": 0.0, "steering_angle_max": 0.0}
    return mi.load_dict(d)


def _check_vessel_arrival_bins(ui, buf):
    """element e with |x_e| < r hits at z_h = D - sqrt(r^2 - x_e^2) and its echo at receiver j arrives in bin
    round(fs (z_h + sqrt((x_j - x_e)^2 + z_h^2)) / c) within one; nothing else is heard, and the earliest bin is round(2 (D - r) / c fs)"""
    D, r, c, fs, N, n_t = V_D, V_R, V_C, V_FS, V_N, V_T
    assert buf.shape == (1, N, n_t)
    ex = ui.elem_x.numpy().astype(np.float64)
    assert np.any(np.abs(ex) < 1e-12) and np.abs(ex).max() < r
    allowed = np.zeros((N, n_t), bool)
    for e in range(N):
        zh = D - math.sqrt(r * r - ex[e] ** 2)
        for j in range(N):
            t = (zh + math.sqrt((ex[j] - ex[e]) ** 2 + zh * zh)) / c
            b = int(np.rint(t * fs))
            allowed[j, max(0, b - 1):min(n_t, b + 2)] = True
    nz = buf[0] != 0
    assert nz.sum() >= N and nz.any(axis=1).all() and not np.any(nz & ~allowed)
    assert np.argwhere(nz)[:, 1].min() == int(np.rint(2 * (D - r) / c * fs))


@pytest.mark.parametrize("tables", [True, False])
def test_vessel_echo_arrival_bins(mi, capi, tables):
    """the vessel scene at depth D, radius r, one bounce: the arrival bins of _check_vessel_arrival_bins, with and without the
    first-bounce tables"""
    sc = _vessel_scene(mi)
    ui = sc.integrator()
    q = ui.quirks | (0 if tables else capi.USQ_NO_FIRST_TABLES)
    _check_vessel_arrival_bins(ui, ui._acquire(sc, q, paths_per_ray=300, seed=5))


@pytest.mark.parametrize("accel", ["brute", "bvh"])
def test_vessel_echo_arrival_bins_with_emitter_rays(mi, capi, accel):
    """the same bins when every path's primary ray comes from the jitter-free emitter: drawn inside k_us_bounce<true, _BIG, true>
    (brute force), written by k_us_init_wf for k_trace + k_us_shade<., true> (the BVH streams); a ray from another element's origin
    lands outside the allowed bins"""
    sc = _vessel_scene(mi, emitter=True)
    sc.accel = _accel(capi, accel)
    ui = sc.integrator()
    ui.primary_rays = "emitter"
    assert ui.us_params(sc).primary == capi.US_PRIMARY_EMITTER
    _check_vessel_arrival_bins(ui, ui._acquire(sc, ui.quirks, paths_per_ray=300, seed=5))


@pytest.mark.parametrize("accel", ["brute", "bvh"])
def test_vessel_emitter_rays_without_jitter_are_the_integrators_own_rays(mi, capi, accel):
    """test_gpu_analytic.py::test_emitter_rays_without_jitter_are_the_integrators_own_rays on the vessel, four bounces: the emitter
    without jitter draws exactly the integrator's own primary ray, so every path is the same path and every echo the integrator's
    times the ray's weight 1 / (15 * 3).  The bounds are that test's: the emitter places its elements with linspace, the integrator
    with pitch * (i - (N - 1) / 2), positions that can differ in the last bit, so a roulette or time-bin decision may fall the other
    way for a path in a million.
    The vessel's axis lies half a pitch beside the probe's: with it at x = 0 the integrator's middle element (x = 0 exactly) meets the
    wall at exactly normal incidence, where the reference's literal arithmetic gives NaN echoes and ends the path,
    while the emitter's middle element lies at x = -5.8e-11 and goes on -- measured there, brute force and BVH alike: 15 NaN bins and
    1984 segments with the integrator's own rays, none and 2054 with the emitter's, rel. L2 7e-8 on the other bins.  Measured here:
    2058 segments on both sides, rel. L2 2.3e-6."""
    ppr = 96
    sc = _vessel_scene(mi, max_depth=4, attenuation=0.1, emitter=True, x0=V_PITCH / 2)
    sc.accel = _accel(capi, accel)
    ui = sc.integrator()
    own = ui._acquire(sc, ui.quirks, paths_per_ray=ppr, seed=4)
    st_own = mi.default_context().stats()
    ui.primary_rays = "emitter"
    assert ui.us_params(sc).primary == capi.US_PRIMARY_EMITTER
    em = ui._acquire(sc, ui.quirks, paths_per_ray=ppr, seed=4)
    st_em = mi.default_context().stats()
    w = 1.0 / (V_N * 3)
    assert st_own["segments"] >= V_N * ppr and abs(st_em["segments"] - st_own["segments"]) <= 1e-3 * st_own["segments"]
    assert all(abs(a - b) <= 1e-3 * max(b, 1) + 2 for a, b in zip(st_em["live"], st_own["live"]))
    assert np.isfinite(own).all() and np.abs(own).max() > 0 and np.mean((em != 0) == (own != 0)) > 0.9999
    ref = own.astype(np.float64) * w
    assert np.linalg.norm(em - ref) <= 1e-3 * np.linalg.norm(ref)


# ---- 5. the vessel phantom ------------------------------------------------------------------------------------------------------
def test_vessel_phantom_first_bounce_tables_change_nothing(mi, capi):
    sc = mi.load_file(scene_path("us_vessel_box.xml"), paths_per_ray=128, seed=8)
    ui = sc.integrator()
    with_tables = ui._acquire(sc, ui.quirks)
    without = ui._acquire(sc, ui.quirks | capi.USQ_NO_FIRST_TABLES)
    assert np.array_equal(with_tables != 0, without != 0) and (with_tables != 0).sum() > 100
    assert np.allclose(with_tables, without, rtol=2e-5, atol=1e-7 * np.abs(without).max())


def test_vessel_phantom_fused_bounce_against_the_bvh_streams(mi, capi):
    """the fused brute-force k_us_bounce (seven primitives) against the BVH streams (k_trace + k_us_shade, tree in LDS) and the tree
    in global memory: the same echoes"""
    ppr = 256
    bufs = {}
    for name in ("brute", "bvh", "bvh_global"):
        sc = mi.load_file(scene_path("us_vessel_box.xml"), paths_per_ray=ppr, seed=12)
        sc.accel = _accel(capi, name)
        ui = sc.integrator()
        bufs[name] = ui._acquire(sc, ui.quirks)
    ref = bufs["brute"]
    assert (ref != 0).sum() > 1000 and np.isfinite(ref).all()
    for name in ("bvh", "bvh_global"):
        assert np.array_equal(bufs[name] != 0, ref != 0), name
        assert _rel_l2(bufs[name], ref) <= 1e-3, name


def test_vessel_phantom_path_sharding_adds_up(mi):
    sc = mi.load_file(scene_path("us_vessel_box.xml"), seed=6)
    ui = sc.integrator()
    full = ui._acquire(sc, ui.quirks, paths_per_ray=300, seed=6)
    a = ui._acquire(sc, ui.quirks, paths_per_ray=100, path_offset=0, norm_paths=300, seed=6)
    b = ui._acquire(sc, ui.quirks, paths_per_ray=200, path_offset=100, norm_paths=300, seed=6)
    assert (full != 0).sum() > 1000
    assert _rel_l2(a + b, full) <= 1e-5 and np.array_equal((a + b) != 0, full != 0)


def _emitter_vessel_phantom(mi, capi, accel, ppr, seed):
    sc = mi.load_file(scene_path("us_vessel_box.xml"), primary_rays="emitter", paths_per_ray=ppr, seed=seed)
    sc.accel = _accel(capi, accel)
    return sc, sc.integrator()


def test_vessel_phantom_emitter_primary_rays(mi, capi, monkeypatch):
    """emitter rays on the vessel phantom by three routes of ray generation: drawn inside the fused brute-force bounce
    (k_us_bounce<true, _BIG, true>), written by k_us_init_wf for the BVH streams with the tree in LDS and in global memory -- the
    same echoes, by the criteria of test_vessel_phantom_fused_bounce_against_the_bvh_streams; and on the brute-force scene the rays
    through k_us_emit_init and the path state (PBRT_US_EMIT_FUSED=0): one computation in two instances, by the criterion of
    test_gpu_ultrasound.py::test_specialised_and_generic_bounce_kernels_agree.
    Measured: rel. L2 2.6e-8 for both BVH routes against brute force, far below the 1e-3 this comparison is held to."""
    ctx = mi.default_context()
    bufs, stats = {}, {}
    for name in ("brute", "bvh", "bvh_global"):
        sc, ui = _emitter_vessel_phantom(mi, capi, name, 256, 3)
        assert ui.us_params(sc).primary == capi.US_PRIMARY_EMITTER
        bufs[name] = ui._acquire(sc, ui.quirks)
        stats[name] = ctx.stats()
    buf = bufs["brute"]
    assert buf.shape == (5, 64, 10000) and np.isfinite(buf).all() and (buf != 0).sum() > 1000
    for name in ("bvh", "bvh_global"):
        print(f"\nemitter rays on the vessel phantom, {name} against brute: rel. L2 {_rel_l2(bufs[name], buf):.3g}")
        assert np.isfinite(bufs[name]).all() and np.array_equal(bufs[name] != 0, buf != 0), name
        assert _rel_l2(bufs[name], buf) <= 1e-3, name
    assert stats["bvh"]["bounce_launches"] > 1 and stats["bvh_global"]["bounce_launches"] > 1
    sc, ui = _emitter_vessel_phantom(mi, capi, "brute", 256, 3)
    monkeypatch.setenv("PBRT_US_EMIT_FUSED", "0")
    unfused = ui._acquire(sc, ui.quirks)
    st_u = ctx.stats()
    monkeypatch.delenv("PBRT_US_EMIT_FUSED")
    st = stats["brute"]
    assert (st_u["segments"], st_u["shadow_rays"], st_u["live"]) == (st["segments"], st["shadow_rays"], st["live"]) and st["segments"] > 0
    assert np.array_equal(unfused != 0, buf != 0) and np.allclose(unfused, buf, rtol=2e-5, atol=1e-7 * np.abs(buf).max())


def test_vessel_phantom_emitter_rays_path_sharding_adds_up(mi, capi):
    """a path's emitter ray is a function of its index in the whole acquisition (path_offset + k), not of the call it is drawn in"""
    sc, ui = _emitter_vessel_phantom(mi, capi, "brute", 300, 6)
    full = ui._acquire(sc, ui.quirks, paths_per_ray=300, seed=6)
    a = ui._acquire(sc, ui.quirks, paths_per_ray=100, path_offset=0, norm_paths=300, seed=6)
    b = ui._acquire(sc, ui.quirks, paths_per_ray=200, path_offset=100, norm_paths=300, seed=6)
    assert (full != 0).sum() > 1000
    assert _rel_l2(a + b, full) <= 1e-5 and np.array_equal((a + b) != 0, full != 0)
