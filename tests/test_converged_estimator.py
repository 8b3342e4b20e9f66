"""K13, the reference by itself: the independent float64 estimator of tests/converged_util.py meets two closed
forms, and the two halves of every committed fixture meet the three criteria against each other.  CPU only, no oracle, no device."""
import json
import math

import numpy as np
import pytest

import converged_util as cu

T, R, S = cu._translate, cu._rotate, cu._scale
CAMERA = {"up": [0, 1, 0], "near": 1e-3, "far": 100.0}


def test_estimator_white_furnace():
    """The furnace of test_gpu_analytic.py: a closed box of albedo rho whose six walls emit Le, depth budget D: every pixel carries
    Le (1 + rho + ... + rho^(D-1)).  Here the emission is seen at the camera vertex and every later term is a next-event sample to each
    of the six walls, so the film is noisy; tolerance: five of its own standard errors, and 0.2 %."""
    rho, Le, D = 0.5, 0.75, 5
    walls = {"zp": [T([0, 0, 1]), R("y", 180)], "zn": [T([0, 0, -1])], "xp": [T([1, 0, 0]), R("y", -90)], "xn": [T([-1, 0, 0]), R("y", 90)],
             "yp": [T([0, 1, 0]), R("x", 90)], "yn": [T([0, -1, 0]), R("x", -90)]}
    sc = {"integrator": {"type": "path", "max_depth": D, "rr_depth": 100}, "film": {"width": 8, "height": 8, "filter": "box"},
          "camera": dict(CAMERA, origin=[0, 0, 0], target=[0.3, 0.2, 1], fov=40.0),
          "materials": {"w": {"type": "diffuse", "rgb": [rho] * 3}},
          "rectangles": [cu._rect(k, c, "w", [Le] * 3) for k, c in walls.items()], "meshes": [], "spheres": [], "points": []}
    for r in sc["rectangles"]:   # all normals face the centre
        c = np.asarray(r["p0"]) + 0.5 * np.asarray(r["e1"]) + 0.5 * np.asarray(r["e2"])
        assert np.dot(np.cross(r["e1"], r["e2"]), -c) > 0
    films = cu.render_batches(sc, 16, 512, seed=11)   # 0.5 M paths: a standard error near 0.1 %
    want = Le * sum(rho ** k for k in range(D))
    m = films.mean(axis=(1, 2, 3))
    got, se = m.mean(), m.std(ddof=1) / math.sqrt(len(m))
    print(f"furnace: {got:.6f} against {want:.6f}, {100 * (got / want - 1):+.4f} %, standard error {100 * se / want:.4f} %")
    assert abs(got - want) <= 5 * se and abs(got - want) <= 2e-3 * want
    # a budget of one hit is the emission itself, exactly
    assert np.array_equal(cu.render_batches(sc, 1, 2, seed=3, max_depth=1), np.full((1, 8, 8, 3), Le))


def test_estimator_direct_illumination_form_factor():
    """The direct-illumination scene of test_gpu_analytic.py: a diffuse floor under a small square light of half-side a at height h.
    At the point below its centre the irradiance is exactly  E = Le * 4 * a / s * atan(a / s),  s = sqrt(a^2 + h^2)  (four corner
    rectangles), L = rho / pi * E.  The centre pixel's footprint (about 0.005 wide) changes E by 2 (x / h)^2 < 1e-5 relative."""
    rho, Le, h, a = 0.8, 50.0, 2.0, 0.05
    sc = {"integrator": {"type": "direct"}, "film": {"width": 9, "height": 9, "filter": "box"},
          "camera": {"origin": [2.0, 3.0, 0.0], "target": [0, 0, 0], "up": [0, 0, 1], "fov": 0.5, "near": 1e-3, "far": 100.0},
          "materials": {"floor": {"type": "diffuse", "rgb": [rho] * 3}, "black": {"type": "diffuse", "rgb": [0.0] * 3}},
          "rectangles": [cu._rect("floor", [R("x", -90), S(10)], "floor"),
                         cu._rect("lamp", [T([0, h, 0]), R("x", 90), S(a)], "black", [Le] * 3)],
          "meshes": [], "spheres": [], "points": []}
    films = cu.render_batches(sc, 16, 256, seed=12)
    s = math.hypot(a, h)
    want = rho / math.pi * Le * 4 * a / s * math.atan(a / s)
    small = rho / math.pi * Le * (2 * a) ** 2 / (h * h)
    assert abs(small / want - 1) < 2e-3      # the small-source value of the older tests, as they say
    m = films[:, 4, 4, :].mean(axis=1)
    got, se = m.mean(), m.std(ddof=1) / math.sqrt(len(m))
    print(f"form factor: {got:.8f} against {want:.8f}, {100 * (got / want - 1):+.5f} %, standard error {100 * se / want:.5f} %")
    assert abs(got - want) <= 5 * se + 1e-5 * want and abs(got - want) <= 2e-3 * want


def test_estimator_and_device_test_stand_without_the_build():
    """converged_util imports numpy and the standard library only (scipy for one quantile, if present); tests/test_gpu_converged.py
    imports nothing of oracle/ and not the conftest helpers that render with it"""
    import ast
    allowed = {"json", "math", "os", "numpy", "scipy", "statistics"}
    for fn, ok in (("converged_util.py", lambda m: m in allowed), ("test_gpu_converged.py", lambda m: m not in ("oracle", "conftest"))):
        with open(cu.os.path.join(cu.HERE, fn)) as fh:
            for node in ast.walk(ast.parse(fh.read())):
                if isinstance(node, ast.Import):
                    assert all(ok(a.name.split(".")[0]) for a in node.names), fn
                elif isinstance(node, ast.ImportFrom):
                    assert ok((node.module or "").split(".")[0]), fn


def test_trilight_asset_is_the_estimators_mesh():
    tri = cu.read_obj_triangles(cu.os.path.join(cu.MESHES, cu.TRILIGHT_OBJ))
    assert np.array_equal(tri, np.asarray(cu.TRILIGHT))
    cs = cu._Compiled(cu.scene("meshlight_glass"))
    mesh = [lt for lt in cs.lights if lt["kind"] == "area" and len(lt["prims"]) == 3]
    assert len(mesh) == 1
    a = cs.area[mesh[0]["prims"]]
    assert np.allclose(a / a[0], [1, 2, 4], rtol=0.05) and a.sum() >= 1.0   # a quarter of the 2 x 2 ceiling
    assert np.allclose(cs.N[mesh[0]["prims"]], [0, -1, 0])


@pytest.mark.parametrize("name", cu.SCENES)
def test_fixture_meets_the_budget_and_agrees_with_itself(name):
    """A fixture holds what make_converged.py wrote for the scene of today's converged_util.scene(); its film mean has a relative
    standard error <= 0.1 % per channel (the budget condition, recomputed from the batches), and its first and second half of the
    batches meet the three criteria against each other."""
    f = cu.load_fixture(name)
    assert f["scene"] == json.loads(json.dumps(cu.scene(name)))
    b = f["batches"]
    assert b.dtype == np.float64 and b.shape == (16, 8, 8, 3) and np.isfinite(b).all() and b.min() >= 0
    rel = cu.film_mean_rel_se(b)
    print(f"{name}: {len(b)} x {f['spp']} spp, {f['seconds']:.0f} s, film mean rel. standard error % {100 * rel}")
    assert np.allclose(rel, f["rel_se"]) and np.all(rel <= 1e-3)
    r = cu.compare(b[:len(b) // 2], b[len(b) // 2:], stride=2 if f["scene"]["film"]["filter"] == "tent" else 1)
    cu.report(f"{name} halves", r)
    assert r["ok"] == (True, True, True)
