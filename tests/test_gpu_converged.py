"""K13 on the DEVICE: films rendered through libpbrt_hip.so against the fixtures of the independent float64
estimator (tests/converged_util.py, tests/golden/k13_<scene>.npz), under the three criteria of converged_util.compare.  Nothing
under oracle/ is imported: the check needs the .npz fixtures and the package only.  Per case seeds 0 .. 31 at 4096 samples per pixel
on the 8 x 8 film: 32 renders of 262 144 paths.  The seeds were fixed before anything was rendered; they are not to be changed to make
a case pass."""
import copy

import numpy as np
import pytest

import converged_util as cu

pytestmark = pytest.mark.gpu

SEEDS, SPP = range(32), 4096
POWER = 1.5e-3    # combined relative standard error of the film mean: with |z| <= 4 any bias of the film mean is below 0.6 %


def device_films(mi, capi, sc, accel):
    s = mi.load_dict(cu.to_mitsuba_dict(sc, mi))
    s.accel = {"brute": capi.ACCEL_BRUTE, "bvh": capi.ACCEL_BVH, "bvh_global": capi.ACCEL_BVH_GLOBAL}[accel]
    films = np.stack([mi.render(s, seed=seed, spp=SPP) for seed in SEEDS])
    assert films.shape == (len(SEEDS), 8, 8, 3) and np.isfinite(films).all()
    return s, films


@pytest.mark.parametrize("accel", ["brute", "bvh", "bvh_global"])
@pytest.mark.parametrize("name", cu.SCENES)
def test_device_film_converges_to_the_estimator(mi, capi, name, accel):
    """brute: the k_bounce chain; bvh / bvh_global: k_trace + k_shade on the tree in LDS and in global memory"""
    f = cu.load_fixture(name)
    s, films = device_films(mi, capi, f["scene"], accel)
    if name == "meshlight_glass":   # the mesh light stays three triangles: the triangle branch of sample_emitter is what this scene pins
        fl = s.flatten()
        mesh = [e for e in fl["emitters"] if e["count"] == 3]
        assert len(fl["emitters"]) == 2 and len(mesh) == 1
        lp = fl["light_prims"][mesh[0]["first"]:mesh[0]["first"] + 3]
        assert np.all(fl["prims"]["type"][lp] == capi.PRIM_TRIANGLE)
    r = cu.compare(films, f["batches"], stride=2 if f["scene"]["film"]["filter"] == "tent" else 1)
    cu.report(f"device {name} {accel}", r)
    assert np.all(r["mean_rel_se"] <= POWER)
    assert r["ok"] == (True, True, True)


def test_device_with_a_shorter_depth_budget_is_caught(mi, capi):
    """negative control: `box` rendered with max_depth 5 instead of 6 (the film mean drops by 0.6 .. 1.2 %) must miss the film-mean
    criterion by more than 5 standard errors"""
    f = cu.load_fixture("box")
    sc = dict(f["scene"], integrator={"type": "path", "max_depth": 5, "rr_depth": 3})
    _, films = device_films(mi, capi, sc, "brute")
    r = cu.compare(films, f["batches"])
    cu.report("device box, max_depth 5", r)
    assert np.all(r["mean_rel_se"] <= POWER)
    assert not r["ok"][2] and np.abs(r["z_mean"]).max() > 5 and np.all(r["z_mean"] < 0)


def test_device_with_a_brighter_dim_light_is_caught(mi, capi):
    """negative control: the radiance of `lamp2`, the dim light of `box`, times 1.05.  By the estimator (the light switched off, 8 x 1024
    samples per pixel) it carries 16 / 29 / 49 % of the film mean in r / g / b, so the film mean moves by +0.8 / +1.4 / +2.4 %: green
    and blue, which move by more than 1 %, must each miss the film-mean criterion by more than 5 standard errors."""
    f = cu.load_fixture("box")
    sc = copy.deepcopy(f["scene"])
    lamp2 = [r for r in sc["rectangles"] if r["name"] == "lamp2"][0]
    lamp2["radiance"] = [1.05 * v for v in lamp2["radiance"]]
    _, films = device_films(mi, capi, sc, "brute")
    r = cu.compare(films, f["batches"])
    cu.report("device box, lamp2 x 1.05", r)
    assert np.all(r["mean_rel_se"] <= POWER)
    assert not r["ok"][2] and np.all(r["z_mean"][1:] > 5)
