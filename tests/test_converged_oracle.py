"""K13 on the CPU: the oracle's films of the four K13 scenes against the fixtures of the independent float64
estimator (tests/converged_util.py, tests/golden/k13_<scene>.npz), under the three criteria of converged_util.compare.  The oracle
shares its leaf arithmetic with the kernels statement for statement, so what fails here fails on the device and the other way round;
tests/test_gpu_converged.py asks the device itself at a larger budget.  Seeds 0 .. 15, 1024 samples per pixel each (1 M paths)."""
import numpy as np
import pytest

import converged_util as cu
from conftest import oracle_render

SEEDS, SPP = range(16), 1024


def oracle_films(mi, ob, sc):
    s = mi.load_dict(cu.to_mitsuba_dict(sc, mi))
    return s, np.stack([oracle_render(ob, s, seed, SPP)[0] for seed in SEEDS])


@pytest.mark.parametrize("name", cu.SCENES)
def test_oracle_film_converges_to_the_estimator(mi, ob, capi, name):
    f = cu.load_fixture(name)
    s, films = oracle_films(mi, ob, f["scene"])
    if name == "meshlight_glass":   # the mesh light stays three triangles: the triangle branch of sample_emitter is what this scene pins
        fl = s.flatten()
        mesh = [e for e in fl["emitters"] if e["count"] == 3]
        assert len(fl["emitters"]) == 2 and len(mesh) == 1
        lp = fl["light_prims"][mesh[0]["first"]:mesh[0]["first"] + 3]
        assert np.all(fl["prims"]["type"][lp] == capi.PRIM_TRIANGLE)
    r = cu.compare(films, f["batches"], stride=2 if f["scene"]["film"]["filter"] == "tent" else 1)
    cu.report(f"oracle {name}", r)
    assert r["ok"] == (True, True, True)


def test_oracle_with_a_shorter_depth_budget_is_caught(mi, ob):
    """negative control: `box` rendered with max_depth 3 instead of 6 must miss the film-mean criterion by more than 5 standard errors"""
    f = cu.load_fixture("box")
    sc = dict(f["scene"], integrator={"type": "path", "max_depth": 3, "rr_depth": 3})
    _, films = oracle_films(mi, ob, sc)
    r = cu.compare(films, f["batches"])
    cu.report("oracle box, max_depth 3", r)
    assert not r["ok"][2] and np.all(r["z_mean"] < -5)
