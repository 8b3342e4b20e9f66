"""A brute-force scene whose two primitive lists are class-ordered (parallelograms, then triangles, then curved records:
csrc/prim_runs.h prim_runs_ordered) is walked by three loops over three counts, without the run tables (device_scene.h
brute_intersect ORDERED): the four k_bounce<FIRST, ACCEL_K_BRUTE_ORDERED, NB> instances and, by a uniform branch, the leaf kernels.
Same loops, same indices, same list order, so the results are those of the table walk for every input:

* leaf kernels: closest hit (t, prim, u, v bit for bit) and occlusion of ~4 300 rays per scene -- the ray families of
  tests/test_gpu_typed_runs.py, zero, NaN, +-inf and 1e30 rays among them -- equal the oracle's on Q, S, QS, QQQSS, QTS, TTS and a
  32-primitive Q..T..S.. list in which every triangle is one half of a rectangle (exact ties across the step from the parallelogram
  loop into the triangle loop; the first in list order wins) and spheres repeat (ties inside the one curved loop);
* films of 16 x 16 pixels at 4 spp, max_depth 6: the film is the oracle's bit for bit, segments and shadow rays are the oracle's (it
  counts no live paths per depth: those are held to the table walk), and film, segments, shadow rays and live paths are those of
  the same render through the table-walk instances (PBRT_FILM_NO_ORDERED_WALK) -- plain, as one launch per pass, as pairs, as one
  launch per bounce (together the four instances), each chain with and without keep words and with the primitive list in place of
  the occluder list, on a region of 256 pixels (keep words) and on one of a pixel count that is no multiple of 64 (none);
* a list that is not ordered (Q S Q) takes the table walk with and without the flag."""
import numpy as np
import pytest

from conftest import oracle_render, scene_path
from test_gpu_typed_runs import CLASS_OF, _bits, _film_parts, _rays, _room, _scene, _shapes

pytestmark = pytest.mark.gpu

Q32 = "Q" * 11 + "T" * 11 + "S" * 10
LEAF_SPECS = ["Q", "S", "QS", "QQQSS", "QTS", "TTS", Q32]
RUN_CLASS = {2: 0, 0: 1, 1: 2, 3: 2, 4: 2}  # PBRT_PRIM_* -> PRIM_RUN_*


def _ordered(sc):
    cls = [RUN_CLASS[int(t)] for t in sc.flatten()["prims"]["type"]]
    return cls == sorted(cls)


@pytest.mark.parametrize("spec", LEAF_SPECS, ids=[s if len(s) < 8 else "Q11_T11_S10" for s in LEAF_SPECS])
def test_leaf_kernels_equal_the_oracle(mi, ob, capi, tmp_path, spec):
    sc = _scene(mi, capi, tmp_path, spec)
    assert _ordered(sc) and len(sc.flatten()["prims"]) == len(spec) <= 32
    prims = sc.flatten()["prims"]
    o, d, tmax, kind = _rays(prims, 7)
    assert 4000 <= len(o) <= 4300
    osc = ob.OracleScene.from_scene(sc)
    got = sc.ray_intersect(o, d, tmax)
    t, prim, u, v = osc.ray_intersect(o, d, tmax)
    occ, occ_ref = sc.ray_test(o, d, tmax), osc.ray_test(o, d, tmax)
    bad = (got["prim"] != prim) | (_bits(got["t"]) != _bits(t)) | (_bits(got["u"]) != _bits(u)) | (_bits(got["v"]) != _bits(v))
    bad_occ = np.asarray(occ) != np.asarray(occ_ref)
    for k in dict.fromkeys(kind):
        sel = kind == k
        print(f"{spec:34s} {k:20s} rays {sel.sum():5d} hits {int(np.asarray(got['valid'])[sel].sum()):5d} "
              f"closest-hit mismatches {int(bad[sel].sum())} occlusion mismatches {int(bad_occ[sel].sum())}")
    assert not bad.any(), (spec, sorted(set(kind[bad])))
    assert not bad_occ.any(), (spec, sorted(set(kind[bad_occ])))
    hit = np.asarray(got["valid"])
    assert hit.sum() > 50  # the rays do meet the scene


def test_ties_across_the_loops_go_to_the_first_in_list_order(mi, ob, capi, tmp_path):
    """Q T S: the triangle is one half of the rectangle -- the same candidate from the parallelogram loop and from the triangle
    loop; Q Q Q S S: the second sphere is the first again.  The first one is reported."""
    sc = _scene(mi, capi, tmp_path, "QTS")
    g = sc.flatten()["prims"]["g"].astype(np.float64)
    assert np.allclose(g[0, :9], g[1, :9], rtol=0, atol=1e-6)
    inside = g[0, 0:3] + 0.2 * g[0, 3:6] + 0.3 * g[0, 6:9]  # in the half of the rectangle that the triangle covers
    nrm = np.cross(g[0, 3:6], g[0, 6:9])
    nrm /= np.linalg.norm(nrm)
    o = np.stack([inside + 1e-3 * nrm, inside - 1e-3 * nrm]).astype(np.float32)
    d = np.stack([-nrm, nrm]).astype(np.float32)
    got = sc.ray_intersect(o, d)
    t, prim, u, v = ob.OracleScene.from_scene(sc).ray_intersect(o, d, np.full(2, np.inf, np.float32))
    assert list(got["prim"]) == [0, 0] and np.array_equal(got["prim"], prim) and np.array_equal(_bits(got["t"]), _bits(t))

    sc = _scene(mi, capi, tmp_path, "QQQSS")
    g = sc.flatten()["prims"]["g"].astype(np.float64)
    assert np.array_equal(g[3, :4], g[4, :4])  # the same centre and radius
    o = (g[3, 0:3] + [0, 0, 0.1 * g[3, 3]])[None].astype(np.float32)  # inside the sphere
    d = np.array([[0, 0, 1.0]], np.float32)
    got = sc.ray_intersect(o, d)
    t, prim, u, v = ob.OracleScene.from_scene(sc).ray_intersect(o, d, np.full(1, np.inf, np.float32))
    assert list(got["prim"]) == [3] and np.array_equal(got["prim"], prim) and np.array_equal(_bits(got["t"]), _bits(t))


def _film_scene(mi, tmp_path, name):
    if name == "cbox":
        return mi.load_file(scene_path("cbox.xml"), res=16, spp=4, max_depth=6)
    if name == "room_on_the_hull":
        return _room(mi, False)  # five walls and a point light: every primitive on the convex hull, n_occ = 0
    spec = {"lit_QQS": "QQS", "lit_QTS": "QTS", "lit_SQ": "SQ"}[name]
    d = _film_parts(mi)  # the light, a rectangle, comes first in the list
    d.update(_shapes(mi, tmp_path, spec, len(spec)))
    sc = mi.load_dict(d)
    assert [int(t) for t in sc.flatten()["prims"]["type"]] == [2] + [CLASS_OF[c] for c in spec]
    return sc


def _flag_sets(capi):
    one, pairs, each = capi.film_fuse_plan(0x1F), capi.film_fuse_plan(0x15), capi.film_fuse_plan(0)
    cull, occ = capi.FILM_NO_TILE_CULL, capi.FILM_NO_OCCLUDER_PRUNING
    return {"plain": 0, "plain_no_cull": cull, "plain_unpruned": occ,
            "one_launch": one, "one_launch_no_cull": one | cull, "one_launch_unpruned": one | occ,
            "pairs": pairs, "pairs_no_cull": pairs | cull, "pairs_unpruned": pairs | occ,
            "launch_per_bounce": each, "launch_per_bounce_no_cull": each | cull, "launch_per_bounce_unpruned": each | occ}


CROP = (2, 3, 9, 5)  # with its filter border a region of no multiple of 64 pixels whatever the filter's radius (0, 1 or 2)


def _check_films(mi, ob, capi, sc, seed, name):
    integ, ctx = sc.integrator(), mi.default_context()
    assert integ.max_depth == 6
    small = len(sc.flatten()["prims"]) <= 32
    for crop in (None, CROP):
        refs = {}
        for what, flags in _flag_sets(capi).items():
            img = integ.render(sc, seed=seed, spp=4, crop=crop, flags=flags)
            st = ctx.stats()
            keep = ctx.tile_keep()["used"]
            assert keep == (small and crop is None and not flags & capi.FILM_NO_TILE_CULL), (name, what, crop)
            tab = integ.render(sc, seed=seed, spp=4, crop=crop, flags=flags | capi.FILM_NO_ORDERED_WALK)
            st_tab = ctx.stats()
            pruning = flags & capi.FILM_NO_OCCLUDER_PRUNING
            if pruning not in refs:
                refs[pruning] = oracle_render(ob, sc, seed, 4, crop=crop, flags=pruning)
            ref, ost = refs[pruning]
            assert img.shape == ref.shape == ((16, 16, 3) if crop is None else (CROP[3], CROP[2], 3))
            assert np.array_equal(img, ref) and (crop is not None or img.mean() > 0), (name, seed, what, crop)  # (a crop may be black)
            assert np.array_equal(img, tab), (name, seed, what, crop)
            assert (st["segments"], st["shadow_rays"], list(st["live"])) == (st_tab["segments"], st_tab["shadow_rays"], list(st_tab["live"])), (name, what)
            assert st["live"][0] > 0
            if crop is None:  # (the oracle counts the paths of the crop, the library those of the region its filter reads)
                assert (st["segments"], st["shadow_rays"]) == (ost["segments"], ost["shadow_rays"]), (name, what)
                assert st["live"][0] == 16 * 16 * 4


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("name", ["cbox", "lit_QQS", "room_on_the_hull", "lit_QTS"])
def test_films_of_ordered_scenes(mi, ob, capi, tmp_path, name, seed):
    sc = _film_scene(mi, tmp_path, name)
    assert _ordered(sc)
    _check_films(mi, ob, capi, sc, seed, name)


def test_a_list_that_is_not_ordered_takes_the_table_walk_either_way(mi, ob, capi, tmp_path):
    sc = _film_scene(mi, tmp_path, "lit_SQ")  # Q S Q
    assert not _ordered(sc)
    _check_films(mi, ob, capi, sc, 0, "lit_SQ")
