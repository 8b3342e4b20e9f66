"""The brute-force kernels walk their primitive lists in runs of one class (csrc/prim_runs.h, device_scene.h brute_intersect):
lists whose runs have length one, run boundaries inside the list, a cone (and a cylinder) between planar runs, 32 and 33
primitives, occluder lists that are shorter than the primitive list or empty.  The closest hit (t, prim, u, v bit for bit) and
the occlusion test of ~4 200 rays per scene -- random ones, rays through corners and edges that primitives of different runs
share (duplicated primitives tie exactly: the lowest index wins), axis-aligned rays, a zero direction, NaN / +-inf components and
operands of magnitude 1e30 -- equal the oracle's, and so do small films and one acquisition.

The oracle has no cylinder, so the list with a cone AND a cylinder is held to the library's BVH kernels and to the float64
restatement of tests/cylinder_util.py instead (test_cone_and_cylinder_between_planar_runs); the same list without the cylinder goes
through the oracle like the others.

What the non-finite rays found: with max(us, vs) <= det as the parallelogram's upper bound a ray with an infinite component was
accepted with a NaN barycentric (max drops the NaN) where the oracle rejects it -- up to 8 closest hits and 8 occlusion answers
of the 96 +-inf rays of a scene, in the parent commit as well.  The bound is us <= det & vs <= det since."""
import numpy as np
import pytest

from conftest import oracle_render, scene_path

pytestmark = pytest.mark.gpu

DIF = {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.7, 0.6, 0.5]}}


def _shapes(mi, tmp_path, spec, seed):
    """{name: shape dict} in the order of spec: Q rectangle, T one-triangle mesh, S sphere, C cone, Y cylinder.  A triangle takes
    three corners of the latest rectangle that has no such twin yet (the same v0, e1, e2: exact ties on its half), a sphere repeats
    the latest sphere that has no twin yet -- twins sit in different runs."""
    rng = np.random.default_rng(seed)
    T = mi.ScalarTransform4f
    out, free_q, free_s = {}, [], []

    def pose(scale):
        return T().translate(list(rng.uniform(-1.2, 1.2, 3))) @ T().rotate(list(rng.normal(size=3)), float(rng.uniform(0, 360))) @ T().scale(scale)

    for k, c in enumerate(spec):
        if c == "Q":
            tw = pose([float(rng.uniform(0.4, 1.0)), float(rng.uniform(0.4, 1.0)), 1.0])
            out[f"q{k}"] = {"type": "rectangle", "to_world": tw, "bsdf": DIF}
            free_q.append(tw)
        elif c == "T":
            if free_q:
                v = free_q.pop().transform_affine(np.array([[-1.0, -1, 0], [1, -1, 0], [-1, 1, 0]]))
            else:
                v = rng.uniform(-1.2, 1.2, (1, 3)) + rng.normal(scale=0.6, size=(3, 3))
            path = tmp_path / f"tri_{seed}_{k}.obj"
            with open(path, "w") as f:
                for p in v:
                    f.write(f"v {p[0]:.17g} {p[1]:.17g} {p[2]:.17g}\n")
                f.write("f 1 2 3\n")
            out[f"t{k}"] = {"type": "obj", "filename": str(path), "bsdf": DIF}
        elif c == "S":
            if free_s:
                ctr, r = free_s.pop()
            else:
                ctr, r = list(rng.uniform(-1.2, 1.2, 3)), float(rng.uniform(0.3, 0.7))
                free_s.append((ctr, r))
            out[f"s{k}"] = {"type": "sphere", "center": ctr, "radius": r, "bsdf": DIF}
        elif c == "C":
            out[f"c{k}"] = {"type": "cone", "to_world": pose([float(rng.uniform(0.3, 0.7)), float(rng.uniform(0.3, 0.7)), float(rng.uniform(0.5, 1.2))]), "bsdf": DIF}
        else:
            out[f"y{k}"] = {"type": "cylinder", "radius": float(rng.uniform(0.2, 0.5)), "p0": list(rng.uniform(-1.2, 1.2, 3)),
                            "p1": list(rng.uniform(-1.2, 1.2, 3)), "bsdf": DIF}
    return out


def _film_parts(mi, light=True):
    T = mi.ScalarTransform4f
    d = {"type": "scene", "integrator": {"type": "path", "max_depth": 6},
         "sensor": {"type": "perspective", "fov": 50, "to_world": T().look_at([0, 0, 5.5], [0, 0, 0], [0, 1, 0]),
                    "film": {"type": "hdrfilm", "width": 16, "height": 16, "rfilter": {"type": "tent"}},
                    "sampler": {"type": "independent", "sample_count": 4}}}
    if light:
        d["light"] = {"type": "rectangle", "to_world": T().translate([0, 2.6, 0]) @ T().rotate([1, 0, 0], 90) @ T().scale([1.2, 1.2, 1]),
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [4, 4, 4]}}, "bsdf": {"type": "diffuse"}}
    return d


def _room(mi, with_ball):
    """five walls, open towards the camera, a point light inside.  with_ball: the convex room of tests/test_oracle_transport.py -- a
    blocker, a ball and a lamp inside, three occluders in three runs beside eight primitives in three.  Without: every primitive lies
    on the convex hull of the scene, n_occ = 0."""
    T = mi.ScalarTransform4f
    d = _film_parts(mi, light=False)
    d["sensor"]["to_world"] = T().look_at([0, 0.2, 3.6], [0, 0, 0], [0, 1, 0])
    d.update({"floor": {"type": "rectangle", "to_world": T().translate([0, -1, 0]).rotate([1, 0, 0], -90), "bsdf": DIF},
              "ceil": {"type": "rectangle", "to_world": T().translate([0, 1, 0]).rotate([1, 0, 0], 90), "bsdf": DIF},
              "back": {"type": "rectangle", "to_world": T().translate([0, 0, -1]), "bsdf": DIF},
              "left": {"type": "rectangle", "to_world": T().translate([-1, 0, 0]).rotate([0, 1, 0], 90), "bsdf": DIF},
              "right": {"type": "rectangle", "to_world": T().translate([1, 0, 0]).rotate([0, 1, 0], -90), "bsdf": DIF}})
    if with_ball:
        d.update({"blocker": {"type": "rectangle", "to_world": T().translate([0.2, -0.3, 0.1]).rotate([0, 1, 0], 30).scale(0.35), "bsdf": DIF},
                  "ball": {"type": "sphere", "center": [-0.4, -0.6, 0.2], "radius": 0.4, "bsdf": DIF},
                  "lamp": {"type": "rectangle", "to_world": T().translate([0, 0.98, 0]).rotate([1, 0, 0], 90).scale(0.3),
                           "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [6, 6, 6]}}}})
    d["bulb"] = {"type": "point", "position": [0.3, 0.2, 0.5], "intensity": {"type": "rgb", "value": [8, 8, 8]}}
    return mi.load_dict(d)


def _mixed(n, seed):
    return "".join(np.random.default_rng(seed).choice(list("QTS"), n))


# name -> the primitive classes of the scene, in list order
LEAF_SCENES = {
    "one_quad": "Q", "one_triangle": "T", "one_sphere": "S",
    "runs_of_one": "TSQTS",
    "boundaries_inside": "QQQSSTT",
    "mixed_32": _mixed(32, 32), "mixed_33": _mixed(33, 33),
    "cone_between_planar_runs": "QQCSTT",
}
WITH_CYLINDER = "QQCYSTT"  # the oracle does not know the cylinder: test_cone_and_cylinder_between_planar_runs
CLASS_OF = {"Q": 2, "T": 0, "S": 1, "C": 3, "Y": 4}  # PBRT_PRIM_*


def _scene(mi, capi, tmp_path, name):
    if name == "room_with_ball":
        return _room(mi, True)
    if name == "room_without_occluder":
        return _room(mi, False)
    spec = LEAF_SCENES.get(name, name)
    d = {"type": "scene"}
    d.update(_shapes(mi, tmp_path, spec, len(spec)))
    sc = mi.load_dict(d)
    if len(spec) > 32:
        sc.accel = capi.ACCEL_BRUTE  # 33 primitives on the brute-force path: the _BIG kernel variant
    assert [int(t) for t in sc.flatten()["prims"]["type"]] == [CLASS_OF[c] for c in spec]
    return sc


def _rays(prims, seed):
    """(o, d, tmax, kind): kind names the family of every ray"""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    fam = []

    def unit(v):
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    n = 2600
    fam.append(("random", rng.uniform(-3, 3, (n, 3)), unit(rng.normal(size=(n, 3)))))
    # corners, edge midpoints and centres of the primitives (spheres: centre and a point of the silhouette)
    g = prims["g"].astype(np.float64)
    pts = []
    for P, ty in zip(g, prims["type"]):
        if ty in (0, 2):
            v0, e1, e2 = P[0:3], P[3:6], P[6:9]
            pts += [v0, v0 + e1, v0 + e2, v0 + 0.5 * e1, v0 + 0.5 * e2, v0 + 0.5 * (e1 + e2), v0 + 0.25 * (e1 + e2)]
            if ty == 2:
                pts += [v0 + e1 + e2, v0 + e1 + 0.5 * e2, v0 + e2 + 0.5 * e1]
        elif ty == 1:
            pts += [P[0:3], P[0:3] + [P[3], 0, 0], P[0:3] + [0, 0, P[3]]]
        else:
            O = np.linalg.inv(np.vstack([P.reshape(3, 4), [0, 0, 0, 1]]))  # object -> world: the base centre and the middle of the axis
            pts += [O[:3, 3], (O @ [0, 0, 0.5, 1])[:3]]
    pts = np.asarray(pts)
    tgt = pts[rng.integers(0, len(pts), 700)]
    o = rng.uniform(-3, 3, (700, 3))
    fam.append(("corners_and_edges", o, unit(tgt - o)))
    # axis-aligned: random origins, and lines through the points above (two coordinates exactly theirs)
    ax = np.eye(3)[rng.integers(0, 3, 300)] * rng.choice([-1.0, 1.0], (300, 1))
    fam.append(("axis_random", rng.uniform(-2, 2, (300, 3)), ax))
    ax = np.eye(3)[rng.integers(0, 3, 300)] * rng.choice([-1.0, 1.0], (300, 1))
    tgt = pts[rng.integers(0, len(pts), 300)].astype(f32).astype(np.float64)
    fam.append(("axis_through_points", tgt - 4.0 * ax, ax))
    # degenerate and non-finite rays
    m = 48
    o, d = rng.uniform(-1, 1, (m, 3)), np.zeros((m, 3))
    fam.append(("zero_direction", o, d))
    for name, val in (("nan", np.nan), ("plus_inf", np.inf), ("minus_inf", -np.inf)):
        o, d = rng.uniform(-2, 2, (m, 3)), unit(rng.normal(size=(m, 3)))
        k = np.arange(m)
        o[k[: m // 2], rng.integers(0, 3, m // 2)] = val                      # first half: in the origin
        d[k[m // 2:], rng.integers(0, 3, m - m // 2)] = val                   # second half: in the direction
        fam.append((name, o, d))
    o, d = rng.uniform(-2, 2, (m, 3)) * 1e30, unit(rng.normal(size=(m, 3)))
    fam.append(("origin_1e30", o, d))
    o, d = rng.uniform(-2, 2, (m, 3)), unit(rng.normal(size=(m, 3))) * 1e30
    fam.append(("direction_1e30", o, d))
    o = rng.uniform(-2, 2, (m, 3)) * 1e30
    fam.append(("both_1e30", o, -o))
    O = np.concatenate([f[1] for f in fam]).astype(f32)
    D = np.concatenate([f[2] for f in fam]).astype(f32)
    kind = np.concatenate([[f[0]] * len(f[1]) for f in fam])
    tmax = np.where(np.arange(len(O)) % 4 == 0, 3.0, np.inf).astype(f32)
    return O, D, tmax, kind


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(LEAF_SCENES) + ["room_with_ball", "room_without_occluder"])
def test_leaf_kernels_equal_the_oracle(mi, ob, capi, tmp_path, name):
    sc = _scene(mi, capi, tmp_path, name)
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
        print(f"{name:22s} {k:20s} rays {sel.sum():5d} hits {int(np.asarray(got['valid'])[sel].sum()):5d} "
              f"closest-hit mismatches {int(bad[sel].sum())} occlusion mismatches {int(bad_occ[sel].sum())}")
    assert not bad.any(), (name, sorted(set(kind[bad])))
    assert not bad_occ.any(), (name, sorted(set(kind[bad_occ])))
    hit = np.asarray(got["valid"])
    assert hit[kind == "corners_and_edges"].mean() > 0.3 and hit.sum() > 300   # the rays do meet the scene


def test_cone_and_cylinder_between_planar_runs(mi, capi, tmp_path):
    """Q Q C Y S T T: one curved run of a cone, a cylinder and a sphere between two planar runs (the _BIG kernel).  The CPU oracle
    has no cylinder, so the references are the library's BVH kernels on the same scene (the same primitive tests, no run tables:
    t and prim bit for bit, as tests/test_gpu_cylinder.py holds the accelerators to) and, for the cylinder itself, the float64
    restatement of tests/cylinder_util.py away from its rims and silhouette.  Finite rays only: a box test culls non-finite ones."""
    import cylinder_util as cu
    sc = _scene(mi, capi, tmp_path, WITH_CYLINDER)
    bvh = _scene(mi, capi, tmp_path, WITH_CYLINDER)
    bvh.accel = capi.ACCEL_BVH
    prims = sc.flatten()["prims"]
    o, d, tmax, kind = _rays(prims, 7)
    finite = np.isin(kind, ["random", "corners_and_edges", "axis_random", "axis_through_points"])
    o, d, tmax = o[finite], d[finite], tmax[finite]
    got, ref = sc.ray_intersect(o, d, tmax), bvh.ray_intersect(o, d, tmax)
    assert np.array_equal(got["prim"], ref["prim"]) and np.array_equal(_bits(got["t"]), _bits(ref["t"]))
    occ = sc.ray_test(o, d, tmax)
    assert np.array_equal(occ, bvh.ray_test(o, d, tmax)) and np.array_equal(occ, got["valid"])
    c = WITH_CYLINDER.index("Y")
    cyl = cu.intersect(cu.record_matrix(prims[c]), o, d, tmax)
    sure = (cyl["margin"] > 1e-4) & (cyl["chord"] > 0.1) & (cyl["gap"] > 0.1)
    on_cyl = got["prim"] == c
    assert on_cyl.sum() > 100 and {2, 3, 4} <= {int(p) for p in got["prim"][got["valid"]]}   # every member of the curved run is met
    assert cyl["valid"][on_cyl & sure].all()                                       # a reported cylinder hit is one
    assert np.allclose(got["t"][on_cyl & sure], cyl["t"][on_cyl & sure], rtol=1e-5, atol=0)
    front = sure & cyl["valid"] & ~on_cyl                                           # a sure cylinder hit not reported: something nearer was
    assert got["valid"][front].all() and np.all(got["t"][front] <= cyl["t"][front] * (1 + 1e-5))


def test_twins_in_different_runs_tie_and_the_lowest_index_wins(mi, ob, capi, tmp_path):
    """runs_of_one is T S Q T S: triangle 3 is one half of rectangle 2 and sphere 4 is sphere 1 again -- the same candidate from two
    runs, and the first one is reported"""
    sc = _scene(mi, capi, tmp_path, "runs_of_one")
    g = sc.flatten()["prims"]["g"].astype(np.float64)
    inside = g[2, 0:3] + 0.2 * g[2, 3:6] + 0.3 * g[2, 6:9]          # in the rectangle's half that the triangle covers
    nrm = np.cross(g[2, 3:6], g[2, 6:9])
    nrm /= np.linalg.norm(nrm)
    o = np.stack([inside + 1e-3 * nrm, g[1, 0:3] + [0, 0, 0.1 * g[1, 3]]]).astype(np.float32)   # just above the rectangle; inside the sphere
    d = np.stack([-nrm, [0, 0, 1.0]]).astype(np.float32)
    got = sc.ray_intersect(o, d)
    t, prim, u, v = ob.OracleScene.from_scene(sc).ray_intersect(o, d, np.full(2, np.inf, np.float32))
    assert list(got["prim"]) == [2, 1] and np.array_equal(got["prim"], prim) and np.array_equal(_bits(got["t"]), _bits(t))


FILMS = ["cbox", "runs_of_one_lit", "room_with_ball", "room_with_ball_unpruned", "room_without_occluder"]


@pytest.mark.parametrize("name", FILMS)
def test_films_equal_the_oracle(mi, ob, capi, tmp_path, name):
    flags = 0
    if name == "cbox":
        sc = mi.load_file(scene_path("cbox.xml"), res=16, spp=4, max_depth=6)
    elif name == "runs_of_one_lit":
        d = _film_parts(mi)
        d.update(_shapes(mi, tmp_path, "TSQTS", 5))
        sc = mi.load_dict(d)
        assert [int(t) for t in sc.flatten()["prims"]["type"]] == [2, 0, 1, 2, 0, 1]  # the light first: still runs of one
    else:
        sc = _room(mi, name != "room_without_occluder")
        flags = capi.FILM_NO_OCCLUDER_PRUNING if name.endswith("unpruned") else 0
    integ = sc.integrator()
    assert integ.max_depth == 6
    for seed in (0, 1):
        img = integ.render(sc, seed=seed, spp=4, flags=flags)
        ref, _ = oracle_render(ob, sc, seed, 4, flags=flags)
        assert img.shape == ref.shape == (16, 16, 3)
        assert np.array_equal(img, ref) and img.mean() > 0, (name, seed)


def test_acquisition_of_the_sphere_box_phantom(mi, ob):
    from test_gpu_ultrasound import check, oracle
    sc = mi.load_file(scene_path("us_sphere_box.xml"), paths_per_ray=64, seed=0)
    ui = sc.integrator()
    ui.simulate_acquisition_parallel(sc)
    ref, tx, tol = oracle(ob, sc, ui.us_params(sc), 0, 64)
    check(ui.channel_buf, ref, tol)
    assert np.array_equal(ui.transmission_delays_buf, tx) and (ref != 0).sum() > 100
