"""The 'cylinder' shape on the host: the PRIM_CYLINDER record scene.py builds from p0 / p1 / radius / to_world /
flip_normals, its XML form, the orientation encoding as Scene._surface reads it, and the refusals.  No GPU: the records are
checked against the float64 restatement of tests/cylinder_util.py."""
import os

import numpy as np
import pytest

import cylinder_util as cu


def _scene(mi, **cyl):
    return mi.load_dict({"type": "scene", "c": {"type": "cylinder", **cyl}})


def _record(mi, **cyl):
    P = _scene(mi, **cyl).flatten()["prims"]
    assert len(P) == 1
    return P[0]


def _to_world(mi):
    """rotated, non-uniformly scaled, translated (right-handed)"""
    T = mi.ScalarTransform4f
    return T().translate([0.3, -0.2, 0.5]) @ T().rotate([1, 2, 0.5], 37.0) @ T().scale([1.3, 0.8, 1.1])


def test_defaults_are_the_unit_tube(mi, capi):
    rec = _record(mi)
    assert rec["type"] == capi.PRIM_CYLINDER == 4
    assert np.array_equal(cu.record_matrix(rec), np.eye(3, 4))
    assert rec["emitter"] == -1


@pytest.mark.parametrize("case", ["defaults_to_world", "p0_p1_radius", "all"])
def test_surface_points_map_to_the_unit_tube(mi, case):
    kw, tw = {}, None
    if case in ("p0_p1_radius", "all"):
        kw = dict(p0=[0.1, -0.4, 0.2], p1=[-0.3, 0.5, 0.9], radius=0.35)
    if case in ("defaults_to_world", "all"):
        tw = _to_world(mi)
        kw["to_world"] = tw
    W = cu.record_matrix(_record(mi, **kw))
    O = cu.object_to_world(**{k: v for k, v in kw.items() if k != "to_world"}, to_world=None if tw is None else tw.matrix)
    rng = np.random.default_rng(3)
    phi, s = rng.uniform(0, 2 * np.pi, 500), rng.uniform(0, 1, 500)
    pw = cu.surface_points(O, phi, s)
    q = pw @ W[:, :3].T + W[:, 3]
    assert np.abs(q[:, 0] ** 2 + q[:, 1] ** 2 - 1.0).max() < 1e-6
    assert np.abs(q[:, 2] - s).max() < 1e-6
    # the end-disc centres: p0 -> (0, 0, 0), p1 -> (0, 0, 1)
    ends = cu.surface_points(O, np.zeros(2), np.array([0.0, 1.0])) - (O[:3, 0])[None, :]
    qe = ends @ W[:, :3].T + W[:, 3]
    assert np.allclose(qe, [[0, 0, 0], [0, 0, 1]], atol=1e-6)
    assert np.linalg.det(W[:, :3]) > 0           # outward normals (flip_normals unset)


def test_xml_form_gives_the_dict_record(mi, tmp_path):
    xml = """<scene version="3.0.0">
    <shape type="cylinder" id="c">
        <point name="p0" x="0.1" y="-0.4" z="0.2"/>
        <point name="p1" value="-0.3, 0.5, 0.9"/>
        <float name="radius" value="0.35"/>
        <boolean name="flip_normals" value="true"/>
        <transform name="to_world"><scale x="1.3" y="0.8" z="1.1"/><rotate x="1" y="2" z="0.5" angle="37"/><translate x="0.3" y="-0.2" z="0.5"/></transform>
    </shape>
</scene>"""
    path = os.path.join(tmp_path, "cyl.xml")
    with open(path, "w") as f:
        f.write(xml)
    a = mi.load_file(path).flatten()["prims"]
    b = _scene(mi, p0=[0.1, -0.4, 0.2], p1=[-0.3, 0.5, 0.9], radius=0.35, flip_normals=True, to_world=_to_world(mi)).flatten()["prims"]
    assert np.array_equal(a["type"], b["type"]) and np.allclose(a["g"], b["g"], rtol=0, atol=1e-6)


@pytest.mark.parametrize("mirrored", [False, True])
def test_flip_normals_encoding_through_surface(mi, capi, mirrored):
    """flip_normals is the sign of det(M) (object x mirrored where needed): _surface's normal points away from the axis without it
    and towards it with it, whatever the handedness of to_world; the hit point is o + t d"""
    T = mi.ScalarTransform4f
    tw = _to_world(mi) @ (T().scale([-1, 1, 1]) if mirrored else T())
    kw = dict(p0=[0.0, 0.0, -0.5], p1=[0.0, 0.2, 0.6], radius=0.4, to_world=tw)
    O = cu.object_to_world(kw["p0"], kw["p1"], kw["radius"], tw.matrix)
    rng = np.random.default_rng(7)
    phi, s = rng.uniform(0, 2 * np.pi, 64), rng.uniform(0.1, 0.9, 64)
    target = cu.surface_points(O, phi, s)
    centre = (np.c_[np.zeros((64, 2)), s, np.ones(64)] @ O.T)[:, :3]      # the axis point at the same height
    o = centre + 3.0 * (target - centre)                                      # outside, aimed at the axis through `target`
    d = (target - o) / np.linalg.norm(target - o, axis=1, keepdims=True)
    out = {}
    for flip in (False, True):
        sc = _scene(mi, flip_normals=flip, **kw)
        W = cu.record_matrix(sc.flatten()["prims"][0])
        assert (np.linalg.det(W[:, :3]) < 0) == flip
        ref = cu.intersect(W, o, d)
        assert ref["valid"].all() and np.allclose(ref["p"], target, atol=1e-5)
        n = len(o)
        srf = sc._surface(o.astype(np.float32), d.astype(np.float32), ref["t"].astype(np.float32), np.zeros(n, np.uint32),
                          np.zeros(n, np.float32), np.zeros(n, np.float32), np.ones(n, bool))
        assert np.allclose(srf["p"], target, atol=1e-5) and np.all(srf["shape"] == 0)
        assert np.allclose(srf["n"], ref["n"], atol=1e-5)
        radial = target - centre
        side = np.einsum("ij,ij->i", srf["n"], radial)
        assert np.all(side < 0) if flip else np.all(side > 0)
        out[flip] = srf["n"]
    assert np.allclose(out[True], -out[False], atol=1e-6)


@pytest.mark.parametrize("bad", [dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")),
                                 dict(p0=[0.2, 0.3, 0.4], p1=[0.2, 0.3, 0.4]), dict(p1=[0.0, float("nan"), 1.0]),
                                 "singular", "singular_rank2"])
def test_invalid_cylinders_are_refused(mi, bad):
    T = mi.ScalarTransform4f
    if bad == "singular":
        bad = dict(to_world=T().scale([1.0, 0.0, 1.0]))
    elif bad == "singular_rank2":
        bad = dict(to_world=T(np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [1.0, 1.0, 0, 0], [0, 0, 0, 1.0]])))
    with pytest.raises(ValueError, match="cylinder"):
        _scene(mi, **bad)


def test_area_emitter_on_a_cylinder_is_refused(mi):
    sc = _scene(mi, emitter={"type": "area", "radiance": {"type": "rgb", "value": [1.0, 1.0, 1.0]}})
    with pytest.raises(NotImplementedError, match="cylinder"):
        sc.flatten()


def test_vessel_phantom_loads(mi, capi):
    from conftest import scene_path
    sc = mi.load_file(scene_path("us_vessel_box.xml"))
    P = sc.flatten()["prims"]
    cyl = P[P["type"] == capi.PRIM_CYLINDER]
    assert len(cyl) == 2 and np.sum(P["type"] == capi.PRIM_PARALLELOGRAM) == 5
    for rec in cyl:
        assert np.linalg.det(cu.record_matrix(rec)[:, :3]) > 0
