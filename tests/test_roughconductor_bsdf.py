"""Rough and Fresnel conductors without a GPU: the loaders, the refusals, and self-checks of the float64
restatement (tests/roughconductor_util.py) that the device tests are held against."""
import os

import numpy as np
import pytest

import roughconductor_util as ru

METAL_ETA, METAL_K = [0.2, 0.9, 1.1], [3.9, 2.4, 2.2]  # a coloured metal (gold-like in rgb)


def prototype_dict(mi):
    """the scene dict of the reference's first prototype, literally (a cylinder whose only BSDF is a GGX rough conductor)"""
    return {
        'type': 'scene',
        'integrator': {
            'type': 'path'
        },
        'cylinder': {
            'type': 'cylinder',
            'radius': 0.2,
            'p0': [0, -0.5, 0],
            'p1': [0, 0.5, 0],
            'bsdf': {
                'type': 'roughconductor',
                'alpha': 0.1,
                'distribution': 'ggx'
            }
        },
        'sensor': {
            'type': 'perspective',
            'to_world': mi.ScalarTransform4f().look_at(origin=[0, 0, 2], target=[0, 0, 0], up=[0, 1, 0]),
            'film': {
                'type': 'hdrfilm',
                'width': 64,
                'height': 64,
                'rfilter': {'type': 'box'}
            },
            'sampler': {
                'type': 'independent',
                'sample_count': 16
            }
        }
    }


# ---- loaders --------------------------------------------------------------------------------------------------------------------
def test_prototype_scene_dict_loads_and_flattens(mi, capi):
    sc = mi.load_dict(prototype_dict(mi))
    f = sc.flatten()
    assert len(f["prims"]) == 1 and f["prims"]["type"][0] == capi.PRIM_CYLINDER
    assert len(f["materials"]) == 1 and f["materials"]["type"][0] == capi.MAT_ROUGHCONDUCTOR == 5
    assert np.array_equal(f["materials"]["p"][0], np.array([0.1, 0, 0, 0, 1, 1, 1], np.float32))
    b = f["material_objects"][0]
    assert isinstance(b, mi.RoughConductorBSDF) and b.alpha == 0.1


def _bsdf(mi, **kw):
    return mi.load_dict({"type": "scene", "s": {"type": "sphere", "bsdf": kw}}).flatten()["materials"][0]


def test_conductor_with_and_without_eta_k(mi, capi):
    m = _bsdf(mi, type="conductor")
    assert m["type"] == capi.MAT_CONDUCTOR == 1 and np.array_equal(m["p"][:3], [1, 1, 1])
    m = _bsdf(mi, type="conductor", specular_reflectance={"type": "rgb", "value": [0.9, 0.8, 0.7]})
    assert m["type"] == capi.MAT_CONDUCTOR and np.allclose(m["p"][:3], [0.9, 0.8, 0.7])
    m = _bsdf(mi, type="conductor", eta=0.5, k={"type": "rgb", "value": METAL_K})
    assert m["type"] == capi.MAT_CONDUCTOR_FRESNEL == 6
    assert np.allclose(m["p"], [0, 0.5, 0.5, 0.5, *METAL_K])
    m = _bsdf(mi, type="conductor", k=2.0)               # eta keeps the default of material 'none'
    assert m["type"] == capi.MAT_CONDUCTOR_FRESNEL and np.allclose(m["p"], [0, 0, 0, 0, 2, 2, 2])
    m = _bsdf(mi, type="roughconductor", distribution="ggx", alpha=0.3, eta={"type": "rgb", "value": METAL_ETA}, k=METAL_K,
              material="none", sample_visible=True, specular_reflectance=1.0)
    assert m["type"] == capi.MAT_ROUGHCONDUCTOR and np.allclose(m["p"], [0.3, *METAL_ETA, *METAL_K])
    m = _bsdf(mi, type="roughconductor", distribution="ggx", alpha_u=0.25, alpha_v=0.25)
    assert np.allclose(m["p"], [0.25, 0, 0, 0, 1, 1, 1])


@pytest.mark.parametrize("kw,word", [
    (dict(type="roughconductor"), "distribution"),                                     # Mitsuba's default is beckmann
    (dict(type="roughconductor", distribution="beckmann"), "distribution"),
    (dict(type="roughconductor", distribution="ggx", sample_visible=False), "sample_visible"),
    (dict(type="roughconductor", distribution="ggx", alpha_u=0.1, alpha_v=0.2), "alpha_u"),
    (dict(type="roughconductor", distribution="ggx", alpha_u=0.1), "alpha_u"),
    (dict(type="roughconductor", distribution="ggx", material="Au"), "material"),
    (dict(type="conductor", material="Cu"), "material"),
    (dict(type="roughconductor", distribution="ggx", specular_reflectance=0.5, eta=1.0, k=2.0), "specular_reflectance"),
    (dict(type="roughconductor", distribution="ggx", specular_reflectance=0.5), "specular_reflectance"),   # also without eta / k (D17)
    (dict(type="conductor", specular_reflectance=0.5, eta=1.0), "specular_reflectance"),
])
def test_refusals_name_the_property(mi, kw, word):
    with pytest.raises(NotImplementedError, match=word):
        _bsdf(mi, **kw)


def test_the_refusal_of_the_default_distribution_says_what_to_pass(mi):
    with pytest.raises(NotImplementedError, match="distribution='ggx'"):
        _bsdf(mi, type="roughconductor", alpha=0.1)


def test_xml_loader_accepts_the_same_properties(mi, capi, tmp_path):
    p = tmp_path / "rc.xml"
    p.write_text("""<scene version="3.0.0">
  <shape type="sphere">
    <bsdf type="roughconductor">
      <string name="distribution" value="ggx"/> <float name="alpha" value="0.2"/> <boolean name="sample_visible" value="true"/>
      <rgb name="eta" value="0.2, 0.9, 1.1"/> <spectrum name="k" value="3"/> <string name="material" value="none"/>
    </bsdf>
  </shape>
  <shape type="sphere"> <bsdf type="conductor"> <rgb name="eta" value="0.2, 0.9, 1.1"/> <float name="k" value="3"/> </bsdf> </shape>
  <shape type="sphere"> <bsdf type="roughconductor"> <float name="alpha" value="0.2"/> </bsdf> </shape>
</scene>""")
    with pytest.raises(NotImplementedError, match="distribution"):
        mi.load_file(str(p))
    p.write_text(p.read_text().replace('<shape type="sphere"> <bsdf type="roughconductor"> <float name="alpha" value="0.2"/> </bsdf> </shape>', ""))
    M = mi.load_file(str(p)).flatten()["materials"]
    assert list(M["type"]) == [capi.MAT_ROUGHCONDUCTOR, capi.MAT_CONDUCTOR_FRESNEL]
    assert np.allclose(M["p"][0], [0.2, 0.2, 0.9, 1.1, 3, 3, 3]) and np.allclose(M["p"][1], [0, 0.2, 0.9, 1.1, 3, 3, 3])


def test_traverse_exposes_alpha_eta_k(mi):
    sc = mi.load_dict(prototype_dict(mi))
    params = mi.traverse(sc)
    assert {"cylinder.bsdf.alpha", "cylinder.bsdf.eta", "cylinder.bsdf.k"} <= set(params.keys())
    sc.flatten()
    params["cylinder.bsdf.alpha"] = 0.4
    params["cylinder.bsdf.k"] = np.array([2.0, 3.0, 4.0])
    params.update()
    t, p = sc.flatten()["material_objects"][0].to_material()
    assert t == 5 and np.allclose(p, [0.4, 0, 0, 0, 2, 3, 4]) and sc._dirty_materials == {0}


@pytest.mark.parametrize("key,bad", [("alpha", 0.0), ("alpha", -0.1), ("alpha", float("nan")), ("alpha", float("inf")),
                                     ("eta", -1.0), ("eta", np.array([0.2, float("nan"), 1.0])), ("k", np.array([1.0, 2.0, -3.0])),
                                     ("k", float("inf"))])
def test_update_refuses_what_the_constructor_refuses(mi, key, bad):
    """params.update() raises the constructor's ValueError, the object keeps its values and no record is marked for upload"""
    sc = mi.load_dict(prototype_dict(mi))
    sc.flatten()
    params = mi.traverse(sc)
    params[f"cylinder.bsdf.{key}"] = bad
    with pytest.raises(ValueError, match=f"roughconductor: {key} must be finite"):
        params.update()
    t, p = sc.flatten()["material_objects"][0].to_material()
    assert t == 5 and np.array_equal(np.asarray(p, np.float32), np.array([0.1, 0, 0, 0, 1, 1, 1], np.float32))
    assert sc._dirty_materials == set()
    with pytest.raises(ValueError, match=f"roughconductor: {key} must be finite"):
        _bsdf(mi, type="roughconductor", distribution="ggx", **{key: bad if np.ndim(bad) == 0 else list(bad)})


@pytest.mark.parametrize("key,bad", [("eta", -0.5), ("k", float("nan"))])
def test_update_of_a_fresnel_conductor_is_validated(mi, key, bad):
    sc = mi.load_dict({"type": "scene", "s": {"type": "sphere", "bsdf": {"type": "conductor", "eta": METAL_ETA, "k": METAL_K}}})
    sc.flatten()
    params = mi.traverse(sc)
    params[f"s.bsdf.{key}"] = bad
    with pytest.raises(ValueError, match=f"conductor: {key} must be finite"):
        params.update()
    t, p = sc.flatten()["material_objects"][0].to_material()
    assert t == 6 and np.allclose(p, [0, *METAL_ETA, *METAL_K]) and sc._dirty_materials == set()
    params[f"s.bsdf.{key}"] = 0.75                                      # a valid value still goes through
    params.update()
    assert np.allclose(sc.flatten()["material_objects"][0].to_material()[1][1 + 3 * (key == "k"):][:3], 0.75)
    assert sc._dirty_materials == {0}


def test_header_declares_the_two_types_and_keeps_the_abi():
    from conftest import ROOT
    h = open(os.path.join(ROOT, "include", "pbrt_hip.h")).read()
    assert "#define PBRT_MAT_ROUGHCONDUCTOR 5u" in h and "#define PBRT_MAT_CONDUCTOR_FRESNEL 6u" in h
    assert "#define PBRT_ABI_VERSION 5" in h


# ---- self-checks of the restatement (float64) -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu,alpha", [(0.2, 0.05), (0.9, 0.1), (0.5, 0.5), (0.3, 1.0), (1.0, 0.02), (0.05, 0.3)])
def test_weak_white_furnace(mu, alpha):
    """with F = 1 the density D G1(wi) / (4 wi.z) integrates to 1 over the full sphere of wo (the visible normals are a
    distribution).  Quadrature over wo = reflect(wi, m) with d omega_o = 4 (wi . m) d omega_m, m on a grid that resolves the peak"""
    wi = np.array([np.sqrt(1 - mu * mu), 0.0, mu])
    v = [ru.integrate_over_wo(lambda wo: ru.terms(alpha, 0, 1, np.broadcast_to(wi, wo.shape), wo, hemisphere=False)[1][:, None],
                              alpha, wi, n)[0] for n in (256, 512)]
    assert abs(v[1] - 1.0) < 2e-5 and abs(v[1] - v[0]) < 2e-5, v


def test_fresnel_of_material_none_is_one_exactly():
    c = np.linspace(0, 1, 1001)
    for dt in (np.float32, np.float64):
        assert np.all(ru.fresnel_conductor(c.astype(dt), 0, 1, dt) == 1) and ru.fresnel_conductor(c.astype(dt), 0, 1, dt).dtype == dt


@pytest.mark.parametrize("eta", [1.5046 / 1.000277, 1.333, 2.419])
def test_fresnel_conductor_equals_the_dielectric_fresnel_at_k_0(eta):
    c = np.linspace(1e-3, 1, 500)
    assert np.allclose(ru.fresnel_conductor(c, eta, 0.0), ru.fresnel_dielectric_reflectance(c, eta), rtol=1e-12, atol=1e-14)
    assert 0.0 < ru.fresnel_conductor(1.0, eta, 0.0) == pytest.approx(((eta - 1) / (eta + 1)) ** 2, rel=1e-12)


def test_reciprocity_of_f():
    """f(wi, wo) = f cos(theta_o) / wo.z is symmetric in its arguments"""
    rng = np.random.default_rng(3)
    a, b = ru.normalize(rng.normal(size=(2000, 3))), ru.normalize(rng.normal(size=(2000, 3)))
    a[:, 2], b[:, 2] = np.abs(a[:, 2]) + 1e-3, np.abs(b[:, 2]) + 1e-3
    a, b = ru.normalize(a), ru.normalize(b)
    for alpha in (0.05, 0.3, 1.0):
        fab = ru.eval_pdf(alpha, METAL_ETA, METAL_K, a, b)[0] / b[:, 2:3]
        fba = ru.eval_pdf(alpha, METAL_ETA, METAL_K, b, a)[0] / a[:, 2:3]
        assert np.all(fab > 0) and np.allclose(fab, fba, rtol=1e-10, atol=0)


def test_weight_times_pdf_is_eval_and_the_sample_is_the_mirror_image():
    wi, u = ru.draw_inputs(7, 2000)
    for alpha in (0.02, 0.5):
        r = ru.sample(alpha, METAL_ETA, METAL_K, wi, u)
        v = r["valid"]
        f, p = ru.eval_pdf(alpha, METAL_ETA, METAL_K, wi[v].astype(np.float64), r["wo"][v])
        assert np.allclose(r["weight"][v] * r["pdf"][v][:, None], f, rtol=1e-12) and np.allclose(p, r["pdf"][v], rtol=1e-12)
        assert np.allclose(ru.normalize(wi[v] + r["wo"][v]), r["m"][v], atol=1e-9)


@pytest.mark.parametrize("alpha", [0.02, 0.1, 0.5, 1.0])
def test_the_drawn_records_of_the_device_test_qualify(alpha):
    """at least 90 % of the (wi, u) records of tests/test_gpu_roughconductor.py sit at least 1e-2 away from every decision of
    the sampler (wi.z, wo.z on either side of 0, |wi . m|), by the restatement alone; most of them return a direction"""
    wi, u = ru.draw_inputs(5, 4096)
    fl, r64, decided, v = ru.sample_floors(alpha, METAL_ETA, METAL_K, wi, u)
    assert decided.mean() >= 0.9 and v.mean() >= 0.55, (decided.mean(), v.mean())
    assert all(np.isfinite(x) and x < 1e-3 for x in fl.values()), fl


def test_albedo_quadrature_converges():
    for alpha in (0.1, 0.5):
        e = [ru.albedo(alpha, METAL_ETA, METAL_K, 0.8, n) for n in (256, 512)]
        assert np.abs(e[1] - e[0]).max() < 1e-4 and np.all((e[1] > 0) & (e[1] < 1))
