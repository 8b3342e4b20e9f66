"""params = traverse(scene); params[key] = v; params.update() on the host (no GPU): after the update everything the scene hands to
the library -- the flattened arrays, the camera, the film description, pbrt_us_params -- is, byte for byte, what a scene BUILT with
the value hands to it (tests/update_util.py), for every key traverse() exposes, with every cache warm beforehand.  Where the CPU
oracle knows the scene, its film or its channel data are those of the fresh scene bit for bit, and not those from before.

A stale cache agrees with itself: the oracle of the suite's other tests is built from scene.flatten(), the arrays the device scene
was uploaded from.  The reference here never went through update()."""
import numpy as np
import pytest

import update_util as upd
import us_util as uu
from conftest import oracle_render

US_PPR = 64


def _warm(sc):
    """every cache of the host side, filled: flatten(), the camera, the film description, the acquisition's block"""
    return upd.snapshot(sc)


def _update(mi, sc, key, value):
    p = mi.traverse(sc)
    p[key] = value
    p.update()
    return p


def _aliases(sc, p, key):
    """every traversed key with the owner and parameter of `key`"""
    owner, name, _ = p._table[key]
    return [k for k, (o, n, _) in p._table.items() if o is owner and n == name]


def _assert_same(got, want, what):
    flat_g, rq_g = got
    flat_w, rq_w = want
    for k in upd.FLAT:
        assert flat_g[k] == flat_w[k], f"{what}: flatten()['{k}'] differs"
    assert rq_g.keys() == rq_w.keys()
    for k in rq_g:
        assert rq_g[k] == rq_w[k], f"{what}: {k} differs"


@pytest.mark.parametrize("name", upd.SCENES)
def test_every_traversed_key_has_a_case(mi, name):
    keys = set(mi.traverse(upd.build(mi, name)).keys())
    assert keys == set(upd.CASES[name]), (sorted(keys - set(upd.CASES[name])), sorted(set(upd.CASES[name]) - keys))
    assert all(upd.CASES[name][k] for k in keys)


def test_the_shared_bsdf_is_traversed_under_its_aliases(mi):
    sc = upd.build(mi, "room")
    p = mi.traverse(sc)
    assert set(_aliases(sc, p, "white.reflectance")) == {"white.reflectance", "floor.bsdf.reflectance", "ceiling.bsdf.reflectance"}
    f = sc.flatten()
    assert len(f["prims"]) <= 32 and f["prims"]["material"][0] == f["prims"]["material"][1]
    assert len(f["emitters"]) == 2 and len(f["light_prims"]) == 1


def _check_case(mi, name, key, value, consumer):
    sc = upd.build(mi, name)
    before = _warm(sc)
    old = mi.traverse(sc)[key]
    fresh = upd.build(mi, name, {key: value})
    want = upd.snapshot(fresh)
    p = _update(mi, sc, key, value)
    for k in _aliases(sc, p, key):
        assert upd.same_value(p[k], value) and upd.same_value(mi.traverse(sc)[k], value), k
    after = upd.snapshot(sc)
    _assert_same(after, want, f"{name} {key}")
    if consumer == "unread":
        assert after == before
    elif consumer != "rx":
        assert after != before, f"{name} {key}: nothing handed to the library changed"
    return sc, fresh, before, old


_IDS = dict(ids=lambda v: v if isinstance(v, str) else upd.case_id(v))
_BEFORE = {}     # scene name -> the oracle's film / channel data of the scene as built: computed once, never written


def _before(name, make):
    if name not in _BEFORE:
        _BEFORE[name] = make()
        _BEFORE[name].setflags(write=False)
    return _BEFORE[name]


@pytest.mark.parametrize("name,case", [(n, c) for n in ("room", "room_glossy") for c in upd.cases(n, ("film",))], **_IDS)
def test_radiance_update_equals_a_fresh_scene(mi, ob, name, case):
    key, value, consumer = case
    what = upd.case_id(case)
    sc, fresh, before, old = _check_case(mi, name, key, value, consumer)
    if name == "room":    # the oracle knows every material of this room
        film0 = _before(name, lambda: oracle_render(ob, upd.build(mi, name), upd.SEED, upd.SPP)[0])
        got, want = oracle_render(ob, sc, upd.SEED, upd.SPP)[0], oracle_render(ob, fresh, upd.SEED, upd.SPP)[0]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what
        assert not np.array_equal(got, film0), f"{what}: the film does not depend on it"
    _update(mi, sc, key, old)
    _assert_same(upd.snapshot(sc), before, f"{what}, and back")
    if name == "room":
        assert np.array_equal(oracle_render(ob, sc, upd.SEED, upd.SPP)[0], film0)


def _us_ref0(mi, ob, name):
    sc0 = upd.build(mi, name)
    return uu.acquire_ref(ob, sc0, sc0.integrator(), upd.US_SEED, US_PPR)[0]


@pytest.mark.parametrize("name,case", [(n, c) for n in ("phantom", "phantom_plain", "phantom_convex")
                                       for c in upd.cases(n, ("acq", "bytes", "unread", "rx"))], **_IDS)
def test_ultrasound_update_equals_a_fresh_scene(mi, ob, name, case):
    key, value, consumer = case
    what = upd.case_id(case)
    sc, fresh, before, old = _check_case(mi, name, key, value, consumer)
    if name != "phantom_convex" and consumer != "rx":       # (the oracle does not know the curved array)
        ref0 = _before(name, lambda: _us_ref0(mi, ob, name))
        assert np.count_nonzero(ref0) > 50
        got = uu.acquire_ref(ob, sc, sc.integrator(), upd.US_SEED, US_PPR)[0]
        want = uu.acquire_ref(ob, fresh, fresh.integrator(), upd.US_SEED, US_PPR)[0]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what
        assert np.array_equal(got, ref0) == (consumer != "acq"), f"{what}: consumer {consumer}"
    if consumer == "rx":
        rx, rx_fresh = sc.sensors()[1], fresh.sensors()[1]
        assert rx.channel_data().shape == rx_fresh.channel_data().shape and not rx.channel_data().any()
        for k in ("number_of_elements", "pitch", "element_width", "element_height", "sample_rate", "speed_of_sound", "time_samples"):
            assert getattr(rx, k) == getattr(rx_fresh, k), k
    _update(mi, sc, key, old)
    _assert_same(upd.snapshot(sc), before, f"{what}, and back")


@pytest.mark.parametrize("name,case", [(n, c) for n in upd.SCENES for c in upd.cases(n, ("raises",))],
                         **_IDS)
def test_what_cannot_be_honoured_raises_and_changes_nothing(mi, name, case):
    key, value, _ = case
    sc = upd.build(mi, name)
    before = _warm(sc)
    p = mi.traverse(sc)
    old = p[key]
    p[key] = value
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        p.update()
    assert upd.same_value(p[key], old) and upd.same_value(mi.traverse(sc)[key], old)
    _assert_same(upd.snapshot(sc), before, f"{name} {key} refused")
    p.update()      # nothing is pending: the refused value is gone
    _assert_same(upd.snapshot(sc), before, f"{name} {key} refused, second update")


def test_the_issue_s_example(mi):
    """cbox.xml and simple.xml: the lights' keys reach flatten() (they did not: update() told the scene about BSDFs only)"""
    from conftest import scene_path
    sc = mi.load_file(scene_path("cbox.xml"), res=8, spp=1)
    e0 = sc.flatten()["emitters"].copy()
    p = mi.traverse(sc)
    p["luminaire.emitter.radiance"] = np.array([2.0, 2.0, 2.0])
    p.update()
    e1 = sc.flatten()["emitters"]
    assert not np.array_equal(e1, e0) and np.array_equal(e1["radiance"][0], np.float32([2, 2, 2]))
    sc = mi.load_file(scene_path("simple.xml"))
    e0 = sc.flatten()["emitters"].copy()
    p = mi.traverse(sc)
    p["lamp_a.intensity"] = 2.0 * np.asarray(p["lamp_a.intensity"])
    p["lamp_a.position"] = np.asarray(p["lamp_a.position"]) + 0.25
    p.update()
    e1 = sc.flatten()["emitters"]
    assert np.array_equal(e1["radiance"][0], 2.0 * e0["radiance"][0]) and np.array_equal(e1["pos"][0], (e0["pos"][0].astype(np.float64) + 0.25).astype(np.float32))
    assert np.array_equal(e1[1:], e0[1:])


def test_keys_that_belong_together_are_updated_together(mi):
    """one of them alone is refused (the cases above); one update() of all four makes the array an arc on both sides"""
    joint = {"integrator.radius": 0.04, "integrator.opening_angle": 40.0, "emitter.radius": 0.04, "emitter.opening_angle": 40.0}
    sc = upd.build(mi, "phantom")
    before = _warm(sc)
    p = mi.traverse(sc)
    for k, v in joint.items():
        p[k] = v
    p.update()
    after = upd.snapshot(sc)
    _assert_same(after, upd.snapshot(upd.build(mi, "phantom", joint)), "phantom, the four array keys")
    assert after != before and sc.integrator().us_params(sc).primary == (mi._capi.US_PRIMARY_EMITTER | mi._capi.US_ARRAY_CONVEX)
