"""params.update() and DeviceScene.update_material on the device: a scene that has rendered -- plan learnt and run, keep words made,
first-bounce tables and a recording of us_render in use -- is updated and rendered again, and is held to a scene BUILT with the value
(tests/update_util.py), which never saw update() or a cache of the updated one.  Radiance films bit for bit, against the fresh
scene's device film and, where the oracle knows the materials, its oracle film; acquisitions under the per-bin tolerance of
tests/us_util.py against the oracle's acquisition of the fresh scene, with the same non-zero bins.  (The oracle does not know the
curved array: phantom_convex is held to the fresh scene's device acquisition under DESIGN.md section 3's ultrasound tolerance, rel.
L2 <= 1e-3 and the same non-zero words, as tests/test_gpu_convex_array.py holds its kernel families to one another.)

Films are 16 x 12 at 2 spp (the warm-up render takes 16: a plan is probed from 16 samples on), acquisitions 8 elements x 2 angles."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import update_util as upd
import us_util as uu
from conftest import oracle_render

pytestmark = pytest.mark.gpu

_IDS = dict(ids=lambda v: v if isinstance(v, str) else upd.case_id(v) if isinstance(v, tuple) else None)
_CACHE = {}     # references computed once and shared, never written


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _update(mi, sc, key, value):
    p = mi.traverse(sc)
    p[key] = value
    p.update()


# ---- radiance: every key of room and room_glossy, every accelerator -------------------------------------------------------------------
def _render(sc, spp=upd.SPP):
    return sc.integrator().render(sc, seed=upd.SEED, spp=spp)


def _warm(mi, capi, sc, accel):
    """two renders: the first probes the plan (brute force), the second runs the learnt one -> the film of the second"""
    sc.accel = accel
    ctx = mi.default_context()
    _render(sc, spp=16)
    st1 = ctx.stats()
    film = _render(sc)
    st2 = ctx.stats()
    if accel == capi.ACCEL_AUTO:
        assert st1["plan_source"] == capi.PLAN_PROBED and st2["plan_source"] == capi.PLAN_LEARNT, (st1["plan_source"], st2["plan_source"])
    else:
        assert st1["plan_source"] == st2["plan_source"] == capi.PLAN_STREAMS
    return film


def _camera_rays(sc):
    sens = sc.sensors()[0]
    w, h = sens.film().size()
    ys, xs = np.mgrid[0:h, 0:w]
    pos = np.stack([(xs.ravel() + 0.375) / w, (ys.ravel() + 0.625) / h], axis=1).astype(np.float32)
    return sens.sample_ray(0.0, 0.0, pos, None)[0]


def _light_queries(sc, rays):
    rng = np.random.default_rng(17)
    q = sc.sample_emitter_direction(rng.uniform(-0.9, 0.9, (1000, 3)).astype(np.float32), rng.random((1000, 4), dtype=np.float32))
    rgb = sc.integrator().sample(sc, sc.sensors()[0].sampler(), rays)[0]
    return {**{k: np.ascontiguousarray(v).tobytes() for k, v in q.items()}, "sample": rgb.tobytes()}


@pytest.mark.parametrize("accel", ["ACCEL_AUTO", "ACCEL_BVH", "ACCEL_BVH_GLOBAL"])
@pytest.mark.parametrize("name,case", [(n, c) for n in ("room", "room_glossy") for c in upd.cases(n, ("film",))], **_IDS)
def test_radiance_update_equals_a_fresh_scene(mi, ob, capi, name, case, accel):
    key, value, _ = case
    accel = getattr(capi, accel)
    sc = upd.build(mi, name)
    old = mi.traverse(sc)[key]
    before = _warm(mi, capi, sc, accel)
    rays = _camera_rays(sc)
    if upd.is_light_key(key):
        _light_queries(sc, rays)                      # (the old light has been asked for, too)
    _update(mi, sc, key, value)
    film = _render(sc)
    fresh = upd.build(mi, name, {key: value})
    fresh.accel = accel
    want = _render(fresh)
    assert _same(film, want), f"{np.count_nonzero(_bits(film) != _bits(want))} of {film.size} words differ from the fresh scene's film"
    if name == "room":
        ref = _cached(("oracle", name, upd.case_id(case)), lambda: oracle_render(ob, upd.build(mi, name, {key: value}), upd.SEED, upd.SPP)[0])
        assert _same(film, ref)
    assert np.isfinite(film).all() and not np.array_equal(film, before)
    assert _same(_render(sc), film)
    if upd.is_light_key(key):
        got, exp = _light_queries(sc, rays), _light_queries(fresh, rays)
        assert got.keys() == exp.keys()
        for k in got:
            assert got[k] == exp[k], f"{k} differs from the fresh scene's"
    _update(mi, sc, key, old)
    assert _same(_render(sc), before)


@pytest.mark.parametrize("name,case", [(n, c) for n in ("room_glossy",) for c in upd.cases(n, ("raises",))], **_IDS)
def test_a_refused_material_value_leaves_the_film(mi, capi, name, case):
    key, value, _ = case
    sc = upd.build(mi, name)
    before = _warm(mi, capi, sc, capi.ACCEL_AUTO)
    p = mi.traverse(sc)
    p[key] = value
    with pytest.raises(ValueError):
        p.update()
    assert _same(_render(sc), before)


# ---- every ordered pair of material types through DeviceScene.update_material -------------------------------------------------------------
def _records(capi):
    eta, k = [0.25, 1.0, 1.5], [3.5, 2.5, 2.0]
    return {"DIFFUSE": (capi.MAT_DIFFUSE, [0.5, 0.25, 0.75]), "CONDUCTOR": (capi.MAT_CONDUCTOR, [0.75, 0.5, 0.25]),
            "DIELECTRIC": (capi.MAT_DIELECTRIC, [1.5]), "NONE": (capi.MAT_NONE, []),
            "ROUGHCONDUCTOR": (capi.MAT_ROUGHCONDUCTOR, [0.25, *eta, *k]), "CONDUCTOR_FRESNEL": (capi.MAT_CONDUCTOR_FRESNEL, [0.0, *eta, *k])}


ORACLE_KNOWS = ("DIFFUSE", "CONDUCTOR", "DIELECTRIC", "NONE")


def _with_record(flat, index, record):
    """the room's material array with one record replaced"""
    mats = flat["materials"].copy()
    mats["type"][index] = record[0]
    mats["p"][index] = 0
    mats["p"][index, :len(record[1])] = record[1]
    return mats


class _Raw:
    """the room's arrays with one material record replaced, as a device scene of its own (pbrt_scene_create sees the record)"""

    def __init__(self, mi, capi, flat, index, record, accel):
        self.capi = capi
        self.dev = capi.DeviceScene(mi.default_context(), flat["prims"], _with_record(flat, index, record), flat["emitters"],
                                    flat["light_prims"], flat["light_cdf"], accel, flat["vertex_normals"])

    def render(self, cam, fd):
        out = np.empty((fd.crop_h, fd.crop_w, 3), np.float32)
        self.dev.ctx.check(self.dev.ctx.lib.pbrt_render_radiance(self.dev.handle, C.byref(cam), C.byref(fd), self.capi.addr(out)),
                           "pbrt_render_radiance")
        return out


def _material_index(sc, shape):
    flat = sc.flatten()
    return next(i for i, b in enumerate(flat["material_objects"]) if b is sc._objects[shape].bsdf())


@pytest.mark.parametrize("accel", ["ACCEL_AUTO", "ACCEL_BVH"])
@pytest.mark.parametrize("shape", ["back", "ball"])
def test_every_pair_of_material_types_through_update_material(mi, ob, capi, shape, accel):
    """src -> dst on the warm room for the 30 ordered pairs: the film after the update is the film of a scene created with dst, bit for
    bit (and the oracle's, where it knows dst).  The pairs switch `glossy` and with it the brute-force variant on and off under a
    learnt plan (any -> ROUGHCONDUCTOR / CONDUCTOR_FRESNEL and back), make paths longer (DIFFUSE -> DIELECTRIC) and shorter
    (-> NONE, which absorbs) than the plan was learnt from."""
    accel = getattr(capi, accel)
    base = upd.build(mi, "room")
    flat = base.flatten()
    index = _material_index(base, shape)
    integ, sens, ctx = base.integrator(), base.sensors()[0], mi.default_context()
    cam, fd, fd16 = sens.camera(), integ._film_desc(base, sens, upd.SEED, upd.SPP), integ._film_desc(base, sens, upd.SEED, 16)
    rec = _records(capi)
    want = {}
    for dst in rec:
        want[dst] = _Raw(mi, capi, flat, index, rec[dst], accel).render(cam, fd)
        if dst in ORACLE_KNOWS:
            osc = ob.OracleScene(flat["prims"], _with_record(flat, index, rec[dst]), flat["emitters"], flat["light_prims"], flat["light_cdf"],
                                 accel, flat["vertex_normals"])
            assert _same(want[dst], osc.render(cam, fd, n_threads=4)), f"created with {dst}: the device film is not the oracle's"
    assert len({want[d].tobytes() for d in want}) == len(want)      # six different films
    for src in rec:
        for dst in rec:
            if src == dst:
                continue
            raw = _Raw(mi, capi, flat, index, rec[src], accel)
            raw.render(cam, fd16)
            st1 = ctx.stats()
            before = raw.render(cam, fd)
            st2 = ctx.stats()
            if accel == capi.ACCEL_AUTO:
                assert (st1["plan_source"], st2["plan_source"]) == (capi.PLAN_PROBED, capi.PLAN_LEARNT), (src, dst)
            assert _same(before, want[src]), (src, dst)
            raw.dev.update_material(index, capi.make_material(*rec[dst]))
            film = raw.render(cam, fd)
            assert _same(film, want[dst]), f"{src} -> {dst}: {np.count_nonzero(_bits(film) != _bits(want[dst]))} words differ from a scene created with {dst}"
            assert _same(raw.render(cam, fd), film), (src, dst)
            raw.dev.close()


@pytest.mark.parametrize("accel", ["ACCEL_AUTO", "ACCEL_BVH"])
def test_a_refused_record_leaves_film_and_scene(mi, capi, accel):
    accel = getattr(capi, accel)
    base = upd.build(mi, "room")
    flat = base.flatten()
    integ, sens = base.integrator(), base.sensors()[0]
    cam, fd, fd16 = sens.camera(), integ._film_desc(base, sens, upd.SEED, upd.SPP), integ._film_desc(base, sens, upd.SEED, 16)
    rec = _records(capi)
    index = _material_index(base, "back")
    raw = _Raw(mi, capi, flat, index, rec["DIFFUSE"], accel)
    raw.render(cam, fd16)
    before = raw.render(cam, fd)
    eta, k = rec["ROUGHCONDUCTOR"][1][1:4], rec["ROUGHCONDUCTOR"][1][4:7]
    for bad in ((capi.MAT_ROUGHCONDUCTOR, [0.0, *eta, *k]), (capi.MAT_ROUGHCONDUCTOR, [float("nan"), *eta, *k]),
                (capi.MAT_ROUGHCONDUCTOR, [0.25, *eta, -1.0, 2.0, 2.0]), (capi.MAT_CONDUCTOR_FRESNEL, [0.0, *eta, 1.0, -0.5, 1.0])):
        with pytest.raises(RuntimeError, match="must be finite"):
            raw.dev.update_material(index, capi.make_material(*bad))
        assert _same(raw.render(cam, fd), before)
    raw.dev.update_material(index, capi.make_material(*rec["ROUGHCONDUCTOR"]))     # the scene still takes a good record
    assert _same(raw.render(cam, fd), _Raw(mi, capi, flat, index, rec["ROUGHCONDUCTOR"], accel).render(cam, fd))


# ---- ultrasound: every key of the phantoms ----------------------------------------------------------------------------------------------
US_PPR = 64      # >= the 8 elements: the first-bounce tables are on (where the rays are the integrator's own)


def _us_reference(mi, ob, name, overrides, ppr, q):
    """(ref, tx, tol) of the oracle for the scene built with the overrides; None for the curved array, which it does not know"""
    fresh = upd.build(mi, name, overrides, ppr=ppr)
    if name == "phantom_convex":
        return fresh, None
    return fresh, uu.acquire_ref(ob, fresh, fresh.integrator(), upd.US_SEED, ppr, quirks=q)


def _hold(name, got, fresh, oracle, q, what):
    """got against the reference of the fresh scene"""
    assert np.isfinite(got).all()
    if oracle is None:
        want = fresh.integrator()._acquire(fresh, q)
        assert (want != 0).sum() > 100
        assert np.array_equal(got != 0, want != 0), f"{what}: {int(((got != 0) != (want != 0)).sum())} words differ in being non-zero"
        rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        assert rel <= 1e-3, f"{what}: rel. L2 {rel:.3g}"
        return
    ref, tx, tol = oracle
    assert np.array_equal(got != 0, ref != 0), f"{what}: {int(((got != 0) != (ref != 0)).sum())} bins differ in being non-zero"
    ratio = uu.worst_ratio(got, ref, tol)
    print(f"{what}: |got - ref| reaches {ratio:.3g} x the per-bin tolerance")
    assert ratio <= 1.0, f"{what}: |got - ref| reaches {ratio:.3g} x the per-bin tolerance"


@pytest.mark.parametrize("name,case", [(n, c) for n in ("phantom", "phantom_plain", "phantom_convex")
                                       for c in upd.cases(n, ("acq", "bytes", "unread"))], **_IDS)
def test_acquisition_after_update_equals_a_fresh_scene(mi, ob, capi, name, case):
    key, value, consumer = case
    material = ".bsdf." in key
    for tables in ((True, False) if material else (True,)):
        sc = upd.build(mi, name, ppr=US_PPR)
        ui = sc.integrator()
        q = ui.quirks | (0 if tables else capi.USQ_NO_FIRST_TABLES)
        what = f"{name} {upd.case_id(case)} tables={tables}"
        before = ui._acquire(sc, q)
        fresh0, oracle0 = _cached(("us0", name, tables), lambda: _us_reference(mi, ob, name, {}, US_PPR, q))
        _hold(name, before, fresh0, oracle0, q, what + " (before)")
        old = mi.traverse(sc)[key]
        _update(mi, sc, key, value)
        after = ui._acquire(sc, q)
        fresh, oracle = _us_reference(mi, ob, name, {key: value}, US_PPR, q)
        _hold(name, after, fresh, oracle, q, what)
        if oracle is not None:
            assert np.array_equal(ui.transmission_delays_buf, oracle[1])
            assert np.array_equal(oracle[0], oracle0[0]) == (consumer != "acq")
        if consumer == "acq" and oracle is not None:      # ... and it is not the acquisition from before: other bins, or beyond its tolerance
            assert not np.array_equal(after != 0, oracle0[0] != 0) or uu.worst_ratio(after, oracle0[0], oracle0[2]) > 1.0, what
        elif consumer == "acq":
            assert not np.array_equal(after != 0, before != 0) or float(np.linalg.norm(after - before)) > 2e-3 * float(np.linalg.norm(before)), what
        _update(mi, sc, key, old)
        _hold(name, ui._acquire(sc, q), fresh0, oracle0, q, what + " (and back)")


@pytest.mark.parametrize("case", [c for c in upd.cases("phantom_plain", ("rx", "unread")) if c[0].startswith("rx.")], **_IDS)
def test_custom_sensor_keys_at_put_data(mi, case):
    key, value, consumer = case
    sc = upd.build(mi, "phantom_plain")
    rx = sc.sensors()[1]
    rays, amp = upd.rx_rays()
    rx.put_data(rays, amp)
    before = rx.channel_data().copy()
    assert np.count_nonzero(before) >= 4
    _update(mi, sc, key, value)
    assert not rx.channel_data().any()                     # parameters_changed clears the buffer (CustomSensor.py:75-76)
    rx.put_data(rays, amp)
    fresh = upd.build(mi, "phantom_plain", {key: value}).sensors()[1]
    fresh.put_data(rays, amp)
    assert _same(rx.channel_data(), fresh.channel_data()) and np.count_nonzero(fresh.channel_data()) >= 4
    assert (rx.channel_data().shape == before.shape and np.array_equal(rx.channel_data(), before)) == (consumer == "unread")


# ---- us_render: the recording follows the update -----------------------------------------------------------------------------------------
def _scan_kw(ui, z0):
    step = (ui.sound_speed / ui.frequency) / 4
    return dict(x_range=(-11.5 * step, 11 * step), z_range=(z0 - 31.5 * step, z0 + 31 * step), step=step)


def _three(mi, sc, kw):
    flags, out = [], None
    for _ in range(3):
        tm = {}
        out = mi.us_render(sc, timing=tm, **kw)
        flags.append(tm["replayed"])
    return flags, out


def _render_reference(mi, ob, name, overrides):
    """what a us_render of the scene built with the overrides is held to: the fresh integrator (probe, sound speed), the reference
    channel data, the delays, the per-bin tolerance (None for the curved array: the reference is the fresh scene's own acquisition on
    the device, made -- and its device scene closed -- before the first us_render: destroying a scene drops the context's recordings)"""
    fresh = upd.build(mi, name, overrides, ppr=1)
    fi = fresh.integrator()
    if name == "phantom_convex":
        ref, tol = fi._acquire(fresh, fi.quirks), None
        delays = np.asarray(fi.transmission_delays_buf, np.float32)
        fresh.device().close()
    else:
        ref, delays, tol = uu.acquire_ref(ob, fresh, fi, upd.US_SEED, 1)
    return dict(scene=fresh, fi=fi, ref=ref, delays=delays, tol=tol)


def _hold_render(mi, sc, out, want, kw, what):
    """the channel buffer the device chain used against the fresh scene's reference, and the display image against the host form of
    the chain on that buffer with the fresh scene's probe and delays -> the channel buffer"""
    bf = import_module(mi.__name__ + ".beamform")
    disp, env, (xs, zs) = out
    assert len(xs) <= 25 and len(zs) <= 65 and disp.shape == (len(zs), len(xs))
    ui = sc.integrator()
    chan = ui._render_plan.d_channel.numpy()
    ref, delays, tol, fi = want["ref"], want["delays"], want["tol"], want["fi"]
    assert np.array_equal(chan != 0, ref != 0) and np.count_nonzero(ref) > 8, what
    if tol is None:
        assert float(np.linalg.norm(chan - ref)) <= 1e-3 * float(np.linalg.norm(ref)), what
    else:
        assert uu.worst_ratio(chan, ref, tol) <= 1.0, what
    assert np.array_equal(np.asarray(ui.transmission_delays_buf, np.float32).ravel(), delays.ravel()), what
    rq = bf._us_render_request(fi, kw["x_range"], kw["z_range"], 60.0, kw["step"], None, None, kw.get("beamformer"), False, 1,
                               kw.get("scan", "grid"), None)
    h_disp, h_env = bf._form_image(rq, np.ascontiguousarray(chan, np.float32), delays.reshape(rq.A, rq.E), bf._HostBuffers)
    assert np.isfinite(env).all() and env.max() > 0
    assert _same(env, h_env) and _same(disp, h_disp.T), f"{what}: the image is not the host chain's on the fresh scene's probe and delays"
    return chan


RENDER_CASES = ([("phantom", c, {}) for c in upd.cases("phantom", ("acq", "bytes", "unread"))] +
                [("phantom_convex", c, {}) for c in upd.cases("phantom_convex", ("acq", "bytes"))] +
                [("phantom_plain", c, {"scan": "polar"}) for c in upd.cases("phantom_plain", ("acq",)) if c[0] in ("integrator.pitch", "p0.bsdf.roughness")] +
                [("phantom_plain", c, {"capon": True}) for c in upd.cases("phantom_plain", ("acq",)) if c[0] == "integrator.pitch"])


@pytest.mark.parametrize("name,case,extra", RENDER_CASES,
                         ids=[f"{n}-{upd.case_id(c)}{'-' + '-'.join(e) if e else ''}" for n, c, e in RENDER_CASES])
def test_us_render_after_update(mi, ob, name, case, extra):
    key, value, consumer = case
    sc = upd.build(mi, name, ppr=1)
    ui = sc.integrator()
    kw = _scan_kw(ui, ui.radius + 0.02 if name == "phantom_convex" else 0.016)
    if extra.get("scan"):
        kw["scan"] = extra["scan"]
    if extra.get("capon"):
        kw["beamformer"] = mi.Capon()
    what = f"{name} {upd.case_id(case)} {extra}"
    want0, want = _render_reference(mi, ob, name, {}), _render_reference(mi, ob, name, {key: value})
    flags, out = _three(mi, sc, kw)
    assert flags == [False, False, True], what
    chan0 = _hold_render(mi, sc, out, want0, kw, what + " (before)")
    _update(mi, sc, key, value)
    flags, out = _three(mi, sc, kw)
    if ".bsdf." in key:
        assert flags == [True, True, True], f"{what}: a material update writes device memory, the recording stands ({flags})"
    elif consumer != "unread":
        assert flags == [False, False, True], f"{what}: the key is part of the request, the recording is made again ({flags})"
    assert flags[2]
    chan = _hold_render(mi, sc, out, want, kw, what)
    if not np.array_equal(want["ref"], want0["ref"]):      # (at one path per ray not every material is met)
        assert not np.array_equal(chan, chan0), what
