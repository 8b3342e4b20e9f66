"""Scene creation as a caller sees it (csrc/scene_request.h; the whole rule table and every decision are held on the CPU by
tests/test_scene_request_host.py): every rule refused through pbrt_scene_create with its code and its exact pbrt_last_error text,
each refusal followed by a valid scene on the same context that renders what it rendered before; the accelerator the library
chooses at 32 and 33 primitives and the two forced trees on a two-primitive scene, each film equal to the oracle's; a material
update to a rough conductor and back against scenes created with those materials; and a refused creation beside a queued
acquisition, which must stay queued.  Scenes of 2 to 33 primitives, films of 16 x 16 pixels at 2 samples."""
import ctypes as C

import numpy as np
import pytest

from conftest import oracle_render
from test_gpu_typed_runs import DIF, _film_parts, _shapes

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -4
INTEGER_STATS = ("samples", "segments", "shadow_rays", "bounce_launches", "passes", "model_bytes", "bounce_model_bytes", "live",
                 "fuse_plan", "plan_source", "pass_paths", "trace_model_bytes")   # (not workspace_bytes: that is the context's history)


def _lit(mi, tmp_path, spec, seed=None, bulb=False):
    d = _film_parts(mi)
    d.update(_shapes(mi, tmp_path, spec, len(spec) if seed is None else seed))
    if bulb:
        d["bulb"] = {"type": "point", "position": [0.3, 0.2, 2.5], "intensity": {"type": "rgb", "value": [8, 8, 8]}}
    return mi.load_dict(d)


def _arrays(sc):
    """copies of the scene's C-ABI arrays, to edit"""
    f = sc.flatten()
    a = {k: f[k].copy() for k in ("prims", "materials", "emitters", "light_prims", "light_cdf")}
    a["vertex_normals"] = None if f["vertex_normals"] is None else f["vertex_normals"].copy()
    return a


def _create(capi, ctx, a, accel=0, desc_edit=None):
    """pbrt_scene_create through ctypes -> (code, handle, message)"""
    desc = capi.fill_scene_desc(a["prims"], a["materials"], a["emitters"], a["light_prims"], a["light_cdf"], accel, a["vertex_normals"])
    if desc_edit:
        desc_edit(desc)
    h = C.c_void_p()
    rc = ctx.lib.pbrt_scene_create(ctx.handle, C.byref(desc), C.byref(h))
    return rc, h, ctx.lib.pbrt_last_error(ctx.handle).decode()


def _render(ctx, handle, sc, seed=1):
    integ, sens = sc.integrator(), sc.sensors()[0]
    fd, cam = integ._film_desc(sc, sens, seed, 2), sens.camera()
    out = np.empty((fd.crop_h, fd.crop_w, 3), np.float32)
    assert ctx.lib.pbrt_render_radiance(handle, C.byref(cam), C.byref(fd), out.ctypes.data) == 0, ctx.lib.pbrt_last_error(ctx.handle)
    st = ctx.stats()
    return out, {k: st[k] for k in INTEGER_STATS}


def _set(field, index, value, sub=None):
    def edit(a):
        if sub is None:
            a[field][index] = value
        else:
            a[field][sub][index] = value
    return edit


def test_every_rule_is_refused_with_its_text_and_leaves_the_context_as_it_was(mi, capi, tmp_path):
    """the light, a rectangle, a triangle, a sphere, a cone and a cylinder, a material each; an area light and a point light"""
    sc = _lit(mi, tmp_path, "QTSCY", bulb=True)
    base = _arrays(sc)
    types = [int(t) for t in base["prims"]["type"]]
    assert types == [2, 2, 0, 1, 3, 4] and len(base["materials"]) == 6 and [int(t) for t in base["emitters"]["type"]] == [0, 1]
    n = len(types)

    def both(*edits):
        return lambda a: [e(a) for e in edits]

    def normals(entry):
        def edit(a):
            a["vertex_normals"] = np.zeros((n, 9), np.float32)
            a["vertex_normals"].reshape(-1)[entry] = np.nan
        return edit

    rough = lambda i, p: both(_set("materials", i, 5, "type"), _set("materials", i, p, "p"))
    ok_p = [0.2, 0.2, 0.9, 1.1, 3.0, 2.4, 2.0]
    COUNTS = "invalid argument: d->n_prims > 0 && d->prims && d->n_materials > 0 && d->materials"
    # (name, edit of the arrays, accel, edit of the descriptor, code, text)
    cases = [
        ("no primitives", None, 0, lambda d: setattr(d, "n_prims", 0), E_INVALID, COUNTS),
        ("no material table", None, 0, lambda d: setattr(d, "materials", None), E_INVALID, COUNTS),
        ("no emitter table", None, 0, lambda d: setattr(d, "emitters", None), E_INVALID, "invalid argument: d->n_emitters == 0 || d->emitters"),
        ("no light cdf", None, 0, lambda d: setattr(d, "light_cdf", None), E_INVALID,
         "invalid argument: d->n_light_prims == 0 || (d->light_prims && d->light_cdf)"),
        ("primitive type", _set("prims", n - 1, 5, "type"), 0, None, E_UNSUPPORTED, f"primitive {n - 1}: type 5 is not supported"),
        ("cone frame", _set("prims", 4, np.zeros(12, np.float32), "g"), 0, None, E_INVALID,
         "primitive 4: cone needs an invertible, finite world -> object matrix"),
        ("cylinder frame", _set("prims", 5, np.full(12, np.nan, np.float32), "g"), 0, None, E_INVALID,
         "primitive 5: cylinder needs an invertible, finite world -> object matrix"),
        ("material index", _set("prims", 0, 6, "material"), 0, None, E_INVALID, "primitive 0: material out of range"),
        ("emitter index", _set("prims", 3, 2, "emitter"), 0, None, E_INVALID, "primitive 3: emitter out of range"),
        ("alpha", rough(1, [0.0] + ok_p[1:]), 0, None, E_INVALID, "material 1: roughconductor alpha must be finite and > 0"),
        ("eta", rough(0, ok_p[:2] + [-0.5] + ok_p[3:]), 0, None, E_INVALID, "material 0: conductor eta must be finite and >= 0"),
        ("k", rough(5, ok_p[:6] + [np.inf]), 0, None, E_INVALID, "material 5: conductor k must be finite and >= 0"),
        ("light range", _set("emitters", 0, 2, "count"), 0, None, E_INVALID, "emitter 0: light primitive range out of bounds"),
        ("area light on a sphere", _set("light_prims", 0, 3), 0, None, E_UNSUPPORTED,
         "emitter 0: area lights need triangle/parallelogram primitives"),
        ("emitter type", _set("emitters", 1, 2, "type"), 0, None, E_INVALID, "emitter 1: unknown type"),
        ("vertex normal", normals(9 * n - 1), 0, None, E_INVALID, f"vertex_normals: entry {9 * n - 1} is not finite"),
        ("accel", None, 4, None, E_INVALID, "invalid argument: d->accel <= PBRT_ACCEL_BVH_GLOBAL"),
        # two rules broken: the earlier one speaks
        ("accel and a material index", _set("prims", 2, 7, "material"), 4, None, E_INVALID, "primitive 2: material out of range"),
        ("a vertex normal and an emitter type", both(normals(0), _set("emitters", 1, 9, "type")), 0, None, E_INVALID, "emitter 1: unknown type"),
    ]
    ctx = mi.Context()
    try:
        rc, h, msg = _create(capi, ctx, base)
        assert rc == 0, msg
        want, want_stats = _render(ctx, h, sc)
        assert ctx.lib.pbrt_scene_destroy(h) == 0 and want.mean() > 0
        for name, edit, accel, desc_edit, code, text in cases:
            a = _arrays(sc)
            if edit:
                edit(a)
            rc, h, msg = _create(capi, ctx, a, accel, desc_edit)
            assert (rc, msg) == (code, text) and not h.value, name
            rc, h, msg = _create(capi, ctx, base)
            assert rc == 0, (name, msg)
            got, got_stats = _render(ctx, h, sc)
            assert ctx.lib.pbrt_scene_destroy(h) == 0
            assert np.array_equal(got, want) and got_stats == want_stats, name
        # the null rule: no description, no place for the handle
        h = C.c_void_p()
        assert ctx.lib.pbrt_scene_create(ctx.handle, None, C.byref(h)) == E_INVALID
        assert ctx.lib.pbrt_last_error(ctx.handle).decode() == "invalid argument: d && out"
        desc = capi.fill_scene_desc(base["prims"], base["materials"], base["emitters"], base["light_prims"], base["light_cdf"], 4)
        assert ctx.lib.pbrt_scene_create(ctx.handle, C.byref(desc), None) == E_INVALID
        assert ctx.lib.pbrt_last_error(ctx.handle).decode() == "invalid argument: d && out"
    finally:
        ctx.close()


@pytest.mark.parametrize("name,n_shapes,accel,streams", [("auto_32", 31, "AUTO", False), ("auto_33", 32, "AUTO", True),
                                                         ("bvh_2", 1, "BVH", True), ("bvh_global_2", 1, "BVH_GLOBAL", True)])
def test_the_accelerator_choice_and_its_film(mi, ob, capi, tmp_path, name, n_shapes, accel, streams):
    """rectangles, spheres and a triangle soup with diffuse materials under the rectangle light (no two primitives alike: the film
    does not depend on which of two tied hits an accelerator reports)"""
    rng = np.random.default_rng(n_shapes)
    T = mi.ScalarTransform4f
    d = _film_parts(mi)
    n_tris = n_shapes // 2
    for k in range(n_shapes - n_tris):
        if k % 2 == 0:
            tw = T().translate(list(rng.uniform(-1.2, 1.2, 3))) @ T().rotate(list(rng.normal(size=3)), float(rng.uniform(0, 360))) @ \
                T().scale([float(rng.uniform(0.3, 0.8)), float(rng.uniform(0.3, 0.8)), 1.0])
            d[f"q{k}"] = {"type": "rectangle", "to_world": tw, "bsdf": DIF}
        else:
            d[f"s{k}"] = {"type": "sphere", "center": list(rng.uniform(-1.2, 1.2, 3)), "radius": float(rng.uniform(0.2, 0.5)), "bsdf": DIF}
    if n_tris:
        v = rng.uniform(-1.4, 1.4, (n_tris, 1, 3)) + rng.normal(scale=0.35, size=(n_tris, 3, 3))
        with open(tmp_path / "soup.obj", "w") as f:
            f.writelines(f"v {p[0]:.6f} {p[1]:.6f} {p[2]:.6f}\n" for p in v.reshape(-1, 3))
            f.writelines(f"f {3 * i + 1} {3 * i + 2} {3 * i + 3}\n" for i in range(n_tris))
        d["soup"] = {"type": "obj", "filename": str(tmp_path / "soup.obj"), "bsdf": DIF}
    sc = mi.load_dict(d)
    assert len(sc.flatten()["prims"]) == n_shapes + 1 and {int(t) for t in sc.flatten()["prims"]["type"]} == ({0, 1, 2} if n_shapes > 1 else {2})
    sc.accel = getattr(capi, "ACCEL_" + accel)
    img = sc.integrator().render(sc, seed=3, spp=2)
    st = mi.default_context().stats()
    assert (st["plan_source"] == capi.PLAN_STREAMS) == streams and st["samples"] == 16 * 16 * 2
    ref, _ = oracle_render(ob, sc, 3, 2, accel=sc.accel)
    assert img.shape == (16, 16, 3) and np.array_equal(img, ref) and img.mean() > 0


def test_a_material_update_renders_what_a_scene_created_with_it_renders(mi, capi, tmp_path):
    """diffuse -> ROUGHCONDUCTOR -> diffuse on material 1 of a small brute-force scene: the kernel variant follows each time"""
    sc = _lit(mi, tmp_path, "QQS")
    diffuse, rough = _arrays(sc), _arrays(sc)
    alu = [0.15, 1.66, 0.88, 0.52, 9.22, 6.27, 4.84]
    rough["materials"]["type"][1], rough["materials"]["p"][1] = 5, alu
    ctx = mi.Context()
    handles = []
    try:
        films = {}
        for key, a in (("diffuse", diffuse), ("rough", rough)):
            rc, h, msg = _create(capi, ctx, a)
            assert rc == 0, msg
            handles.append(h)
            films[key] = _render(ctx, h, sc)
        assert not np.array_equal(films["diffuse"][0], films["rough"][0]) and films["diffuse"][0].mean() > 0 and films["rough"][0].mean() > 0
        rc, h, msg = _create(capi, ctx, diffuse)
        assert rc == 0, msg
        handles.append(h)
        m = capi.make_material(5, alu)
        assert ctx.lib.pbrt_scene_update_material(h, 1, C.byref(m)) == 0
        got = _render(ctx, h, sc)
        assert np.array_equal(got[0], films["rough"][0])
        m = capi.make_material(int(diffuse["materials"]["type"][1]), [float(v) for v in diffuse["materials"]["p"][1]])
        assert ctx.lib.pbrt_scene_update_material(h, 1, C.byref(m)) == 0
        got = _render(ctx, h, sc)
        assert np.array_equal(got[0], films["diffuse"][0])      # (its plan is the one learnt from the render before: any plan, one film)
        # a refused update changes nothing
        m = capi.make_material(5, [0.0] + alu[1:])
        assert ctx.lib.pbrt_scene_update_material(h, 1, C.byref(m)) == E_INVALID
        assert ctx.lib.pbrt_last_error(ctx.handle).decode() == "material 1: roughconductor alpha must be finite and > 0"
        assert np.array_equal(_render(ctx, h, sc)[0], films["diffuse"][0])
    finally:
        for h in handles:
            ctx.lib.pbrt_scene_destroy(h)
        ctx.close()


def test_a_refused_creation_leaves_a_queued_acquisition_queued(mi, capi, tmp_path):
    from test_gpu_us_refusals import NA, NE, T, _acquire, _scene
    us, ui = _scene(mi)
    dev = us.device()
    ctx, lib = dev.ctx, dev.ctx.lib
    bad = _arrays(_lit(mi, tmp_path, "QQS"))
    d, plain = mi.DeviceBuffer(ctx, (NA, NE, T)), mi.DeviceBuffer(ctx, (NA, NE, T))
    try:
        ctx.synchronize()
        assert _acquire(lib, dev.handle, ui.us_params(us), plain, "pbrt_us_acquire_queue_dev") == 0
        assert lib.pbrt_ctx_synchronize(ctx.handle) == 0
        want, want_stats = plain.numpy(), ctx.stats()
        assert want.any() and want_stats["samples"] == NA * NE
        assert _acquire(lib, dev.handle, ui.us_params(us), d, "pbrt_us_acquire_queue_dev") == 0
        for accel, edit, code in ((4, None, E_INVALID), (0, _set("prims", 1, 9, "type"), E_UNSUPPORTED), (2, _set("prims", 0, 5, "material"), E_INVALID)):
            a = {k: (v.copy() if v is not None else None) for k, v in bad.items()}
            if edit:
                edit(a)
            rc, h, msg = _create(capi, ctx, a, accel)
            assert rc == code and not h.value, msg
        # the acquisition is finished by the synchronize, not by the refusals: its counters and its channel data are the plain run's
        assert lib.pbrt_ctx_synchronize(ctx.handle) == 0, lib.pbrt_last_error(ctx.handle)
        got_stats = ctx.stats()
        assert np.array_equal(d.numpy(), want)
        assert {k: got_stats[k] for k in ("samples", "segments", "passes", "live")} == {k: want_stats[k] for k in ("samples", "segments", "passes", "live")}
    finally:
        d.close()
        plain.close()
