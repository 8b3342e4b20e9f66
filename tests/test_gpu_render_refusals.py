"""The radiance driver's host decisions as a caller sees them (csrc/render_request.h; the arithmetic itself is held on the CPU by
tests/test_render_request_host.py): one refusal per argument rule through pbrt_render_radiance and pbrt_render_radiance_dev, each
with its code and its exact text, and after each a render that is bit-equal to the one before, with equal statistics; the pass and
plan bookkeeping pbrt_stats reports, as literals, on the Cornell box (fused brute-force kernels: probe pass, learnt plan, caller's
plan, uneven passes) and on testring.xml (trace / shade streams; a tent-filtered crop at the film's edge); and
pbrt_integrator_sample at one ray, one ray short of a region, a region, and one ray more, against the oracle.  Everything is
16 x 16 pixels or a few thousand rays."""
import ctypes as C

import numpy as np
import pytest

from conftest import oracle_render, scene_path

pytestmark = pytest.mark.gpu

E_INVALID = -1
RES, SPP = 16, 2
FLOAT_STATS = ("kernel_ms", "bounce_ms")

# the texts of the rules, in the order the driver looks at them (`out`: the host form's name for its output)
T_NULL = "invalid argument: cam && f && %s"
T_SIZES = "invalid argument: W > 0 && H > 0 && f->crop_w > 0 && f->crop_h > 0"
T_CROP = "invalid argument: (uint64_t)f->crop_x + f->crop_w <= W && (uint64_t)f->crop_y + f->crop_h <= H"
T_COUNTS = "invalid argument: f->spp > 0 && f->max_depth > 0 && f->filter <= PBRT_FILTER_GAUSSIAN"
T_FILM = "invalid argument: (uint64_t)W * H <= 0xffffffffull"


def _set(**kw):
    def edit(cam, fd):
        for k, v in kw.items():
            setattr(cam if k.startswith("film_") else fd, k, v)
    return edit


# (name, edit of the valid camera and film description, text).  Every case keeps a crop of 16 x 16 or less.
CASES = [
    ("film width 0", _set(film_w=0), T_SIZES),
    ("film height 0", _set(film_h=0), T_SIZES),
    ("crop x overflows 32 bits", _set(crop_x=0xFFFFFFF8), T_CROP),
    ("crop y overflows 32 bits", _set(crop_y=0xFFFFFFF8), T_CROP),
    ("crop beyond the film", _set(crop_x=1), T_CROP),
    ("no samples", _set(spp=0), T_COUNTS),
    ("no depth", _set(max_depth=0), T_COUNTS),
    ("filter beyond gaussian", _set(filter=3), T_COUNTS),
    ("film of 2^32 pixels", _set(film_w=65536, film_h=65536), T_FILM),
    # two rules broken: the earlier one speaks
    ("film width 0 and no samples", _set(film_w=0, spp=0), T_SIZES),
    ("crop beyond the film and filter", _set(crop_y=1, filter=7), T_CROP),
    ("no samples on a film of 2^32 pixels", _set(film_w=65536, film_h=65536, spp=0), T_COUNTS),
]


def _int_stats(ctx):
    return {k: v for k, v in ctx.stats().items() if k not in FLOAT_STATS}


def _call(sc, seed=3):
    integ, sens = sc.integrator(), sc.sensors()[0]
    return sens.camera(), integ._film_desc(sc, sens, seed, SPP)


def test_refusals_have_their_texts_and_leave_the_render_as_it_was(mi):
    sc = mi.load_file(scene_path("cbox.xml"), res=RES, spp=SPP)
    dev = sc.device()
    ctx, lib = dev.ctx, dev.ctx.lib
    d = mi.DeviceBuffer(ctx, (RES, RES, 3))
    out = np.empty((RES, RES, 3), np.float32)

    def host(cam, fd, o=out):
        return lib.pbrt_render_radiance(dev.handle, cam and C.byref(cam), fd and C.byref(fd), None if o is None else o.ctypes.data)

    def device(cam, fd, o=d):
        return lib.pbrt_render_radiance_dev(dev.handle, cam and C.byref(cam), fd and C.byref(fd), None if o is None else C.c_void_p(int(o.ptr)))

    def render_both():
        cam, fd = _call(sc)
        assert host(cam, fd) == 0, lib.pbrt_last_error(ctx.handle)
        st = _int_stats(ctx)
        assert device(cam, fd) == 0, lib.pbrt_last_error(ctx.handle)
        assert _int_stats(ctx) == st and np.array_equal(d.numpy(), out)
        return out.copy(), st

    try:
        assert host(*_call(sc)) == 0                   # (the scene's plan is learnt: every later render starts alike)
        want, want_st = render_both()
        assert want.mean() > 0
        for form, name_of_out in ((host, "out"), (device, "d_out")):
            for name, edit, text in CASES:
                cam, fd = _call(sc)
                edit(cam, fd)
                assert form(cam, fd) == E_INVALID, name
                assert lib.pbrt_last_error(ctx.handle).decode() == text, name
                got, st = render_both()
                assert np.array_equal(got, want) and st == want_st, name
            cam, fd = _call(sc)
            for name, args in (("cam", (None, fd)), ("f", (cam, None)), ("output", (cam, fd, None))):
                assert form(*args) == E_INVALID, name
                assert lib.pbrt_last_error(ctx.handle).decode() == T_NULL % name_of_out, name
            got, st = render_both()
            assert np.array_equal(got, want) and st == want_st
        assert lib.pbrt_render_radiance_dev(None, C.byref(cam), C.byref(fd), C.c_void_p(int(d.ptr))) == E_INVALID
        assert lib.pbrt_render_radiance(None, C.byref(cam), C.byref(fd), out.ctypes.data) == E_INVALID
    finally:
        d.close()


BOOK = ("passes", "fuse_plan", "plan_source", "bounce_launches", "pass_paths", "model_bytes", "bounce_model_bytes", "trace_model_bytes",
        "samples")


def _book(mi):
    st = mi.default_context().stats()
    got = {k: st[k] for k in BOOK}
    print(got)
    return got


def test_pass_and_plan_bookkeeping_of_the_fused_kernels(mi, capi):
    """cbox 16 x 16 at 16 samples, the smallest count at which the probe pass runs: 2 samples, then the other 14 in one pass"""
    sc = mi.load_file(scene_path("cbox.xml"), res=RES, spp=16)
    integ = sc.integrator()
    full = integ.render(sc, seed=5)
    assert _book(mi) == dict(passes=2, fuse_plan=0x1F, plan_source=capi.PLAN_PROBED, bounce_launches=3 + 1, pass_paths=4096,
                             model_bytes=121856, bounce_model_bytes=49152, trace_model_bytes=0, samples=4096)
    assert np.array_equal(integ.render(sc, seed=5), full)
    assert _book(mi) == dict(passes=1, fuse_plan=0x1F, plan_source=capi.PLAN_LEARNT, bounce_launches=1, pass_paths=4096,
                             model_bytes=113664, bounce_model_bytes=49152, trace_model_bytes=0, samples=4096)
    assert np.array_equal(integ.render(sc, seed=5, flags=capi.film_fuse_plan(0)), full)
    assert _book(mi) == dict(passes=1, fuse_plan=0, plan_source=capi.PLAN_CALLER, bounce_launches=6, pass_paths=4096,
                             model_bytes=1426944, bounce_model_bytes=1362432, trace_model_bytes=0, samples=4096)
    # 3 samples and 5 paths per pass: five passes of 3 samples and one of 1
    assert np.array_equal(integ.render(sc, seed=5, pass_paths=RES * RES * 3 + 5), full)
    assert _book(mi) == dict(passes=6, fuse_plan=0x1F, plan_source=capi.PLAN_LEARNT, bounce_launches=6, pass_paths=768,
                             model_bytes=154624, bounce_model_bytes=49152, trace_model_bytes=0, samples=4096)
    # on a scene nothing is known about: the probe pass of 2 samples, then the other 14 as 3, 3, 3, 3, 2
    sc2 = mi.load_file(scene_path("cbox.xml"), res=RES, spp=16)
    assert np.array_equal(sc2.integrator().render(sc2, seed=5, pass_paths=RES * RES * 3 + 5), full)
    assert _book(mi) == dict(passes=6, fuse_plan=0x1F, plan_source=capi.PLAN_PROBED, bounce_launches=3 + 5, pass_paths=768,
                             model_bytes=154624, bounce_model_bytes=49152, trace_model_bytes=0, samples=4096)


def test_pass_and_plan_bookkeeping_of_the_streams(mi, ob, capi):
    """testring.xml (a tree in LDS: k_trace / k_shade) at 16 x 16: two launches per bounce and pass, no plan, no probe pass"""
    sc = mi.load_file(scene_path("testring.xml"), res=RES, spp=16)
    integ = sc.integrator()
    depth = integ.max_depth
    full = integ.render(sc, seed=5)
    first = _book(mi)
    assert first == dict(passes=1, fuse_plan=0, plan_source=capi.PLAN_STREAMS, bounce_launches=2 * depth, pass_paths=4096,
                         model_bytes=1583604, bounce_model_bytes=1519092, trace_model_bytes=385996, samples=4096)
    assert np.array_equal(integ.render(sc, seed=5), full) and _book(mi) == first
    assert np.array_equal(integ.render(sc, seed=5, pass_paths=RES * RES * 3 + 5), full)
    assert _book(mi) == dict(first, passes=6, bounce_launches=6 * 2 * depth, pass_paths=768, model_bytes=1624564)
    # a tent-filtered 13 x 7 crop in the film's lower right corner: the rendered region is the crop and one pixel more on its two
    # inner sides
    sc.sensors()[0].film().rfilter = mi.ReconstructionFilter(mi.Properties("tent"))
    tent = integ.render(sc, seed=5)
    ref, _ = oracle_render(ob, sc, 5, 16)
    assert np.array_equal(tent, ref)
    crop = integ.render(sc, seed=5, crop=(RES - 13, RES - 7, 13, 7))
    st = _book(mi)
    assert np.array_equal(crop, tent[RES - 7:, RES - 13:])
    assert st["samples"] == 14 * 8 * 16 and st["pass_paths"] == 14 * 8 * 16 and st["passes"] == 1
    assert st["plan_source"] == capi.PLAN_STREAMS and st["bounce_launches"] == 2 * depth
    assert (st["model_bytes"], st["bounce_model_bytes"], st["trace_model_bytes"]) == (732600, 705636, 175324)


def _rays(n, lo, hi):
    rng = np.random.default_rng(11)
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("scene,region,lo,hi", [("cbox.xml", 512, -0.95, 0.95), ("testring.xml", 4096, -0.1, 0.1)])
def test_integrator_sample_around_a_region(mi, ob, scene, region, lo, hi):
    """the caller's rays fill one region but for a slot, exactly one, and one and a slot; a call without rays is no call"""
    sc = mi.load_file(scene_path(scene), res=RES, spp=1, max_depth=6)
    integ = sc.integrator()
    osc = ob.OracleScene.from_scene(sc)
    smp = mi.Sampler(mi.Properties("independent", dict(seed=9, sample_index=2, index_offset=7)))
    o, d = _rays(region + 1, lo, hi)
    tmax = np.full(region + 1, np.inf, np.float32)
    want = osc.integrator_sample(o, d, tmax, 7, 2, 9, integ.max_depth, integ.rr_depth)
    assert want.mean() > 1e-3
    for n in (1, region - 1, region, region + 1):
        rgb, _, _ = integ.sample(sc, smp, dict(o=o[:n], d=d[:n], maxt=tmax[:n]))
        assert rgb.shape == (n, 3) and np.array_equal(rgb, want[:n]), n
    dev = sc.device()
    ctx, lib = dev.ctx, dev.ctx.lib
    before = _int_stats(ctx)
    rgb = np.full((3, 4), 7.0, np.float32)
    a = lambda x: x.ctypes.data
    assert lib.pbrt_integrator_sample(dev.handle, 0, a(o), a(d), a(tmax), 7, 2, 9, 6, 5, a(rgb)) == 0
    assert (rgb == 7.0).all() and _int_stats(ctx) == before
