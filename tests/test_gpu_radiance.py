"""GPU parity, radiance mode: the HIP wavefront path (through the C-ABI) against the CPU oracle on the
same scene / seed, against committed golden images, and -- at BASELINE size -- through size-independent
properties.

Tolerance: BASELINE.json's north star states per-pixel L2 <= 1e-3 vs the CPU reference.  Under the numeric
contract the radiance kernels reproduce the oracle bit for bit on gfx950, so the tests assert
exact equality where only {+,-,*,/,sqrt,fma} are involved and keep the 1e-3 bound as the stated contract."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, oracle_render, scene_path

pytestmark = pytest.mark.gpu
TOL_L2 = 1e-3   # north_star: per-pixel L2 <= 1e-3 vs CPU reference


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


@pytest.mark.parametrize("res,spp,seed", [(64, 16, 0), (64, 16, 1), (96, 8, 2), (33, 5, 3)])
def test_cbox_matches_oracle(mi, ob, res, spp, seed):
    sc = mi.load_file(scene_path("cbox.xml"), res=res, spp=spp)
    img = mi.render(sc, seed=seed)
    ref, st = oracle_render(ob, sc, seed, spp)
    assert img.shape == (res, res, 3) and np.isfinite(img).all()
    assert rmse(img, ref) <= TOL_L2
    assert np.array_equal(img, ref), f"not bit-exact: {np.mean(img != ref):.2e} of values differ"
    gst = mi.default_context().stats()
    assert gst["segments"] == st["segments"] and gst["shadow_rays"] == st["shadow_rays"]
    assert gst["samples"] == res * res * spp


@pytest.mark.parametrize("scene,name", [("cbox.xml", "cbox_32x32_spp8_seed0.npy"), ("cone_room.xml", "cone_room_32x32_spp8_seed0.npy")])
def test_golden_images(mi, scene, name):
    """committed oracle films: the Cornell box (brute-force kernels), and a room with a diffuse and a glass analytic cone
    and a mirror sphere (the brute-force variant that carries the cone code)"""
    g = np.load(os.path.join(GOLDEN, name))
    sc = mi.load_file(scene_path(scene), res=32, spp=8)
    img = mi.render(sc, seed=0)
    assert rmse(img, g) <= TOL_L2 and np.array_equal(img, g)


def test_simple_scene_direct_integrator_bvh(mi, ob, capi):
    """BASELINE config 1: scenes/simple.xml 64x64, 4 spp (teapot, 2256 triangles -> BVH staged in LDS)."""
    sc = mi.load_file(scene_path("simple.xml"), res=64, spp=4)
    img = mi.render(sc, seed=0)
    ref, st = oracle_render(ob, sc, 0, 4)                              # the oracle's own (median-split) BVH
    assert np.array_equal(img, ref) and img.max() > 0.1
    brute, _ = oracle_render(ob, sc, 0, 4, accel=capi.ACCEL_BRUTE)     # and by brute force: independent of any BVH
    assert np.allclose(img, brute, rtol=1e-5, atol=1e-6)
    g = np.load(os.path.join(GOLDEN, "simple_64x64_spp4_seed0.npy"))
    assert np.array_equal(img, g)
    assert mi.default_context().stats()["segments"] == st["segments"]


@pytest.mark.parametrize("accel", ["auto", "bvh_forced_on_cbox", "brute_forced_on_ring"])
def test_accel_variants_agree(mi, ob, capi, accel):
    if accel == "bvh_forced_on_cbox":
        sc = mi.load_file(scene_path("cbox.xml"), res=48, spp=4)
        sc.accel = capi.ACCEL_BVH
    elif accel == "brute_forced_on_ring":
        sc = mi.load_file(scene_path("testring.xml"), res=24, spp=2)
        sc.accel = capi.ACCEL_BRUTE
    else:
        sc = mi.load_file(scene_path("testring.xml"), res=64, spp=8)
    spp = sc.sensors()[0].sampler().sample_count
    img = mi.render(sc, seed=5)
    # the accelerator is part of the numeric contract (brute force: ratio-ranked candidates + occluder list for
    # shadow segments; BVH: rounded-t ranking, ties by primitive id): same accelerator -> bit-identical ...
    ref, _ = oracle_render(ob, sc, 5, spp, accel=sc.accel)
    assert np.array_equal(img, ref) and img.mean() > 0
    # ... and the other accelerator agrees except on measure-zero ties
    other, _ = oracle_render(ob, sc, 5, spp, accel=capi.ACCEL_BRUTE if sc.accel != capi.ACCEL_BRUTE else capi.ACCEL_BVH)
    assert np.allclose(img, other, rtol=1e-5, atol=1e-6)


def test_filters_box_and_gaussian(mi, ob):
    for filt, exact in (("box", True), ("gaussian", False)):
        sc = mi.load_file(scene_path("cbox.xml"), res=40, spp=6)
        sc.sensors()[0].film().rfilter = mi.ReconstructionFilter(mi.Properties(filt))
        img = mi.render(sc, seed=2)
        ref, _ = oracle_render(ob, sc, 2, 6)
        assert rmse(img, ref) <= TOL_L2
        if exact:
            assert np.array_equal(img, ref)
        else:   # the gaussian weight uses expf: ocml vs libm differ in the last ulp
            assert np.allclose(img, ref, rtol=1e-5, atol=1e-7)


def test_crop_sample_offset_raw_and_pass_size(mi, ob):
    sc = mi.load_file(scene_path("cbox.xml"), res=48, spp=12)
    integ = sc.integrator()
    full = integ.render(sc, seed=4, spp=12)
    # (a) results do not depend on how many paths are kept in flight per pass
    assert np.array_equal(integ.render(sc, seed=4, spp=12, pass_paths=48 * 48 * 5), full)
    assert np.array_equal(integ.render(sc, seed=4, spp=12, pass_paths=1000), full)
    # (b) a crop equals the slice of the full film (halo rows are rendered redundantly)
    crop = integ.render(sc, seed=4, spp=12, crop=(7, 11, 20, 9))
    assert np.array_equal(crop, full[11:20, 7:27])
    # (c) sample ranges add up (un-normalised accumulators), against the oracle's too
    r0 = integ.render(sc, seed=4, spp=8, raw=True)
    r1 = integ.render(sc, seed=4, spp=4, sample_offset=8, raw=True)
    rr = integ.render(sc, seed=4, spp=12, raw=True)
    assert np.allclose(r0 + r1, rr, rtol=1e-6, atol=1e-7)
    ref_raw, _ = oracle_render(ob, sc, 4, 4, sample_offset=8, raw=True)
    assert np.array_equal(r1, ref_raw)
    assert np.array_equal(rr[..., :3] * (np.float32(1.0) / rr[..., 3:4]), full)      # resolve multiplies by 1/w


@pytest.mark.parametrize("filt", ["tent", "box", "gaussian"])
def test_bvh_scene_crops_and_passes_with_tiled_pixel_order(mi, ob, filt):
    """BVH kernels walk the rendered region in 8-row bands, column by column (region_index): regions whose height is
    not a multiple of 8 keep their last rows in row-major order, and the film gather must use the same index --
    crops of every alignment equal the slice of the full film, and the full film equals the oracle's"""
    sc = mi.load_file(scene_path("testring.xml"), res=45, spp=3)
    sc.sensors()[0].film().rfilter = mi.ReconstructionFilter(mi.Properties(filt))
    integ = sc.integrator()
    full = integ.render(sc, seed=6, spp=3)
    ref, _ = oracle_render(ob, sc, 6, 3)
    if filt == "gaussian":   # expf in the filter weight: ocml vs libm, last ulp
        assert np.allclose(full, ref, rtol=1e-5, atol=1e-7) and full.mean() > 0
    else:
        assert np.array_equal(full, ref) and full.mean() > 0
    for crop in ((0, 0, 45, 45), (3, 5, 29, 13), (0, 37, 45, 8), (10, 0, 7, 7), (40, 1, 5, 44), (0, 8, 45, 16), (11, 19, 1, 1)):
        x, y, w, h = crop
        assert np.array_equal(integ.render(sc, seed=6, spp=3, crop=crop), full[y:y + h, x:x + w]), crop
    assert np.array_equal(integ.render(sc, seed=6, spp=3, pass_paths=45 * 45 + 17), full)       # passes of 1 sample + change


def test_non_square_film_and_camera(mi, ob):
    sc = mi.load_dict({
        "type": "scene", "integrator": {"type": "path", "max_depth": 4},
        "sensor": {"type": "perspective", "fov": 50, "fov_axis": "x", "near_clip": 0.01, "far_clip": 50,
                   "to_world": mi.ScalarTransform4f().look_at([1.5, 0.4, 3.5], [0, -0.2, 0], [0, 1, 0]),
                   "film": {"type": "hdrfilm", "width": 70, "height": 37, "rfilter": {"type": "tent"}},
                   "sampler": {"type": "independent", "sample_count": 5}},
        "floor": {"type": "rectangle", "to_world": mi.ScalarTransform4f().translate([0, -1, 0]).rotate([1, 0, 0], -90).scale(3),
                  "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.6, 0.5, 0.4]}}},
        "ball": {"type": "sphere", "center": [0.2, -0.5, 0.1], "radius": 0.5, "bsdf": {"type": "dielectric"}},
        "lamp": {"type": "rectangle", "to_world": mi.ScalarTransform4f().translate([0, 2, 0]).rotate([1, 0, 0], 90).scale(0.7),
                 "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [4, 5, 6]}}},
        "bulb": {"type": "point", "position": [-2, 1, 1], "intensity": {"type": "rgb", "value": [3, 3, 3]}},
    })
    img = mi.render(sc, seed=9)
    ref, _ = oracle_render(ob, sc, 9, 5)
    assert img.shape == (37, 70, 3) and np.array_equal(img, ref) and img.max() > 0.5


def test_unbounded_depth_and_rr(mi, ob):
    """Mitsuba max_depth = -1: paths end by Russian roulette / escape only."""
    sc = mi.load_file(scene_path("cbox.xml"), res=24, spp=4, max_depth=-1)
    assert sc.integrator().max_depth == 0xFFFFFFFF
    sc.integrator().max_depth = 200        # finite but far beyond any surviving path
    img = mi.render(sc, seed=1)
    ref, _ = oracle_render(ob, sc, 1, 4)
    assert np.array_equal(img, ref)


@pytest.mark.parametrize("max_depth", [1, 2, 3, 40, -1])
def test_bvh_scene_depth_budgets(mi, ob, max_depth):
    """the k_trace / k_shade streams with the smallest depth budgets (1: emitters seen directly, 2: one next-event estimate and
    the emitter lookup of the second bounce), with a budget above 32 (the host polls the live count every 8 bounces and stops
    early: the shadow rays of the last shaded bounce still get their trace + shade) and unbounded (Mitsuba max_depth = -1)"""
    sc = mi.load_file(scene_path("testring.xml"), res=48, spp=3, max_depth=max_depth)
    img = mi.render(sc, seed=6)
    st = mi.default_context().stats()
    ref, _ = oracle_render(ob, sc, 6, 3)
    assert np.array_equal(img, ref) and (img.mean() > 0 or max_depth == 1)   # (the camera does not see the emitter itself)
    if max_depth in (40, -1):
        assert 2 * 8 <= st["bounce_launches"] <= 2 * 33      # stopped by the poll, not by the budget
    else:
        assert st["bounce_launches"] == 2 * max_depth


@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (65, 63), (64, 64), (17, 241), (23, 359)])
def test_bvh_streams_at_the_edges_of_a_region(mi, ob, w, h):
    """the scaffold k_shade shares with k_us_shade (shade_walk) at the path counts where it can go wrong, one sample per pixel and
    regions of 4096 slots: a single lane (1 path), one chunk (64), one slot short of a region (4095), exactly one region (4096), a
    second region with one path (4097: three of its four waves find no chunk on entry) and two full regions plus one chunk and one
    lane (8257).  max_depth 8 lies beyond rr_depth, so Russian roulette ends paths that have just sent a shadow ray: the records at
    the back of a region.  Box filter: the rendered region is the film."""
    sc = mi.load_file(scene_path("testring.xml"), res=64, spp=1, max_depth=8)
    film = sc.sensors()[0].film()
    film.width, film.height, film.crop = w, h, (0, 0, w, h)
    film.rfilter = mi.ReconstructionFilter(mi.Properties("box"))
    img = mi.render(sc, seed=5)
    st = mi.default_context().stats()
    ref, _ = oracle_render(ob, sc, 5, 1)
    assert img.shape == (h, w, 3) and np.array_equal(img, ref)
    assert st["bounce_launches"] == 2 * 8      # no poll at a budget of 32 bounces or fewer: k_trace + k_shade per bounce
    assert img.mean() > 0 or w * h < 4095


def test_material_update_reaches_the_device(mi, ob):
    sc = mi.load_file(scene_path("cbox.xml"), res=24, spp=4)
    a = mi.render(sc, seed=0)
    params = mi.traverse(sc)
    params["left.bsdf.reflectance"] = np.array([0.9, 0.1, 0.9])
    params.update()
    b = mi.render(sc, seed=0)
    ref, _ = oracle_render(ob, sc, 0, 4)
    assert not np.array_equal(a, b) and np.array_equal(b, ref)


def _render_rays(mi, sc, seed, s_idx):
    """the camera rays of sample s_idx of every pixel, as render generates them: jitter = rng4(pixel, sample, 0, seed).xy
    (the counter-based generator restated in tests/pinned_util.py), through Sensor.sample_ray"""
    import sys
    from conftest import GOLDEN
    sys.path.insert(0, GOLDEN)
    import pinned_util as rt
    sens = sc.sensors()[0]
    W, H = sens.film().size()
    jit = np.array([rt.rng4(p, s_idx, 0, seed)[:2] for p in range(W * H)], np.float32)
    px = np.arange(W * H, dtype=np.int64)
    fx = (px % W).astype(np.float32) + jit[:, 0]
    fy = (px // W).astype(np.float32) + jit[:, 1]
    pos = np.stack([fx / np.float32(W), fy / np.float32(H)], axis=1).astype(np.float32)
    ray, _ = sens.sample_ray(0.0, 0.0, pos, None)
    return ray


@pytest.mark.parametrize("scene,kw", [("cbox.xml", dict(res=24, max_depth=6)), ("cbox.xml", dict(res=16, max_depth=-1)),
                                      ("testring.xml", dict(res=40))])
def test_integrator_sample_on_caller_rays(mi, ob, scene, kw):
    """Integrator.sample(scene, sampler, ray, ...) (CustomIntegrator.py:52): radiance along explicit rays.  Against its
    oracle twin (key mode 1: keys (index_offset + i, sample_index), tmax carried by the first bounce, brute force and
    BVH, bounded and unbounded depth), and against the film: the rays of sample s of every pixel, in pixel order, give
    the 1-spp box-filter film of sample s bit for bit."""
    sc = mi.load_file(scene_path(scene), spp=1, **({"rfilter": "box"} if scene == "cbox.xml" else {}), **kw)
    if scene != "cbox.xml":
        sc.sensors()[0].film().rfilter = mi.ReconstructionFilter(mi.Properties("box"))
    integ, sens = sc.integrator(), sc.sensors()[0]
    if kw.get("max_depth") == -1:
        integ.max_depth = 60                      # beyond any surviving path; exercises the polling of the live count
    W, H = sens.film().size()
    smp = mi.Sampler(mi.Properties("independent", dict(seed=9, sample_index=2)))
    ray = _render_rays(mi, sc, 9, 2)
    rgb, valid, aovs = integ.sample(sc, smp, ray)
    assert rgb.shape == (W * H, 3) and np.isfinite(rgb).all() and rgb.mean() > 1e-3 and aovs == [] and valid.all()
    osc = ob.OracleScene.from_scene(sc)
    want = osc.integrator_sample(ray["o"], ray["d"], ray["maxt"], 0, 2, 9, integ.max_depth, integ.rr_depth)
    assert np.array_equal(rgb, want)
    film = integ.render(sc, seed=9, spp=1, sample_offset=2)
    assert np.array_equal(rgb.reshape(H, W, 3), film)
    # other keys: an index offset moves every ray to another stream; a finite maxt cuts the first segment
    smp2 = mi.Sampler(mi.Properties("independent", dict(seed=9, sample_index=2, index_offset=1000)))
    rgb2, _, _ = integ.sample(sc, smp2, ray)
    assert np.array_equal(rgb2, osc.integrator_sample(ray["o"], ray["d"], ray["maxt"], 1000, 2, 9, integ.max_depth, integ.rr_depth))
    assert not np.array_equal(rgb2, rgb)
    short = dict(ray, maxt=np.full(W * H, 0.5, np.float32))
    rgb3, _, _ = integ.sample(sc, smp, short)
    assert np.array_equal(rgb3, osc.integrator_sample(short["o"], short["d"], short["maxt"], 0, 2, 9, integ.max_depth, integ.rr_depth))
    assert rgb3.sum() < rgb.sum()


# ---- BASELINE size (cbox 512 x 512 x 256 spp): size-independent properties ---------------------------
@pytest.fixture(scope="module")
def cbox_full(mi):
    sc = mi.load_file(scene_path("cbox.xml"), res=512, spp=256)
    img = mi.render(sc, seed=0)
    return sc, img, mi.default_context().stats()


def test_full_size_determinism_and_statistics(mi, cbox_full):
    sc, img, st = cbox_full
    assert st["samples"] == 512 * 512 * 256 and st["passes"] >= 1
    assert np.isfinite(img).all() and img.min() >= 0
    again = mi.render(sc, seed=0)
    assert np.array_equal(img, again)
    # every path performs between 1 and max_depth intersections
    assert 1.0 <= st["segments"] / st["samples"] <= 6.0


def test_full_size_linearity_in_emitted_radiance(mi, cbox_full):
    sc, img, _ = cbox_full
    sc2 = mi.load_file(scene_path("cbox.xml"), res=512, spp=256)
    p = mi.traverse(sc2)
    p["luminaire.emitter.radiance"] = np.array([2.0, 2.0, 2.0])   # x2: exact in binary floating point
    p.update()
    img2 = mi.render(sc2, seed=0)
    assert np.array_equal(img2, 2.0 * img)


def test_full_size_matches_oracle_on_a_band(mi, ob, cbox_full):
    """The oracle finishes 8 rows x 512 x 256 spp in seconds; the GPU film must agree there bit for bit."""
    sc, img, _ = cbox_full
    ref, _ = oracle_render(ob, sc, 0, 256, crop=(0, 300, 512, 8), n_threads=16)
    assert rmse(img[300:308], ref) <= TOL_L2
    assert np.array_equal(img[300:308], ref)


def test_full_size_energy_sanity(cbox_full):
    _, img, _ = cbox_full
    # the luminaire (y = 0.99, |x|,|z| <= 0.25) projects to rows 67..89, columns 211..301: radiance 1 seen directly
    lum = img[70:86, 220:292]
    assert 0.99 <= np.median(lum) <= 1.2
    assert img[:, :170].mean(axis=(0, 1)).argmax() == 1   # left third is dominated by the green wall
    assert img[:, 342:].mean(axis=(0, 1)).argmax() == 0   # right third by the red wall


def diag_renders(mi, capi, scene, load_kw, renders, accel=None):
    """the same scene through the DIAGNOSTIC build of the library (libpbrt_hip_diag.so: the launch structures the product build
    leaves out): -> [(film, stats)] for every kwargs dict in `renders`"""
    out = []
    with capi.use_library(capi.DIAG_LIB_PATH):
        sc = mi.load_file(scene_path(scene), **load_kw)
        if accel is not None:
            sc.accel = accel
        integ = sc.integrator()
        for kw in renders:
            img = integ.render(sc, **kw)
            out.append((img, mi.default_context().stats()))
        sc._dev = None  # the handle belongs to the diagnostic library's context
    return out


def test_bvh_scene_at_scale_streams_and_the_fused_kernels(mi, ob, capi):
    """the ring scene with a few hundred regions.  Product path: a bounce is k_trace (stream of ray queries, several regions per
    workgroup) + k_shade (per-wave lists, slot reservation): same film with other pass sizes, with the tree in global memory, and
    equal to the oracle on a band.  Diagnostic build: the fused bounce kernels (PBRT_FILM_NO_HIT_POOL), with and without the
    re-dealing of the live paths before bounces >= 2 -- same film, same segments, shadow rays and per-depth path counts."""
    sc = mi.load_file(scene_path("testring.xml"), res=320, spp=12)
    integ = sc.integrator()
    img = integ.render(sc, seed=2, spp=12)
    st = mi.default_context().stats()
    assert st["plan_source"] == capi.PLAN_STREAMS and st["fuse_plan"] == 0 and st["workspace_bytes"] > 0
    assert np.array_equal(img, integ.render(sc, seed=2, spp=12, pass_paths=300_000))      # 6 passes of 2 samples
    assert mi.default_context().stats()["passes"] == 6
    assert np.array_equal(img, integ.render(sc, seed=2, spp=12))                           # slot order is not deterministic
    band = (0, 150, 320, 24)
    ref, _ = oracle_render(ob, sc, 2, 12, crop=band)
    assert np.array_equal(img[150:174], ref) and img.mean() > 0
    assert st["samples"] == 320 * 320 * 12 and st["live"][0] == st["samples"] and st["live"][2] < st["live"][1] < st["live"][0]
    scg = mi.load_file(scene_path("testring.xml"), res=320, spp=12)
    scg.accel = capi.ACCEL_BVH_GLOBAL
    assert np.array_equal(scg.integrator().render(scg, seed=2, spp=12), img)
    with pytest.raises(RuntimeError, match="diagnostic"):   # the product build does not carry the fused BVH kernels
        integ.render(sc, seed=2, spp=12, flags=capi.FILM_NO_HIT_POOL)
    for accel in (None, capi.ACCEL_BVH_GLOBAL):
        rs = diag_renders(mi, capi, "testring.xml", dict(res=320, spp=12),
                          [dict(seed=2, spp=12), dict(seed=2, spp=12, flags=capi.FILM_NO_HIT_POOL),
                           dict(seed=2, spp=12, flags=capi.FILM_NO_HIT_POOL | capi.FILM_NO_REPACK)], accel=accel)
        for im, s0 in rs:
            assert np.array_equal(im, img)
            assert list(s0["live"]) == list(st["live"]) and s0["segments"] == st["segments"] and s0["shadow_rays"] == st["shadow_rays"]


def test_bvh_with_a_short_last_pass(mi, ob, capi):
    """spp that does not split into equal passes: 13 samples at 300 000 paths per pass are 6 passes of 2 and one of 1,
    so the last pass launches half the regions the workspace was sized for (the queue of a k_trace workgroup must stay inside the
    regions that pass launched; an odd max_depth leaves survivors in both counter arrays).  Diagnostic build: the fused kernels'
    re-dealing of the live paths under the same conditions."""
    sc = mi.load_file(scene_path("testring.xml"), res=320, spp=13, max_depth=7)
    integ = sc.integrator()
    img = integ.render(sc, seed=3, spp=13)
    short = integ.render(sc, seed=3, spp=13, pass_paths=300_000)
    assert np.array_equal(short, img)
    assert mi.default_context().stats()["passes"] == 7
    band = (0, 160, 320, 16)
    ref, _ = oracle_render(ob, sc, 3, 13, crop=band)
    assert np.array_equal(short[160:176], ref)
    rs = diag_renders(mi, capi, "testring.xml", dict(res=320, spp=13, max_depth=7),
                      [dict(seed=3, spp=13, pass_paths=300_000, flags=capi.FILM_NO_HIT_POOL),
                       dict(seed=3, spp=13, pass_paths=300_000, flags=capi.FILM_NO_HIT_POOL | capi.FILM_NO_REPACK)])
    assert all(np.array_equal(im, img) for im, _ in rs)


def test_first_render_of_a_scene_probes_its_launch_plan(mi, capi):
    """the launch plan of a brute-force scene is state of the scene: the FIRST render (plan left to the library, >= 16 spp) spends
    a 2-spp probe pass on learning it, later renders use what the previous one measured.  Either way the film, the per-depth path
    counts, the segments and the shadow rays are those of one launch per bounce; pbrt_stats says which plan ran and why."""
    for scene, kw in (("cbox.xml", dict(res=40)), ("cone_room.xml", dict(res=32))):   # both brute-force kernel variants
        for spp in (16, 37):
            ref_sc = mi.load_file(scene_path(scene), spp=spp, **kw)
            base = ref_sc.integrator().render(ref_sc, seed=9, spp=spp, flags=capi.film_fuse_plan(0))
            st0 = mi.default_context().stats()
            assert st0["plan_source"] == capi.PLAN_CALLER and st0["fuse_plan"] == 0
            sc = mi.load_file(scene_path(scene), spp=spp, **kw)   # a freshly loaded scene: no plan yet
            integ = sc.integrator()
            first = integ.render(sc, seed=9, spp=spp)
            st1 = mi.default_context().stats()
            second = integ.render(sc, seed=9, spp=spp)
            st2 = mi.default_context().stats()
            assert np.array_equal(first, base) and np.array_equal(second, base)
            for st in (st1, st2):
                assert list(st["live"]) == list(st0["live"]) and st["segments"] == st0["segments"] and st["shadow_rays"] == st0["shadow_rays"]
            assert st1["plan_source"] == capi.PLAN_PROBED and st2["plan_source"] == capi.PLAN_LEARNT
            assert st1["passes"] == st2["passes"] + 1 and st1["fuse_plan"] == st2["fuse_plan"] != 0
        few = mi.load_file(scene_path(scene), spp=6, **kw)   # too few samples for a probe: the default plan (pairs)
        few.integrator().render(few, seed=9, spp=6)
        st = mi.default_context().stats()
        assert st["plan_source"] == capi.PLAN_DEFAULT and st["fuse_plan"] == 0x15


@pytest.mark.parametrize("scene,kw", [("cbox.xml", dict(res=48, max_depth=6)), ("cbox.xml", dict(res=32, max_depth=5)),
                                      ("cbox.xml", dict(res=24, max_depth=2)), ("cone_room.xml", dict(res=32))])
def test_fused_bounce_launches_change_nothing(mi, ob, capi, scene, kw):
    """a launch of the brute-force kernels may walk two bounces of its paths in registers (include/pbrt_hip.h
    PBRT_FILM_FUSE_PLAN: bit d = the launch at depth d also does bounce d + 1): every plan gives the film of one launch per
    bounce, bit for bit, the same per-depth path counts, and the oracle's film -- even and odd depth budgets, a budget
    of 2 (nothing left to fuse after the emitter lookup), both brute-force kernel variants (cone_room: the _BIG one)"""
    sc = mi.load_file(scene_path(scene), spp=6, **kw)
    integ = sc.integrator()
    ctx = mi.default_context()
    base = integ.render(sc, seed=5, spp=6, flags=capi.film_fuse_plan(0))
    st0 = ctx.stats()
    ref, _ = oracle_render(ob, sc, 5, 6)
    assert np.array_equal(base, ref)
    for plan in (0x1, 0x2, 0x3, 0x4, 0x5, 0x7, 0xA, 0xE, 0x15, 0x1B, 0x1F, 0xFF):   # pairs, triples, chains of 4, 5 and 6 bounces
        img = integ.render(sc, seed=5, spp=6, flags=capi.film_fuse_plan(plan))
        st = ctx.stats()
        assert np.array_equal(img, base), hex(plan)
        assert list(st["live"]) == list(st0["live"]) and st["segments"] == st0["segments"] and st["shadow_rays"] == st0["shadow_rays"]
        assert st["bounce_launches"] <= st0["bounce_launches"] and st["bounce_model_bytes"] <= st0["bounce_model_bytes"]
    md = integ.max_depth
    img = integ.render(sc, seed=5, spp=6, flags=capi.film_fuse_plan(0xFF))
    assert ctx.stats()["bounce_launches"] == ctx.stats()["passes"] * -(-md // 6)   # six bounces per launch
    # the library's own choice: pairs for the first render of a scene, then the plan learnt from its path survival
    assert np.array_equal(integ.render(sc, seed=5, spp=6), base) and np.array_equal(integ.render(sc, seed=5, spp=6), base)
    assert list(ctx.stats()["live"]) == list(st0["live"])
    # the launch structures that lost their A/B live in the diagnostic build only
    with pytest.raises(RuntimeError, match="diagnostic"):
        integ.render(sc, seed=5, spp=6, flags=capi.FILM_REGEN)
    # k_walk: one launch walks every remaining bounce of a pass (PBRT_FILM_WALK_FROM), with and without a fused first trip;
    # k_regen: persistent waves, every lane walks one path to its end and then takes the next one (PBRT_FILM_REGEN): no path
    # state in memory, one launch per pass -- and still the same film, segments, shadow rays and per-depth path counts
    walks = [dict(seed=5, spp=6, flags=capi.film_fuse_plan(plan) | capi.film_walk_from(walk))
             for plan, walk in ((0x0, 0), (0x1, 0), (0x0, 1), (0x1, 2), (0x4, 2), (0x0, 3))]
    regens = [dict(seed=5, spp=6, flags=capi.FILM_REGEN, pass_paths=pp) for pp in (0, 3 * base.shape[0] * base.shape[1] + 5)]
    rs = diag_renders(mi, capi, scene, dict(spp=6, **kw), walks + regens)
    for k, (img, st) in enumerate(rs):
        assert np.array_equal(img, base), k
        assert list(st["live"]) == list(st0["live"]) and st["segments"] == st0["segments"] and st["shadow_rays"] == st0["shadow_rays"]
        if k >= len(walks):
            assert st["bounce_launches"] == st["passes"] and st["bounce_model_bytes"] == 12 * st["samples"]
    # k_chain_pair (diagnostic build, PBRT_PAIR_MERGE = merge bounce): the whole path in one launch, two 64-path tiles per wave whose
    # survivors share the wave from the merge bounce on -- same film and counts for every merge bounce, also with a short last pass
    if md <= 6:
        import os
        try:
            for m in range(1, md):
                os.environ["PBRT_PAIR_MERGE"] = str(m)
                pairs = [dict(seed=5, spp=6, flags=capi.film_fuse_plan(0x3F), pass_paths=pp) for pp in (0, 4 * base.shape[0] * base.shape[1] + 7)]
                for img, st in diag_renders(mi, capi, scene, dict(spp=6, **kw), pairs):
                    assert np.array_equal(img, base), m
                    assert list(st["live"]) == list(st0["live"]) and st["segments"] == st0["segments"] and st["shadow_rays"] == st0["shadow_rays"]
                    assert st["bounce_launches"] == st["passes"]
        finally:
            os.environ.pop("PBRT_PAIR_MERGE", None)
    # passes: a short last pass and the fused first launch
    assert np.array_equal(integ.render(sc, seed=5, spp=6, pass_paths=4 * base.shape[0] * base.shape[1] + 7, flags=capi.film_fuse_plan(0x5)), base)


def _child_films(env, scene, res, spp, seed, pass_paths):
    """films (sha256) and launch counts of renders in a CHILD process (the PBRT_WF_* switches are read once per process)"""
    import os, subprocess, sys
    child = ("import hashlib, sys; sys.path.insert(0, %r); import pbrt_amd as mi\n"
             "sc = mi.load_file(%r, res=%d, spp=%d)\n"
             "for pp in %r:\n"
             "    img = sc.integrator().render(sc, seed=%d, spp=%d, pass_paths=pp); st = mi.default_context().stats()\n"
             "    print('film', hashlib.sha256(img.tobytes()).hexdigest(), st['passes'], st['bounce_launches'])\n"
             % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), scene_path(scene), res, spp, tuple(pass_paths), seed, spp))
    r = subprocess.run([sys.executable, "-c", child], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("film")]


def test_bvh_passes_split_over_cu_masked_streams_render_the_same_film(mi):
    """PBRT_WF_SPLIT=s:parts (opt-in, measured slower: DESIGN.md section 6): k_trace and k_shade run on two streams with disjoint CU
    masks, the regions of a pass go through them in `parts` sets one phase apart -- a pass of 288 regions and a two-pass render give
    the film of the one-stream default, and the launch count says the pipeline really ran"""
    import hashlib
    sc = mi.load_file(scene_path("testring.xml"), res=384, spp=8)
    want = [hashlib.sha256(sc.integrator().render(sc, seed=3, spp=8, pass_paths=pp).tobytes()).hexdigest() for pp in (0, 700_000)]
    md = sc.integrator().max_depth
    for spec, parts in (("2:2", 2), ("3:4", 4)):
        got = _child_films(dict(PBRT_WF_SPLIT=spec), "testring.xml", 384, 8, 3, (0, 700_000))
        assert [g[0] for g in got] == want, spec
        assert int(got[0][1]) == 1 and int(got[0][2]) == 2 * parts * md, spec   # one pass: parts x (k_trace + k_shade) per bounce
        assert int(got[1][1]) == 2


@pytest.mark.parametrize("scene,res,spp", [("testring.xml", 201, 5), ("bunny.xml", 97, 3)])
def test_camera_rays_walked_per_tile_or_per_lane_give_the_same_film(mi, ob, scene, res, spp):
    """bounce 0 of a BVH scene: k_trace_primary walks the tree once per 64-path tile (wave-uniform node, every lane tests the four
    child boxes and every primitive of a leaf with its own ray); PBRT_WF_PACKET=0 keeps the per-lane traversal of k_trace.  Same
    film either way (tree in LDS and in global memory; a film whose pixel count is no multiple of 64, a short last pass), and the
    oracle's"""
    import hashlib
    sc = mi.load_file(scene_path(scene), res=res, spp=spp)
    pps = (0, 2 * res * res + 17)
    imgs = [sc.integrator().render(sc, seed=11, spp=spp, pass_paths=pp) for pp in pps]
    want = [hashlib.sha256(i.tobytes()).hexdigest() for i in imgs]
    assert want[0] == want[1]
    got = _child_films(dict(PBRT_WF_PACKET="0"), scene, res, spp, 11, pps)
    assert [g[0] for g in got] == want
    band = (0, res // 2, res, 8)
    ref, _ = oracle_render(ob, sc, 11, spp, crop=band)
    assert np.array_equal(imgs[0][res // 2:res // 2 + 8], ref) and imgs[0].mean() > 0


def test_render_larger_than_a_pass_with_an_odd_pixel_count(mi, ob, capi):
    """more samples than the 64 Mi paths of a pass, on a film whose pixel count divides nothing: 521 x 521 x 256 = 69.5 M samples run
    as two equal passes of 128 spp; a band of the film equals the oracle's render of that crop (the crop render redoes the halo rows).
    With the plan that walks every bounce in one launch no path state is allocated: the workspace stays far below the 8 GB the
    ping-pong state of 64 Mi paths would take."""
    sc = mi.load_file(scene_path("cbox.xml"), res=521, spp=256)
    integ = sc.integrator()
    integ.render(sc, seed=4, spp=1)
    ws0 = mi.default_context().stats()["workspace_bytes"]   # (the workspace of a context only grows: earlier renders count)
    img = integ.render(sc, seed=4, spp=256, flags=capi.film_fuse_plan(0x3F))
    st = mi.default_context().stats()
    H, W = img.shape[:2]
    assert st["samples"] == W * H * 256 > (64 << 20) and st["passes"] == 2 and st["pass_paths"] == W * H * 128
    assert st["bounce_launches"] == 2 and st["workspace_bytes"] - ws0 < 3 * 10**9
    y0 = H // 2
    ref, _ = oracle_render(ob, sc, 4, 256, crop=(0, y0, W, 8))
    assert np.array_equal(img[y0:y0 + 8], ref)
