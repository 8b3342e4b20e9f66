"""k_path (csrc/kernels_radiance.h): a pass of camera paths of an ACCEL_K_BRUTE scene whose every bounce one launch walks
(max_depth <= MAX_CHAIN = 6 and a fuse plan that chains them all) runs a kernel without survivor compaction -- no barrier after the
table staging, one 1 KiB record store per wave after the bounce loop, statistics through workgroup counters in LDS, an argument
block of its own.  Same camera start, keep word, bounce_step and RNG keys as k_bounce<true, .., 2>, so every render here equals
the same render with PBRT_FILM_NO_PATH_KERNEL (that pass through k_bounce) bit for bit: film, segments, shadow rays, live paths per
depth, launches.  Where it is cheap the film is held to the CPU oracle as well (bit for bit).

Cases: the Cornell box at 64 x 64, 4 spp, max_depth 6; a 13 x 7 crop at 3 spp (273 paths: a partial last wave, a region whose
width is no multiple of 8, no keep words); a 15 x 11 region with a band, a partial last column and a row-major tail; max_depth 1 and 2; max_depth 8 (above MAX_CHAIN: two launches, k_path not selected);
ordered walk on and off, keep words on and off; a scene whose camera sees nothing (segments == 0); several passes with a non-zero
sample_offset; the second render of a scene, whose plan is learnt from the first."""
import numpy as np
import pytest

from conftest import oracle_render, scene_path

pytestmark = pytest.mark.gpu

PLAN_LEARNT, PLAN_PROBED = 1, 2


@pytest.fixture(scope="module")
def cbox(mi):
    return mi.load_file(scene_path("cbox.xml"), res=64, spp=4, max_depth=6)


@pytest.fixture(scope="module")
def cbox_ref(ob, cbox):
    """the oracle's film and statistics of the 64 x 64 x 4 render, seed 3: computed once"""
    img, st = oracle_render(ob, cbox, 3, 4)
    img.setflags(write=False)
    return img, st


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _counts(st):
    return st["segments"], st["shadow_rays"], list(st["live"])


def _both(mi, capi, sc, flags=0, **kw):
    """the render through k_path and the same render through k_bounce: film and statistics bit-equal -> (film, stats)"""
    integ, ctx = sc.integrator(), mi.default_context()
    img = integ.render(sc, flags=flags, **kw)
    st = ctx.stats()
    ref = integ.render(sc, flags=flags | capi.FILM_NO_PATH_KERNEL, **kw)
    st_ref = ctx.stats()
    print({k: st[k] for k in ("segments", "shadow_rays", "bounce_launches", "fuse_plan", "plan_source")}, list(st["live"])[:8])
    assert img.shape == ref.shape and np.array_equal(_bits(img), _bits(ref)), kw
    assert _counts(st) == _counts(st_ref), (kw, _counts(st), _counts(st_ref))
    assert st["bounce_launches"] == st_ref["bounce_launches"] and st["fuse_plan"] == st_ref["fuse_plan"]
    return img, st


def test_cbox_64_equals_k_bounce_and_the_oracle(mi, capi, cbox, cbox_ref):
    one = capi.film_fuse_plan(0x1F)
    img, st = _both(mi, capi, cbox, flags=one, seed=3, spp=4)
    ref, ost = cbox_ref
    assert np.array_equal(_bits(img), _bits(ref)) and img.mean() > 0
    assert (st["segments"], st["shadow_rays"]) == (ost["segments"], ost["shadow_rays"])
    assert st["live"][0] == 64 * 64 * 4 and st["bounce_launches"] == 1
    assert all(st["live"][d] > 0 for d in range(6)) and st["live"][6] == 0


@pytest.mark.parametrize("ordered", [True, False], ids=["ordered", "table_walk"])
@pytest.mark.parametrize("keep", [True, False], ids=["keep_words", "no_keep_words"])
def test_ordered_walk_and_keep_words_on_and_off(mi, capi, cbox, cbox_ref, ordered, keep):
    flags = capi.film_fuse_plan(0x1F) | (0 if ordered else capi.FILM_NO_ORDERED_WALK) | (0 if keep else capi.FILM_NO_TILE_CULL)
    img, st = _both(mi, capi, cbox, flags=flags, seed=3, spp=4)
    assert mi.default_context().tile_keep()["used"] == keep
    assert np.array_equal(_bits(img), _bits(cbox_ref[0]))
    assert (st["segments"], st["shadow_rays"]) == (cbox_ref[1]["segments"], cbox_ref[1]["shadow_rays"])


def test_crop_13_by_7_has_a_partial_last_wave(mi, ob, capi):
    sc = mi.load_file(scene_path("cbox.xml"), res=64, spp=3, max_depth=6, rfilter="box")
    crop = (21, 30, 13, 7)
    img, st = _both(mi, capi, sc, flags=capi.film_fuse_plan(0x1F), seed=5, spp=3, crop=crop)
    assert st["live"][0] == 13 * 7 * 3 == 273 and st["bounce_launches"] == 1
    assert not mi.default_context().tile_keep()["used"]
    ref, ost = oracle_render(ob, sc, 5, 3, crop=crop)
    assert img.shape == (7, 13, 3) and np.array_equal(_bits(img), _bits(ref)) and img.mean() > 0
    assert (st["segments"], st["shadow_rays"]) == (ost["segments"], ost["shadow_rays"])


def test_crop_with_a_band_a_partial_last_column_and_a_row_major_tail(mi, ob, capi):
    """film 21 x 13, crop (3, 2, 13, 9), tent filter: the region is 15 x 11 at (2, 1) -- one 8-row band whose last column of tiles
    is 7 pixels wide, three rows in row-major order behind it, away from the film's origin (csrc/film_key.h region_pixel)"""
    sc = mi.load_file(scene_path("cbox.xml"), res=32, spp=2, max_depth=3, rfilter="tent")
    film = sc.sensors()[0].film()
    film.width, film.height, film.crop = 21, 13, (0, 0, 21, 13)
    crop = (3, 2, 13, 9)
    img, st = _both(mi, capi, sc, flags=capi.film_fuse_plan(0x1F), seed=7, spp=2, crop=crop)
    assert st["live"][0] == 15 * 11 * 2 and st["bounce_launches"] == 1
    ref, ost = oracle_render(ob, sc, 7, 2, crop=crop)
    assert img.shape == (9, 13, 3) and np.array_equal(_bits(img), _bits(ref)) and img.mean() > 0
    assert (st["segments"], st["shadow_rays"]) == (ost["segments"], ost["shadow_rays"])


@pytest.mark.parametrize("max_depth", [1, 2])
def test_short_paths(mi, ob, capi, max_depth):
    sc = mi.load_file(scene_path("cbox.xml"), res=64, spp=4, max_depth=max_depth)
    img, st = _both(mi, capi, sc, flags=capi.film_fuse_plan(0x1F), seed=2, spp=4)
    ref, ost = oracle_render(ob, sc, 2, 4)
    assert np.array_equal(_bits(img), _bits(ref))
    assert (st["segments"], st["shadow_rays"]) == (ost["segments"], ost["shadow_rays"])
    assert st["bounce_launches"] == 1 and st["live"][0] == 64 * 64 * 4 and st["live"][max_depth] == 0
    assert (st["live"][1] > 0) == (max_depth == 2)
    if max_depth == 1:  # only emitters seen directly: no next-event estimation
        assert st["shadow_rays"] == 0


def test_max_depth_above_the_chain_limit_keeps_k_bounce(mi, ob, capi):
    sc = mi.load_file(scene_path("cbox.xml"), res=64, spp=4, max_depth=8)
    img, st = _both(mi, capi, sc, flags=capi.film_fuse_plan(0xFF), seed=2, spp=4)
    assert st["bounce_launches"] == 2  # six bounces, then two: no launch walks every bounce of the pass
    ref, _ = oracle_render(ob, sc, 2, 4)
    assert np.array_equal(_bits(img), _bits(ref))


def test_a_camera_that_sees_nothing(mi, capi):
    T = mi.ScalarTransform4f
    sc = mi.load_dict({
        "type": "scene", "integrator": {"type": "path", "max_depth": 6},
        "sensor": {"type": "perspective", "fov": 50, "to_world": T().look_at([0, 0, 5.5], [0, 0, 11], [0, 1, 0]),
                   "film": {"type": "hdrfilm", "width": 24, "height": 16, "rfilter": {"type": "tent"}},
                   "sampler": {"type": "independent", "sample_count": 4}},
        "wall": {"type": "rectangle", "bsdf": {"type": "diffuse"}},
        "light": {"type": "rectangle", "to_world": T().translate([0, 2.6, 0]) @ T().rotate([1, 0, 0], 90),
                  "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [4, 4, 4]}}, "bsdf": {"type": "diffuse"}}})
    img, st = _both(mi, capi, sc, flags=capi.film_fuse_plan(0x1F), seed=1, spp=4)
    assert st["segments"] == 0 and st["shadow_rays"] == 0 and st["bounce_launches"] == 1
    assert st["live"][0] == 24 * 16 * 4 and not any(list(st["live"])[1:])
    assert not img.any()


def test_several_passes_and_a_sample_offset(mi, ob, capi, cbox):
    one = capi.film_fuse_plan(0x1F)
    img, st = _both(mi, capi, cbox, flags=one, seed=3, spp=6, sample_offset=5, pass_paths=64 * 64 * 2)
    assert st["bounce_launches"] == 3 and st["live"][0] == 64 * 64 * 6
    ref, ost = oracle_render(ob, cbox, 3, 6, sample_offset=5)
    assert np.array_equal(_bits(img), _bits(ref))
    assert (st["segments"], st["shadow_rays"]) == (ost["segments"], ost["shadow_rays"])
    # the passes of a render do not change it
    whole, st_whole = _both(mi, capi, cbox, flags=one, seed=3, spp=6, sample_offset=5)
    assert np.array_equal(_bits(img), _bits(whole)) and _counts(st) == _counts(st_whole) and st_whole["bounce_launches"] == 1


def test_second_render_runs_the_learnt_plan(mi, ob, capi):
    sc = mi.load_file(scene_path("cbox.xml"), res=64, spp=16, max_depth=6)  # a scene of its own: nothing learnt yet
    integ, ctx = sc.integrator(), mi.default_context()
    first = integ.render(sc, seed=7, spp=16)
    st1 = ctx.stats()
    assert st1["plan_source"] == PLAN_PROBED
    img, st = _both(mi, capi, sc, seed=7, spp=16)
    assert st["plan_source"] == PLAN_LEARNT and st["fuse_plan"] & 0x1F == 0x1F and st["bounce_launches"] == 1
    assert np.array_equal(_bits(img), _bits(first)) and _counts(st) == _counts(st1)
    ref, _ = oracle_render(ob, sc, 7, 16)
    assert np.array_equal(_bits(img), _bits(ref))
