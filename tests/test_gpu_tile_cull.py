"""The first bounce of a brute-force scene leaves out the primitives the keep word of its camera tile rules out (csrc/tile_cull.h,
kernels_radiance.h k_tile_keep, device_scene.h brute_intersect): a cleared bit is a proof that the float test rejects, so the film
is the oracle's bit for bit, and the film, the segments, the shadow rays and the per-depth path counts are those of the same
render with the walk of every primitive (PBRT_FILM_NO_TILE_CULL).  Regions of whole blocks (64 x 64, crops 24 x 16 and 12 x 16 --
the second with blocks across the 8-row bands), a region without a table (13 x 7), a sample offset, three passes, one launch per
bounce and six bounces per launch, a camera in and next to a primitive's plane, 32 primitives, 33 (the _BIG kernel: no table) and
random scenes."""
import numpy as np
import pytest

from conftest import oracle_render, scene_path

pytestmark = pytest.mark.gpu


def _both(mi, ob, capi, sc, seed, spp, crop=None, sample_offset=0, pass_paths=0, flags=0):
    """the film with and without the keep words, both held to each other and to the oracle; -> (film, statistics)"""
    integ, ctx = sc.integrator(), mi.default_context()
    img = integ.render(sc, seed=seed, spp=spp, crop=crop, sample_offset=sample_offset, pass_paths=pass_paths, flags=flags)
    st = ctx.stats()
    full = integ.render(sc, seed=seed, spp=spp, crop=crop, sample_offset=sample_offset, pass_paths=pass_paths,
                        flags=flags | capi.FILM_NO_TILE_CULL)
    st_full = ctx.stats()
    ref, ost = oracle_render(ob, sc, seed, spp, crop=crop, sample_offset=sample_offset)
    assert img.shape == ref.shape and np.array_equal(img, full) and np.array_equal(img, ref) and img.mean() > 0
    assert st["segments"] == st_full["segments"] and st["shadow_rays"] == st_full["shadow_rays"] and list(st["live"]) == list(st_full["live"])
    if crop is None:  # (the oracle counts the paths of the crop, the library those of the region its filter reads)
        assert st["segments"] == ost["segments"] and st["shadow_rays"] == ost["shadow_rays"]
    return img, st


@pytest.mark.parametrize("rfilter", ["tent", "box"])
@pytest.mark.parametrize("seed", [0, 1])
def test_cornell_box(mi, ob, capi, rfilter, seed):
    sc = mi.load_file(scene_path("cbox.xml"), res=64, spp=4, rfilter=rfilter)
    _, st = _both(mi, ob, capi, sc, seed, 4)
    assert st["live"][0] == 64 * 64 * 4


@pytest.mark.parametrize("crop", [(16, 24, 24, 16), (40, 8, 12, 16), (21, 30, 13, 7)], ids=["24x16", "12x16", "13x7_no_table"])
def test_box_filter_crops(mi, ob, capi, crop):
    sc = mi.load_file(scene_path("cbox.xml"), res=64, spp=4, rfilter="box")
    img, _ = _both(mi, ob, capi, sc, 2, 4, crop=crop)
    assert img.shape == (crop[3], crop[2], 3)


def test_sample_offset(mi, ob, capi):
    sc = mi.load_file(scene_path("cbox.xml"), res=64, spp=4)
    _both(mi, ob, capi, sc, 3, 4, sample_offset=3)


def test_three_passes(mi, ob, capi):
    sc = mi.load_file(scene_path("cbox.xml"), res=64, spp=6)
    _, st = _both(mi, ob, capi, sc, 4, 6, pass_paths=64 * 64 * 2)
    assert st["passes"] == 3


@pytest.mark.parametrize("plan", [0, 0x3F])
def test_fuse_plans(mi, ob, capi, plan):
    sc = mi.load_file(scene_path("cbox.xml"), res=64, spp=4)
    _, st = _both(mi, ob, capi, sc, 5, 4, flags=capi.film_fuse_plan(plan))
    assert st["fuse_plan"] == plan


@pytest.mark.parametrize("name,origin,target", [("in_plane", [0, -1, 3], [0, 0, 0]), ("near_plane", [0.999, 0.1, 0.5], [-1, -0.3, -0.4])])
def test_camera_in_and_next_to_a_primitives_plane(mi, ob, capi, name, origin, target):
    """the cameras of tests/native/tile_cull_check.cpp: in the floor's plane y = -1, and 1e-3 from the wall x = 1"""
    sc = mi.load_file(scene_path("cbox.xml"), res=32, spp=4)
    sc.sensors()[0].transform = mi.ScalarTransform4f().look_at(origin, target, [0, 1, 0])
    _both(mi, ob, capi, sc, 6, 4)


def test_keep_words_are_reused_for_the_same_view_and_rebuilt_for_another(mi, ob, capi):
    """a context keeps the words of its last render: the same scene, camera and region again (another sample offset), then another
    crop, another camera, and a second scene in between"""
    sc = mi.load_file(scene_path("cbox.xml"), res=32, spp=2, rfilter="box")
    other = mi.load_file(scene_path("cbox.xml"), res=32, spp=2, rfilter="box")
    other.sensors()[0].transform = mi.ScalarTransform4f().look_at([1.5, 0.5, 3.5], [0, 0, 0], [0, 1, 0])
    integ = sc.integrator()
    for k, (scene, crop) in enumerate([(sc, None), (sc, None), (sc, (8, 8, 16, 16)), (other, (8, 8, 16, 16)), (sc, (8, 8, 16, 16)), (sc, None)]):
        img = integ.render(scene, seed=8, spp=2, crop=crop, sample_offset=k)
        ref, _ = oracle_render(ob, scene, 8, 2, crop=crop, sample_offset=k)
        assert np.array_equal(img, ref) and img.mean() > 0, k
    sc.sensors()[0].transform = mi.ScalarTransform4f().look_at([-1.0, 0.3, 3.8], [0, 0, 0], [0, 1, 0])
    img = integ.render(sc, seed=8, spp=2)
    ref, _ = oracle_render(ob, sc, 8, 2)
    assert np.array_equal(img, ref)


@pytest.mark.parametrize("n", [32, 33])
def test_32_and_33_primitives(mi, ob, capi, tmp_path, n):
    from test_gpu_typed_runs import _film_parts, _mixed, _shapes
    d = _film_parts(mi)  # a 16 x 16 film and the light: one primitive
    d.update(_shapes(mi, tmp_path, _mixed(n - 1, n), n))
    sc = mi.load_dict(d)
    assert len(sc.flatten()["prims"]) == n
    if n > 32:
        sc.accel = capi.ACCEL_BRUTE  # the _BIG kernel variant: no table
    _both(mi, ob, capi, sc, 7, 4)


@pytest.mark.parametrize("seed,ns,nr,nt", [(1, 3, 4, 0), (2, 5, 10, 12), (7, 2, 6, 5), (8, 6, 3, 9), (9, 0, 8, 14)])
def test_random_scenes(mi, ob, capi, tmp_path, seed, ns, nr, nt):
    from test_gpu_random_scenes import _random_scene
    sc = _random_scene(mi, tmp_path, seed, ns, nr, nt)
    assert len(sc.flatten()["prims"]) <= 32
    _both(mi, ob, capi, sc, seed, 3, crop=(1, 1, 22, 14))  # tent filter: a region of 24 x 16 pixels, six whole blocks
