"""The keep words k_tile_keep leaves on the device, read back with Context.tile_keep() (pbrt_ctx_tile_keep) and held to
 (a) the words csrc/tile_cull.h gives on the host for the same camera, primitives and rectangles -- bit for bit: both sides evaluate
     the same IEEE double operations without contraction -- with the rectangles from tile_cull_util.block_rects, the forward
     statement of region_index the film kernel gathers by, shifted to the region the filter implies;
 (b) the ray census of tests/test_tile_cull_host.py: no ray the oracle's float test accepts lies in a block whose bit is clear;
 (c) the quarter-film assertions of the Cornell box, a cleared bit in every view, and no table where none may be;
 (d) the launch count of k_tile_keep: the same view again reuses the table, another crop, camera or scene and a freed workspace
     buffer rebuild it;
 (e) films against the oracle when passes end inside a sample's blocks.
Regions with a row-major tail (16 x 12, 32 x 10, 64 x 9), without an 8-row band (48 x 4, 128 x 1), 20 and 4 pixels wide, clipped
at the film's corners by a tent and a Gaussian halo, a film with tan_y != tan_x, cameras in and next to a primitive's plane,
32 primitives and random scenes."""
import contextlib

import numpy as np
import pytest

from conftest import oracle_render, scene_path
from tile_cull_util import (_accepted, accepted_in_cleared_blocks, block_rects, cornell_quarters_clear_what_they_cannot_see, run_cases,
                            tile_cull_check_exe, write_cases)

pytestmark = pytest.mark.gpu

# box-filter crops of the Cornell box, every one away from the film's origin: the region is the crop.  128 x 1 does not fit the
# 64 x 64 film of the others: its film is 160 x 8
BOX_CROPS = {"16x12": (40, 8, 16, 12), "32x10": (24, 50, 32, 10), "64x9": (0, 30, 64, 9), "48x4": (10, 33, 48, 4), "128x1": (20, 3, 128, 1),
             "20x16": (31, 40, 20, 16), "4x16": (57, 5, 4, 16), "12x16": (45, 21, 12, 16)}
RANDOM = {"random_2": (2, 5, 10, 12), "random_8": (8, 6, 3, 9)}
VIEWS = (["cbox_64_tent"] + ["cbox_box_" + k for k in BOX_CROPS] +
         ["cbox_tent_corner", "cbox_gaussian_corner", "cbox_96x64", "in_plane", "near_plane", "prims_32"] + list(RANDOM))
IN_PLANE = ("in_plane", "near_plane")


def _cbox(mi, res=64, rfilter="tent", size=None, look_at=None):
    sc = mi.load_file(scene_path("cbox.xml"), res=res, spp=1, rfilter=rfilter)
    if size:  # a film that is not square (the field of view stays the square film's: tan_y = tan_x * height / width)
        film = sc.sensors()[0].film()
        film.width, film.height = size
        film.crop = (0, 0) + tuple(size)
    if look_at:
        sc.sensors()[0].transform = mi.ScalarTransform4f().look_at(look_at[0], look_at[1], [0, 1, 0])
    return sc


def _make(mi, capi, tmp_path, name):
    """-> (scene, crop) of a view"""
    if name == "cbox_64_tent":
        return _cbox(mi), None
    if name.startswith("cbox_box_"):
        key = name[len("cbox_box_"):]
        return _cbox(mi, rfilter="box", size=(160, 8) if key == "128x1" else None), BOX_CROPS[key]
    if name == "cbox_tent_corner":  # region (0, 0, 24, 16): clipped at the top-left corner
        return _cbox(mi), (0, 0, 23, 15)
    if name == "cbox_gaussian_corner":  # region (48, 52, 16, 12), clipped at the bottom-right corner: 192 pixels, a tail of 4 rows
        return _cbox(mi, rfilter="gaussian"), (50, 54, 14, 10)
    if name == "cbox_96x64":
        return _cbox(mi, size=(96, 64)), None
    if name == "in_plane":  # the cameras of tests/native/tile_cull_check.cpp
        return _cbox(mi, res=32, look_at=([0, -1, 3], [0, 0, 0])), None
    if name == "near_plane":
        return _cbox(mi, res=32, look_at=([0.999, 0.1, 0.5], [-1, -0.3, -0.4])), None
    if name == "prims_32":
        return _prims_scene(mi, capi, tmp_path, 32), None
    from test_gpu_random_scenes import _random_scene
    seed, ns, nr, nt = RANDOM[name]
    return _random_scene(mi, tmp_path, seed, ns, nr, nt), (1, 1, 22, 14)  # tent: a region of 24 x 16


def _prims_scene(mi, capi, tmp_path, n):
    from test_gpu_typed_runs import _film_parts, _mixed, _shapes
    d = _film_parts(mi)  # a 16 x 16 film and the light: one primitive
    d.update(_shapes(mi, tmp_path, _mixed(n - 1, n), n))
    sc = mi.load_dict(d)
    assert len(sc.flatten()["prims"]) == n
    if n > 32:
        sc.accel = capi.ACCEL_BRUTE
    return sc


def _implied_region(capi, sc, crop):
    """the crop widened by the filter's reach (box 0, tent 1, Gaussian 2 pixels), clipped to the film"""
    film = sc.sensors()[0].film()
    W, H = film.size()
    cx, cy, cw, ch = crop if crop is not None else film.crop
    R = {capi.FILTER_BOX: 0, capi.FILTER_TENT: 1, capi.FILTER_GAUSSIAN: 2}[film.rfilter.kind]
    x0, y0, x1, y1 = max(cx - R, 0), max(cy - R, 0), min(cx + cw + R, W), min(cy + ch + R, H)
    return x0, y0, x1 - x0, y1 - y0


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return tile_cull_check_exe(tmp_path_factory)


@pytest.fixture(scope="module")
def view(mi, capi, exe, tmp_path_factory):
    """view(name) -> what one render of the view left, made once: info (Context.tile_keep()), region (what the filter implies),
    n_prims, host (the host program's report for the render's camera, primitives and block_rects: its words) and device (the same
    case with the words read back from the device)"""
    made = {}

    def get(name):
        if name not in made:
            tmp = tmp_path_factory.mktemp(name)
            sc, crop = _make(mi, capi, tmp, name)
            img = sc.integrator().render(sc, seed=1, spp=1, crop=crop)
            assert np.isfinite(img).all()
            info = mi.default_context().tile_keep()
            region = _implied_region(capi, sc, crop)
            prims = sc.flatten()["prims"]
            rects = [(region[0] + x0, region[1] + y0, region[0] + x1, region[1] + y1) for x0, y0, x1, y1 in block_rects(region[2], region[3])]
            path = str(tmp / "case.txt")
            write_cases(path, [(name, sc.sensors()[0].camera(), prims, rects)])
            host = run_cases(exe, path)["cases"][name]
            device = dict(host, blocks=[b[:4] + [int(w)] for b, w in zip(host["blocks"], info["words"])])
            made[name] = dict(info=info, region=region, n_prims=len(prims), host=host, device=device, cam=sc.sensors()[0].camera(), prims=prims)
        return made[name]

    return get


# ---- (a) the device's words are the host's

@pytest.mark.parametrize("name", VIEWS)
def test_device_words_equal_the_host_words(capi, view, name):
    v = view(name)
    info, region, n = v["info"], v["region"], v["n_prims"]
    assert region[2] * region[3] % 64 == 0 and n <= 32  # a view that has a table
    assert (info["rx0"], info["ry0"], info["rw"], info["rh"]) == region, (info, region)
    assert info["used"] and info["n_blocks"] == region[2] * region[3] // 64 == len(info["words"]) == len(v["host"]["blocks"])
    # the case file carried the render's camera and primitives exactly
    cam = v["cam"]
    assert np.array_equal(np.float32(v["host"]["cam"][:15]), np.float32(list(cam.to_world) + [cam.tan_half_fov_x, cam.near_clip, cam.far_clip]))
    assert v["host"]["cam"][15:] == [cam.film_w, cam.film_h]
    assert np.array_equal(np.float32([p[1:] for p in v["host"]["prims"]]), v["prims"]["g"])
    words = info["words"].astype(np.uint64)
    low = np.uint64((1 << n) - 1)
    host = np.asarray([b[4] for b in v["host"]["blocks"]], np.uint64)
    differ = np.nonzero((words & low) != host)[0]
    print(f"{name}: region {region}, {len(words)} words, {n} primitives, {len(differ)} words differ from the host's")
    assert not len(differ), [(int(b), v["host"]["blocks"][b][:4], hex(int(words[b] & low)), hex(int(host[b]))) for b in differ[:5]]
    assert np.all(words >> np.uint64(n) == np.uint64(0xFFFFFFFF >> n))  # bits without a primitive stay set
    if name == "prims_32":  # primitive 31 is kept in all four blocks: a device word without bit 31 differs from the host's
        assert low == np.uint64(0xFFFFFFFF) and np.all(host >> np.uint64(31) == 1)


# ---- (b) the device's words are sound

@pytest.mark.parametrize("name", ["cbox_64_tent", "cbox_box_16x12", "cbox_box_48x4", "near_plane"])
def test_no_accepted_ray_in_a_block_whose_device_bit_is_clear(ob, capi, view, name):
    case = view(name)["device"]
    bi, acc = _accepted(ob, capi, case, np.random.default_rng(VIEWS.index(name)))
    seen, bad = accepted_in_cleared_blocks(case, bi, acc)
    print(f"{name}: {len(bi)} rays, {seen} accepted (ray, primitive) pairs, {len(bad)} of them in blocks with the bit clear")
    assert not bad, (name, bad[:5])
    assert seen > 0, name


# ---- (c) the table culls

def test_quarters_of_the_cornell_box_clear_what_they_cannot_see_on_the_device(ob, capi, view):
    share = cornell_quarters_clear_what_they_cannot_see(ob, capi, view("cbox_64_tent")["device"])
    print(f"Cornell box 64 x 64, device words: {share:.3f} of the (block, primitive) bits are clear")
    assert 0.0 < share < 1.0


@pytest.mark.parametrize("name", [n for n in VIEWS if n not in IN_PLANE])
def test_a_bit_is_clear(view, name):
    v = view(name)
    assert np.any(v["info"]["words"] != 0xFFFFFFFF), name


@pytest.mark.parametrize("what", ["no_tile_cull", "13x7", "33_primitives"])
def test_no_table_is_reported_as_none(mi, capi, tmp_path, what):
    ctx = mi.default_context()
    sc = _cbox(mi, rfilter="box")
    sc.integrator().render(sc, seed=1, spp=1)
    before = ctx.tile_keep()
    assert before["used"] and before["n_blocks"] == 64  # there is a table to forget
    if what == "33_primitives":
        sc = _prims_scene(mi, capi, tmp_path, 33)
    crop = (21, 30, 13, 7) if what == "13x7" else None
    sc.integrator().render(sc, seed=1, spp=1, crop=crop, flags=capi.FILM_NO_TILE_CULL if what == "no_tile_cull" else 0)
    tk = ctx.tile_keep()
    assert not tk["used"] and tk["n_blocks"] == 0 and len(tk["words"]) == 0 and (tk["rx0"], tk["ry0"], tk["rw"], tk["rh"]) == (0, 0, 0, 0)
    assert tk["builds"] == before["builds"]


# ---- (d) reuse and rebuild

@contextlib.contextmanager
def _fresh_context(capi):
    """inside, the package renders on a context of its own (as _capi.use_library does for another library)"""
    saved = capi._default_ctx
    capi._default_ctx = {}
    try:
        yield
    finally:
        capi._default_ctx = saved


def test_the_table_is_reused_for_the_same_view_and_rebuilt_for_another(mi, capi):
    origin = ([0, 0, 4], [0, 0, 0])
    moved = ([1.5, 0.5, 3.5], [0, 0, 0])
    crop = (8, 8, 16, 12)

    def fresh(look_at, crop):
        with _fresh_context(capi):
            sc = _cbox(mi, res=32, rfilter="box", look_at=look_at)
            sc.integrator().render(sc, seed=8, spp=1, crop=crop)
            tk = mi.default_context().tile_keep()
            assert tk["builds"] == 1 and tk["used"]
            return tk["words"]

    want = {(k, c): fresh(la, c) for k, la in (("origin", origin), ("moved", moved)) for c in (None, crop)}
    assert not np.array_equal(want["origin", None], want["moved", None]) and not np.array_equal(want["origin", crop], want["moved", crop])

    ctx = mi.default_context()
    sc, twin = _cbox(mi, res=32, rfilter="box"), _cbox(mi, res=32, rfilter="box")
    integ = sc.integrator()
    step = [0]

    def go(scene, crop, flags=0):
        step[0] += 1
        integ.render(scene, seed=8, spp=1, crop=crop, sample_offset=step[0], flags=flags)
        return ctx.tile_keep()

    t = go(sc, None)
    b = t["builds"]
    assert np.array_equal(t["words"], want["origin", None])
    t = go(sc, None)  # the same view, another sample offset
    assert t["builds"] == b and np.array_equal(t["words"], want["origin", None])
    t = go(sc, crop)  # another crop
    assert t["builds"] == b + 1 and (t["rx0"], t["ry0"], t["rw"], t["rh"]) == crop and np.array_equal(t["words"], want["origin", crop])
    t = go(sc, crop)
    assert t["builds"] == b + 1
    sc.sensors()[0].transform = mi.ScalarTransform4f().look_at(moved[0], moved[1], [0, 1, 0])  # another camera
    t = go(sc, crop)
    assert t["builds"] == b + 2 and np.array_equal(t["words"], want["moved", crop])
    sc.sensors()[0].transform = mi.ScalarTransform4f().look_at(origin[0], origin[1], [0, 1, 0])
    t = go(sc, crop)
    assert t["builds"] == b + 3 and np.array_equal(t["words"], want["origin", crop])
    t = go(twin, crop)  # another scene with the same primitives, camera and region
    assert t["builds"] == b + 4 and np.array_equal(t["words"], want["origin", crop])
    t = go(sc, crop)
    assert t["builds"] == b + 5 and np.array_equal(t["words"], want["origin", crop])
    # a render without a table in between: the next one with a table reports its own, and has not lost it
    t = go(sc, crop, flags=capi.FILM_NO_TILE_CULL)
    assert not t["used"] and t["builds"] == b + 5
    t = go(sc, crop)
    assert t["used"] and t["builds"] == b + 5 and np.array_equal(t["words"], want["origin", crop])
    # the workspace buffer freed (the last call did not use it) and allocated again: a new generation
    go(sc, crop, flags=capi.FILM_NO_TILE_CULL)
    ctx.trim()
    t = go(sc, crop)
    assert t["builds"] == b + 6 and np.array_equal(t["words"], want["origin", crop])
    t = go(sc, None)
    assert t["builds"] == b + 7 and np.array_equal(t["words"], want["origin", None])


def test_the_read_back_is_refused_while_a_recording_is_open(mi, capi):
    ctx = mi.default_context()
    sc = _cbox(mi, res=32, rfilter="box")
    sc.integrator().render(sc, seed=1, spp=1)
    want = ctx.tile_keep()
    d_in, d_out = mi.DeviceBuffer.from_host(ctx, np.ones((2, 64), np.float32)), mi.DeviceBuffer(ctx, (2, 64))
    mi.log_compress(d_in, 50.0, out=d_out)  # warm: a recorded call may not allocate
    with ctx.record() as rec:
        mi.log_compress(d_in, 50.0, out=d_out)
        with pytest.raises(RuntimeError, match="recording is open"):
            ctx.tile_keep()  # it would wait for the stream
    rec.graph.close()  # the recording stayed good
    got = ctx.tile_keep()
    assert got["builds"] == want["builds"] and np.array_equal(got["words"], want["words"])


# ---- (e) pass boundaries

@pytest.mark.parametrize("crop,spp,pass_paths", [(None, 6, 64 * 64 * 2 + 100), ((40, 8, 16, 12), 3, 16 * 12 + 10)], ids=["64x64", "16x12"])
def test_passes_that_end_inside_a_sample(mi, ob, capi, crop, spp, pass_paths):
    """pass_paths neither a multiple of 64 nor of the region: three passes; on the 16 x 12 crop tail blocks start passes"""
    from test_gpu_tile_cull import _both
    sc = mi.load_file(scene_path("cbox.xml"), res=64, spp=spp, rfilter="box")
    sc.integrator().render(sc, seed=4, spp=spp, crop=crop, pass_paths=pass_paths)
    tk = mi.default_context().tile_keep()
    assert tk["used"] and tk["n_blocks"] == (64 if crop is None else 3) and np.any(tk["words"] != 0xFFFFFFFF)
    _, st = _both(mi, ob, capi, sc, 4, spp, crop=crop, pass_paths=pass_paths)
    assert st["passes"] == 3
