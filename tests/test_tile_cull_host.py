"""Host-side check of csrc/tile_cull.h: which primitives the camera rays of a block of 64 region indices can meet (the keep words
of the first brute-force bounce).  No GPU: the header is plain C++; tests/native/tile_cull_check.cpp, built with the address and
undefined-behaviour sanitizers and run on its own, prints the keep words of named cases -- the Cornell box at 64 x 64, 48 x 80 and
12 x 16 (blocks that straddle the 8-row bands), films with a row-major tail or without a band (TAIL_CASES), a rotated camera, a
camera 1e-3 from a wall's plane and one exactly in the floor's plane, far clips of 1e4 and 1e6, sliver triangles, spheres tangent
to the corner ray of a tile, spheres around the camera and primitives behind it.

The header may clear a bit only if the kernel's float test rejects every camera ray of the block's rectangle.  For every case and
primitive the oracle's camera (oracle.binding.sensor_sample_ray: the kernel's camera_ray bit for bit) casts rays at the corners, the
edge midpoints and the centre of every rectangle [x0, x1 + 1] x [y0, y1 + 1] and at random positions px + jitter, among them the
jitter that rounds to px + 1.0, and a one-primitive OracleScene.ray_intersect says whether the float test accepts: an accepted ray in
a block whose bit is clear is a failure.  So that keeping everything cannot pass, the Cornell box must clear what a quarter of the
film cannot see, with the film's orientation found by oracle rays.

The program cuts a film into blocks through the inverse of region_index, as path_key and k_tile_keep do; its rectangles must be
those of tile_cull_util.block_rects, which states the layout forward, as the film kernel reads it, and is itself checked here.  The
program's second mode (cases from a file: what tests/test_gpu_tile_keep_words.py compares the device's words with) must give the
words of the built-in cases."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import scene_path
from tile_cull_util import (CSRC, _accepted, _camera, _one_prim_scene, _prims, accepted_in_cleared_blocks, block_rects,
                            cornell_quarters_clear_what_they_cannot_see, region_indices, run_cases, tile_cull_check_exe, write_cases)

# regions with a row-major tail below the last full 8-row band (16 x 12: two 8 x 8 blocks and a 16 x 4 tail block; 32 x 10; 64 x 9: a
# tail of one row), without a band (48 x 4: the middle block spans two rows across the full width; 128 x 1), with a width that is
# no multiple of 8 (20 x 16) and of one block (4 x 16)
TAIL_CASES = ["cbox_16x12", "cbox_32x10", "cbox_64x9", "cbox_48x4", "cbox_128x1", "cbox_20x16", "cbox_4x16"]
CASES = ["cbox_64", "cbox_48x80", "cbox_12x16", "rotated", "near_plane", "in_plane", "far_1e4", "far_1e6", "sliver", "tangent_sphere",
         "sphere_around_camera", "behind_camera"] + TAIL_CASES


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    return subprocess.run([tile_cull_check_exe(tmp_path_factory)], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def report(run):
    assert run.returncode == 0, run.stderr
    return json.loads(run.stdout.strip().splitlines()[-1])


def test_the_program_runs_clean_under_the_sanitizers(run, report):
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert sorted(report["cases"]) == sorted(CASES)


def test_the_header_includes_nothing_of_hip():
    text = open(os.path.join(CSRC, "tile_cull.h")).read()
    assert "#include <hip" not in text and "hip_runtime" not in text


@pytest.mark.parametrize("name", CASES)
def test_no_accepted_ray_in_a_block_whose_bit_is_clear(ob, capi, report, name):
    case = report["cases"][name]
    rng = np.random.default_rng(CASES.index(name))
    bi, acc = _accepted(ob, capi, case, rng)
    seen, bad = accepted_in_cleared_blocks(case, bi, acc)
    print(f"{name}: {len(bi)} rays, {seen} accepted (ray, primitive) pairs, {len(bad)} of them in blocks with the bit clear")
    assert not bad, (name, bad[:5])
    if name not in ("behind_camera",):
        assert seen > 0, name  # the rays do meet the case's primitives


@pytest.mark.parametrize("shape", [(16, 12), (32, 10), (64, 9), (48, 4), (128, 1), (20, 16), (4, 16), (64, 64), (12, 16), (13, 7)],
                         ids=lambda s: "%dx%d" % s)
def test_block_rects_states_the_layout(shape):
    """tile_cull_util.block_rects on its own: the forward region indices are a permutation of [0, rw * rh), every pixel lies in the
    rectangle of its own block, and a block's rectangle holds at least its 64 pixels"""
    rw, rh = shape
    idx = region_indices(rw, rh)
    assert idx.shape == (rh, rw) and np.array_equal(np.sort(idx.ravel()), np.arange(rw * rh))
    rects = block_rects(rw, rh)
    assert len(rects) == -(-rw * rh // 64)
    for y in range(rh):
        for x in range(rw):
            x0, y0, x1, y1 = rects[idx[y, x] >> 6]
            assert x0 <= x <= x1 and y0 <= y <= y1, (x, y)
    for b, (x0, y0, x1, y1) in enumerate(rects):
        assert 0 <= x0 <= x1 < rw and 0 <= y0 <= y1 < rh
        assert (x1 - x0 + 1) * (y1 - y0 + 1) >= min(64, rw * rh - 64 * b)


def test_block_rects_of_shapes_drawn_by_hand():
    assert block_rects(16, 12) == [(0, 0, 7, 7), (8, 0, 15, 7), (0, 8, 15, 11)]
    assert block_rects(32, 10) == [(0, 0, 7, 7), (8, 0, 15, 7), (16, 0, 23, 7), (24, 0, 31, 7), (0, 8, 31, 9)]
    assert block_rects(48, 4) == [(0, 0, 47, 1), (0, 1, 47, 2), (0, 2, 47, 3)]
    assert block_rects(128, 1) == [(0, 0, 63, 0), (64, 0, 127, 0)]
    assert block_rects(4, 16) == [(0, 0, 3, 15)]
    assert block_rects(64, 9)[8] == (0, 8, 63, 8) and block_rects(64, 9)[7] == (56, 0, 63, 7)
    # 20 wide: 2.5 tiles per band, the third block holds the last half tile of the first band and the first half tile of the second
    assert block_rects(20, 16) == [(0, 0, 7, 7), (8, 0, 15, 7), (0, 0, 19, 15), (4, 8, 11, 15), (12, 8, 19, 15)]


@pytest.mark.parametrize("name", CASES)
def test_the_programs_rectangles_are_block_rects(report, name):
    """the rectangles the program derives through the INVERSE of region_index (its pixel_of, as path_key and k_tile_keep) are the
    blocks of the forward form the film kernel gathers by"""
    case = report["cases"][name]
    rw, rh = int(case["cam"][15]), int(case["cam"][16])
    assert [tuple(b[:4]) for b in case["blocks"]] == block_rects(rw, rh)


def test_a_case_file_gives_the_words_of_the_builtin_case(report, tmp_path_factory, tmp_path, capi):
    """the program's second mode: the Cornell box cases written to a file, with their own rectangles, print the same words"""
    names = ["cbox_64", "cbox_16x12", "near_plane", "sliver"]
    cases = [(n, _camera(capi, report["cases"][n]["cam"]), _prims(capi, report["cases"][n]["prims"]),
              [tuple(b[:4]) for b in report["cases"][n]["blocks"]]) for n in names]
    path = str(tmp_path / "cases.txt")
    write_cases(path, cases)
    got = run_cases(tile_cull_check_exe(tmp_path_factory), path)
    for n in names:
        assert got["cases"][n] == report["cases"][n], n
    bad = tmp_path / "bad.txt"
    bad.write_text("case x cam 1 2 3\n")
    assert subprocess.run([tile_cull_check_exe(tmp_path_factory), str(bad)], capture_output=True).returncode == 2


def test_a_miss_is_reported_as_no_primitive(ob, capi):
    """what _accepted relies on: the oracle marks a miss with prim 0xffffffff"""
    P = _prims(capi, [[1, 0, 0, 0, 1] + [0] * 8])
    _, prim, _, _ = _one_prim_scene(ob, capi, P[0]).ray_intersect(np.float32([[0, 0, 4], [0, 3, 4]]), np.float32([[0, 0, -1], [0, 0, -1]]),
                                                                 np.float32([100, 100]))
    assert prim[0] == 0 and prim[1] == 0xFFFFFFFF


def test_the_builtin_cornell_box_is_the_scene_file(mi, capi, report):
    sc = mi.load_file(scene_path("cbox.xml"), res=64, spp=1)
    flat = sc.flatten()["prims"]
    mine = _prims(capi, report["cases"]["cbox_64"]["prims"])
    assert np.array_equal(flat["type"], mine["type"])
    assert np.array_equal(flat["g"][:, :9].view(np.uint32), mine["g"][:, :9].view(np.uint32))  # what the tests read (spheres: 4)
    cam, got = sc.sensors()[0].camera(), report["cases"]["cbox_64"]["cam"]
    want = list(cam.to_world) + [cam.tan_half_fov_x, cam.near_clip, cam.far_clip, cam.film_w, cam.film_h]
    assert np.array_equal(np.float32(got), np.float32(want))


def test_quarters_of_the_cornell_box_clear_what_they_cannot_see(ob, capi, report):
    share = cornell_quarters_clear_what_they_cannot_see(ob, capi, report["cases"]["cbox_64"])
    print(f"Cornell box 64 x 64: {share:.3f} of the (block, primitive) bits are clear; all cases: {report['cleared_share']:.3f}")
    assert 0.0 < report["cleared_share"] < 1.0
