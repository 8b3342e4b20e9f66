"""Build-container check (no GPU) of the compiled resources of k_path<ACCEL_K_BRUTE_ORDERED, 512> (kernels_radiance.h): the launch
a class-ordered ACCEL_K_BRUTE scene such as the Cornell box runs when one launch walks every bounce of a pass.  It is held to the
budget of the kernel it stands in for, k_bounce<true, ACCEL_K_BRUTE_ORDERED, 2> (tests/test_ordered_walk_asm.py): at most 64 VGPRs,
one spilled VGPR, 8 bytes of scratch -- 8 waves per SIMD -- and the 16 IEEE divisions left on purpose (two v_div_scale_f32 each).
Without the survivor compaction and with an argument block of its own it spills 18 SGPRs where that kernel spills 28: the value
reached is pinned, and so is the one barrier (the end of the table staging).  Resources only."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_asm_address_spaces import FLAGS, kernels_of
from test_fp_short_forms_asm import metadata

CSRC = os.path.join(ROOT, "physics-based-ray-tracing_amd", "csrc")
PATH = "_Z6k_pathILi5ELi512EEv8PathArgs"  # k_path<ACCEL_K_BRUTE_ORDERED = 5, 512>
PATH_TABLES = "_Z6k_pathILi0ELi512EEv8PathArgs"  # k_path<ACCEL_K_BRUTE = 0, 512>: the table walk
BOUNCE = "_Z8k_bounceILb1ELi5ELi2EEv7RadArgs"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = str(tmp_path_factory.mktemp("asm") / "pbrt_product.s")
    subprocess.run(["hipcc", *FLAGS, "-o", out, "pbrt_api.hip"], cwd=CSRC, check=True, capture_output=True, timeout=600)
    text = open(out).read()
    return kernels_of(text), metadata(text)


def test_both_instances_exist(asm):
    kernels, md = asm
    assert all(k in kernels and k in md for k in (PATH, PATH_TABLES)), sorted(k for k in kernels if k.startswith("_Z6k_path"))


def test_register_budget(asm):
    _, md = asm
    k = md[PATH]
    print({f: k[f] for f in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "kernarg_segment_size")})
    assert k["vgpr_count"] <= 64 and k["vgpr_spill_count"] <= 1 and k["private_segment_fixed_size"] <= 8, k


def test_fewer_spilled_sgprs_and_a_smaller_argument_block_than_the_bounce_kernel(asm):
    _, md = asm
    k, b = md[PATH], md[BOUNCE]
    assert k["sgpr_spill_count"] <= 18 and k["sgpr_spill_count"] <= b["sgpr_spill_count"], (k["sgpr_spill_count"], b["sgpr_spill_count"])
    assert k["kernarg_segment_size"] < b["kernarg_segment_size"], (k["kernarg_segment_size"], b["kernarg_segment_size"])


def test_division_count_and_the_single_barrier(asm):
    kernels, _ = asm
    ops = [l.split()[0] for l in kernels[PATH]]
    assert ops.count("v_div_scale_f32") <= 32, ops.count("v_div_scale_f32")
    assert ops.count("s_barrier") == 1, ops.count("s_barrier")
