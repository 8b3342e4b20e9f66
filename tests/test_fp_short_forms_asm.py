"""Build-container check (no GPU) of what the short correctly rounded forms (csrc/device_math.h rcp_rn / sqrt_rn / div_rn)
bought in the compiled radiance kernels: the flagship k_bounce<true,0,2> keeps only the IEEE divisions deliberately left
(operands that the code alone cannot bound: sphere roots, mis_weight, emitter pdfs, the dielectric Fresnel terms, Russian
roulette, the brute-force / planar 1/det, the camera's aspect ratio), and the register budget of the kernels the new forms
reach stays where it was."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_asm_address_spaces import FLAGS, kernels_of

CSRC = os.path.join(ROOT, "physics-based-ray-tracing_amd", "csrc")
BOUNCE = "_Z8k_bounceILb1ELi0ELi2EEv7RadArgs"  # k_bounce<true, 0, 2>
IEEE_DIVISIONS_LEFT = 16  # each IEEE division is two v_div_scale_f32
# sgpr / vgpr spill ceilings of the kernels the forms also reach
CEILINGS = {
    "_Z7k_traceILb1ELi2ELb0EEv6WfArgs": (51, 2),  # k_trace<true, 2, false>
    "_Z7k_traceILb0ELi2ELb0EEv6WfArgs": (4, 0),  # k_trace<false, 2, false>
    "_Z7k_shadeILb1ELb1ELb1ELb0EEv6WfArgs": (23, 0),  # k_shade<true, true, true, false>
    "_Z7k_shadeILb0ELb0ELb0ELb0EEv6WfArgs": (26, 0),  # k_shade<false, false, false, false>
    "_Z11k_us_bounceILb1ELi0ELb0ELj319ELi0ELb0EEv6UsArgs": (13, 0),  # k_us_bounce<true, 0, false, 319, 0, false>
    # the glossy and the convex instance: what they spilled while they were k_shade_glossy<true, true, true> (23 / 0) and
    # k_us_bounce_convex<true, 0, false> (50 / 3) -- the same code under the one kernel name, so no margin
    "_Z7k_shadeILb1ELb1ELb1ELb1EEv6WfArgs": (23, 0),  # k_shade<true, true, true, true>
    "_Z11k_us_bounceILb1ELi0ELb0ELj4294967295ELin1ELb1EEv6UsArgs": (50, 3),  # k_us_bounce<true, 0, false, 0xffffffff, -1, true>
    # the ordered chain instances: the first to move when the path-record load / store or the wave scan change form
    # (profiles/shared_path_start.md); what they spill today, no margin
    "_Z8k_bounceILb1ELi5ELi2EEv7RadArgs": (28, 1),  # k_bounce<true, ACCEL_K_BRUTE_ORDERED, 2>
    "_Z8k_bounceILb0ELi5ELi2EEv7RadArgs": (48, 1),  # k_bounce<false, ACCEL_K_BRUTE_ORDERED, 2>
}


def metadata(asm_text):
    """{kernel: {field: int}} from the .amdgpu_metadata block"""
    md = asm_text[asm_text.index(".amdgpu_metadata"):]
    out = {}
    for blk in re.split(r"\n\s+- \.", md):
        m = re.search(r"\.name:\s+(\S+)", blk)
        if not m:
            continue
        out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, flags=re.M)}
    return out


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = str(tmp_path_factory.mktemp("asm") / "pbrt_product.s")
    subprocess.run(["hipcc", *FLAGS, "-o", out, "pbrt_api.hip"], cwd=CSRC, check=True, capture_output=True, timeout=600)
    text = open(out).read()
    return kernels_of(text), metadata(text)


def test_bounce_keeps_only_the_divisions_left_on_purpose(asm):
    kernels, _ = asm
    scales = sum(1 for l in kernels[BOUNCE] if l.split()[0] == "v_div_scale_f32")
    assert scales <= 2 * IEEE_DIVISIONS_LEFT, scales


def test_bounce_register_budget(asm):
    _, md = asm
    k = md[BOUNCE]
    assert k["vgpr_count"] <= 64 and k["vgpr_spill_count"] <= 1 and k["private_segment_fixed_size"] <= 8, k


@pytest.mark.parametrize("name", sorted(CEILINGS))
def test_spills_of_the_other_kernels(asm, name):
    _, md = asm
    sgpr, vgpr = CEILINGS[name]
    k = md[name]
    assert k["sgpr_spill_count"] <= sgpr and k["vgpr_spill_count"] <= vgpr, (name, k)
