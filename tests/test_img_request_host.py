"""Host-side check of the image-step requests (csrc/img_request.h): the makers that turn the arguments of pulse, envelope, log
compression, axial FIR, rf2iq, I/Q envelope and scan conversion into what their launches read -- every rule written once, `empty`,
and the launch shape next to the limit that guards it.  No GPU: the header is plain C++, and tests/native/img_request_check.cpp
holds the table -- every rule refuses its case and accepts the neighbouring boundary, the envelope's overlap is refused for the _dev
form only, `empty` is "no output element", every accepted request of a sweep over the admitted ranges keeps grid, block and LDS
within what a launch may ask for, and the launch shapes equal literals worked out by hand from the expressions the driver carried.
The program is built with the address and undefined-behaviour sanitizers and run on its own."""
import json
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "img_request_check.cpp")
CSRC = os.path.join(ROOT, "physics-based-ray-tracing_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("img_request") / "img_request_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-o", exe, SRC])
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_the_makers_keep_the_rule_table_and_the_launch_shapes(report):
    assert report.returncode == 0, report.stderr
    assert "ERROR: AddressSanitizer" not in report.stderr and "runtime error" not in report.stderr, report.stderr
    rep = json.loads(report.stdout.strip().splitlines()[-1])
    assert rep["failures"] == 0 and rep["checks"] >= 100000


def test_the_header_includes_nothing_of_hip():
    text = open(os.path.join(CSRC, "img_request.h")).read()
    assert "#include <hip" not in text and "hip_runtime" not in text
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<algorithm>", "<cmath>", "<cstddef>", "<cstdint>", '"../../include/pbrt_hip.h"']


def test_the_driver_and_the_kernels_take_rules_and_limits_from_the_header():
    """the limits have one definition, the entry points no rule of their own, and every launch of a step reads its request"""
    api = open(os.path.join(CSRC, "pbrt_api.hip")).read()
    kernels = open(os.path.join(CSRC, "kernels_beamform.h")).read()
    assert '#include "img_request.h"' in kernels
    for name in ("FIR_MAX_K", "RF2IQ_MAX_D", "ENV_MAX_N", "ENV_MAX_BLOCKS", "PULSE_MAX_K"):
        assert f"#define {name}" not in kernels and f"#define {name}" not in api
    assert "ranges_overlap" not in api and not re.search(r"static int \w+_check\(pbrt_ctx", api)
    assert api.count("\n    IMG_QUEUED(ctx, ") == 7 and api.count("\n    IMG_STAGED(ctx, ") == 7
    for kernel in ("k_apply_pulse", "rq.even ? k_hilbert_env_even : k_hilbert_env", "k_hilbert_taps", "k_env_max", "k_log_compress",
                   "k_axial_fir", "k_rf2iq", "k_iq_modulus", "k_scan_convert"):
        assert len(re.findall(r"IMG_LAUNCH\(c, rq\.\w+, %s," % re.escape(kernel), api)) == 1, kernel
