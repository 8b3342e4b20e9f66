"""Host-side check of the Doppler requests (csrc/doppler_request.h): the makers that turn a pbrt_doppler_params and the
pointers of pbrt_doppler_autocorr / pbrt_doppler_maps into what their launches read -- every rule written once, `empty`, the launch
shape next to the limit that guards it, and the smoothing weights.  No GPU: the header is plain C++, and
tests/native/doppler_request_check.cpp holds the table -- every rule refuses its case and accepts the neighbouring boundary, the launch
shapes equal literals worked out by hand, and a sweep over the admitted ranges keeps grid, block and LDS within what a launch may ask
for.  The program is built with the address and undefined-behaviour sanitizers and run on its own."""
import json
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "doppler_request_check.cpp")
CSRC = os.path.join(ROOT, "physics-based-ray-tracing_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("doppler_request") / "doppler_request_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-o", exe, SRC])
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_the_makers_keep_the_rule_table_and_the_launch_shapes(report):
    assert report.returncode == 0, report.stderr
    assert "ERROR: AddressSanitizer" not in report.stderr and "runtime error" not in report.stderr, report.stderr
    rep = json.loads(report.stdout.strip().splitlines()[-1])
    assert rep["failures"] == 0 and rep["checks"] >= 10000


def test_the_header_includes_nothing_of_hip():
    text = open(os.path.join(CSRC, "doppler_request.h")).read()
    assert "#include <hip" not in text and "hip_runtime" not in text and "__global__" not in text
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ['"img_request.h"']


def test_the_driver_the_kernels_and_python_share_the_limits_and_the_rules(capi):
    """one definition of every limit, no rule in the entry points, every launch of a step reads its request, and the Doppler steps
    have lines of their own: the two macros of the seven image steps are not theirs"""
    kernels = open(os.path.join(CSRC, "kernels_beamform.h")).read()
    api = open(os.path.join(CSRC, "pbrt_api.hip")).read()
    driver = open(os.path.join(CSRC, "doppler_driver.h")).read()
    assert '#include "doppler_request.h"' in kernels
    for name in ("DOPPLER_MAX_FRAMES", "DOPPLER_MAX_DEGREE", "DOPPLER_MAX_K", "DOPPLER_TILE_X", "DOPPLER_TILE_Z"):
        assert f"#define {name}" not in kernels and f"#define {name}" not in api
    # the Doppler driver is a header of its own, included once by the driver, which holds nothing else of Doppler
    assert api.count('#include "doppler_driver.h"') == 1 and "doppler_acf" not in api and "DopplerMapsRequest" not in api
    assert f"#define DOPPLER" not in driver and "#include" not in driver
    assert driver.count("MAKE_REQUEST(ctx, DopplerAcfRequest, doppler_acf_request, p, ") == 2
    assert driver.count("MAKE_REQUEST(ctx, DopplerMapsRequest, doppler_maps_request, p, ") == 2
    assert "IMG_QUEUED(" not in driver and "IMG_STAGED(" not in driver and "NEED(" not in driver
    assert len(re.findall(r"IMG_LAUNCH\(c, rq\.launch, k_doppler_autocorr<\d>,", driver)) == 5
    assert len(re.findall(r"IMG_LAUNCH\(c, rq\.launch, k_doppler_maps,", driver)) == 1
    assert (capi.DOPPLER_MAX_FRAMES, capi.DOPPLER_MAX_DEGREE, capi.DOPPLER_MAX_K) == (64, 3, 15)
