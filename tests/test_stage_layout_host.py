"""Host-side check of the staging layout (csrc/stage_layout.h): a call that stages host arrays names each array once, and where the
arrays lie in the workspace buffer and how much the buffer holds follow from that list -- no caller writes a byte count.  No GPU:
tests/native/stage_layout_check.cpp draws lists of 1 to 12 arrays (element sizes 1, 4, 8; lengths 0 to 2^20 + 1; null inputs) and
checks that offsets are multiples of 16, that slots neither overlap nor leave the total, that the total is the sum of the rounded
sizes and that the layout depends on the list alone, then holds the lists of the nine leaf operators and of the beamformers' host
form to the byte counts the driver used to write by hand.  The program is built with the address and undefined-behaviour sanitizers
and run on its own."""
import json
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "stage_layout_check.cpp")
CSRC = os.path.join(ROOT, "physics-based-ray-tracing_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stage_layout") / "stage_layout_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-o", exe, SRC])
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_the_layout_keeps_its_properties(report):
    assert report.returncode == 0, report.stderr
    assert "ERROR: AddressSanitizer" not in report.stderr and "runtime error" not in report.stderr, report.stderr
    rep = json.loads(report.stdout.strip().splitlines()[-1])
    assert rep["failures"] == 0 and rep["checks"] >= 20000


def test_the_header_includes_nothing_of_hip():
    text = open(os.path.join(CSRC, "stage_layout.h")).read()
    assert [line.split()[1] for line in text.splitlines() if line.startswith("#include")] == ["<array>", "<cstddef>"]


def test_no_staged_call_of_the_driver_writes_a_byte_count():
    """every request for the staging buffer is a layout's total, and every staged call goes through Stage::arrays"""
    text = open(os.path.join(CSRC, "pbrt_api.hip")).read()
    assert '#include "stage_layout.h"' in text
    assert re.findall(r'buf\("leaf_io", ([^)]*)\)', text) == ["io_at.total", "L.total"]
    assert text.count("S.arrays(stage_in(") == 17  # nine leaf operators, the beamformers' host form, seven image steps
    assert "bytes + 1024" not in text and "LEAF_LAUNCH" not in text
