"""Device check of the short correctly rounded forms of csrc/device_math.h (rcp_rn, sqrt_rn, div_rn).  The checker
(tests/native/fp_short_forms.hip) is compiled with the library's flags and includes device_math.h; it compares each form bit for
bit with '/' and sqrtf of the same translation unit (two NaNs count as equal):
  rcp_rn, sqrt_rn  every one of the 2^32 inputs, mismatches per (sign, exponent) bucket and inside the declared domain;
  div_rn           every divisor mantissa at 11 exponents x 2050 numerators (domain edges, hard mantissas), then 1.3e10
                   random pairs of the domain.
A form that leaves its domain is exactly what the call sites must not feed it, so those counts are asserted too: a change of the
hardware or the compiler that widened or narrowed a form's exact range shows up here."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "physics-based-ray-tracing_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "fp_short_forms.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-Wall", "-Wno-unused-function"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    exe = str(tmp_path_factory.mktemp("fpchk") / "fp_short_forms")
    subprocess.run(["hipcc", *FLAGS, "-I", CSRC, "-o", exe, SRC], check=True, capture_output=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout)


def buckets(form):
    """{(sign, biased exponent): mismatches}"""
    return {tuple(int(x) for x in k.split(",")): v[0] for k, v in form["buckets"].items()}


@pytest.mark.gpu
def test_rcp_rn_is_exact_for_every_normal_reciprocal(report):
    r = report["rcp_rn"]
    assert r["inputs"] == 2**32
    assert r["domain_mismatches"] == 0, r
    # outside: subnormal divisors and |b| > 2^126, whose reciprocal is subnormal or overflows (v_rcp_f32 flushes)
    assert set(e for _, e in buckets(r)) <= {0, 253, 254}, r["buckets"]


@pytest.mark.gpu
def test_sqrt_rn_is_exact_from_two_to_the_minus_104(report):
    r = report["sqrt_rn"]
    assert r["inputs"] == 2**32
    assert r["domain_mismatches"] == 0, r
    assert all(e < 127 - 104 for _, e in buckets(r)), r["buckets"]
    print(f"sqrt_rn: {r['mismatches']} mismatching inputs, all with 0 < |x| < 2^-104")


@pytest.mark.gpu
def test_div_rn_is_exact_in_its_domain(report):
    g, r = report["div_rn_grid"], report["div_rn_random"]
    assert g["mismatches"] == 0 and r["mismatches"] == 0, (g, r)
    assert g["in_domain"] >= 10**11, g
    assert r["in_domain"] >= 10**10, r
