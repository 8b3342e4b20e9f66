"""The float64 restatement of Capon beamforming (tests/capon_util.py; DESIGN.md D23, include/pbrt_hip.h "Capon") held to what follows
from the definition, on the CPU: its Cholesky against np.linalg.solve, L = 1 against I/Q delay-and-sum, the constant-sample identity
y = N v, the table of L and M, and the point-scatterer inequality that is the reason for the method.  test_gpu_capon.py holds the device
to this restatement."""
import numpy as np
import pytest

import capon_util as cu
import iq_util as iu
from walk_cases import C0, T, geometry


def test_the_cholesky_solves_hermitian_positive_definite_systems():
    rng = np.random.default_rng(3)
    for L in (1, 2, 5, 32):
        X = rng.standard_normal((7, L, L + 3)) + 1j * rng.standard_normal((7, L, L + 3))
        R = X @ np.conj(np.swapaxes(X, 1, 2)) + 0.01 * np.eye(L)
        want = np.linalg.solve(R, np.ones((7, L, 1), complex))[..., 0]
        for order in (0, 1):
            got = cu.chol_ones(R, np.float64, order)
            assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (L, order)
        got32 = cu.chol_ones(R, np.float32, 0)
        assert got32.dtype == np.complex64 and np.abs(got32 - want).max() <= 1e-2 * np.abs(want).max(), L


def test_the_table_of_subarray_lengths():
    #         N: (L, M) at l_prop 0.5, 0.25, 0
    table = {0: ((1, 0), (1, 0), (1, 0)), 1: ((1, 1), (1, 1), (1, 1)), 2: ((1, 2), (1, 2), (1, 2)), 3: ((1, 3), (1, 3), (1, 3)),
             63: ((31, 33), (15, 49), (1, 63)), 64: ((32, 33), (16, 49), (1, 64)), 65: ((32, 34), (16, 50), (1, 65)),
             130: ((32, 99), (32, 99), (1, 130)), 256: ((32, 225), (32, 225), (1, 256))}
    for N, rows in table.items():
        for l_prop, want in zip((0.5, 0.25, 0.0), rows):
            assert cu.lm(N, l_prop) == want, (N, l_prop)
    assert cu.lm(4, 0.5) == (2, 3) and cu.lm(5, 0.5) == (2, 4) and cu.lm(39, 0.5) == (19, 21)


@pytest.mark.parametrize("name", ["a5_e64_lin_f1_sum", "a6_e65_near_f1_mean", "a5_e16_convex_lin_f1_sum"])
def test_one_element_subarrays_are_iq_delay_and_sum(name):
    g = geometry(name)
    data = cu.case_data(name, "noise")
    args = (data, g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, 3.0e6)
    das, B = iu.iq_beamform(*args, **g["kw"])
    for delta_l in (0.01, 10.0):
        one, B1 = cu.capon(*args, l_prop=0.0, delta_l=delta_l, **g["kw"])
        assert np.allclose(B1, B, rtol=1e-12, atol=0) and np.any(B > 0)
        assert np.abs(one - das).max() <= 1e-12 * B.max()
    f32, _ = cu.capon(*args, l_prop=0.0, dtype=np.float32, **g["kw"])
    assert np.abs(f32 - das).max() <= 1e-4 * B.max()


def test_equal_samples_give_n_times_the_sample():
    v = 0.75 + 0.3j
    for N in (1, 2, 3, 7, 39, 64, 65, 130, 256):
        for l_prop, delta_l in ((0.5, 0.01), (0.25, 0.1), (0.0, 0.01), (0.5, 1e3)):
            L, M = cu.lm(N, l_prop)
            V = np.zeros((2, N + cu.MAX_L), complex)
            V[:, :N] = v
            y = cu._group(V, np.array([N, N]), L, l_prop, delta_l, np.float64, 0)
            assert np.abs(y - N * v).max() <= 1e-9 * N * abs(v) * L / min(delta_l, 1.0), (N, l_prop, delta_l)
    # through the whole restatement: constant traces, demod_freq 0 -> v sum_a N_a
    name = "a5_e64_lin_f1_sum"
    g = geometry(name)
    data = np.full((g["A"], g["E"], T), v, np.complex64)
    img, B = cu.capon(data, g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, 0.0, **g["kw"])
    want = complex(np.complex64(v)) * g["n_a"].sum(axis=0)
    assert np.abs(img - want).max() <= 1e-9 * np.abs(want).max() and np.allclose(B, np.abs(want))
    assert np.all(img[g["n_a"].sum(axis=0) == 0] == 0)


def test_zero_samples_give_zero_and_the_orders_agree():
    name = "a5_e64_lin_f1_sum"
    g = geometry(name)
    zero, B = cu.capon(np.zeros((g["A"], g["E"], T), np.complex64), g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, 3.0e6, **g["kw"])
    assert np.all(zero == 0) and np.all(B == 0)
    ref, B = cu.restated(name, "noise", 3.0e6, 0.5, 0.01)
    other, _ = cu.capon(cu.case_data(name, "noise"), g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, 3.0e6, order=1, **g["kw"])
    used = B > 0
    assert (np.abs(other - ref)[used] / B[used]).max() <= 1e-10


def test_capon_narrows_the_point_scatterer():
    def das(s, fn):
        return iu.iq_beamform(s["iq"], s["tx"], s["ex"], s["x"], s["z"], s["fs"], s["c"], s["f0"], f_number=fn)[0]

    def capon(s, fn):
        return cu.capon(s["iq"], s["tx"], s["ex"], s["x"], s["z"], s["fs"], s["c"], s["f0"], l_prop=0.5, delta_l=0.01, f_number=fn)[0]

    cu.assert_capon_narrows_the_scatterer(das, capon)
