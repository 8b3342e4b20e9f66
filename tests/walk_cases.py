"""The walk cases that test_gpu_nlbf.py, test_gpu_iq.py and test_gpu_imgform_nonfinite.py (and their CPU twins) share: the smallest
shapes at which the walk over tiles, elements and angles can still go wrong -- 1 / 5 / 6 / 11 transmissions (a second trip of five
angles with one angle in it, a third one), 3 / 64 / 65 / 130 elements (fewer than the four waves of a workgroup; a second block of 64
with one element in it, a third with two), scans of 9 x 13, 9 x 17 and 24 x 16 pixels (partial 8 x 8 tiles), traces of 160 samples."""
import functools

import numpy as np

import convex_util as cu
import nlbf_util as nu

C0, FS, T = 1540.0, 20.0e6, 160

#        A, E,  (nx, nz), interpolation, f#,  compound, probe,    x step (m)
CASES = {
    "a1_e3_small_lin_f0_sum": (1, 3, (9, 13), "linear", 0.0, "sum", "line", 0.27e-3),
    "a5_e64_lin_f1_sum": (5, 64, (24, 16), "linear", 1.0, "sum", "line", 0.27e-3),
    "a6_e65_near_f1_mean": (6, 65, (24, 16), "nearest", 1.0, "mean", "line", 0.27e-3),
    "a6_e3_wide_lin_f1_mean": (6, 3, (24, 16), "linear", 1.0, "mean", "line", 0.5e-3),     # x tiles 0 and 2 see no element
    "a5_e65_small_near_f0_sum": (5, 65, (9, 13), "nearest", 0.0, "sum", "line", 0.27e-3),
    "a1_e64_near_f0_mean": (1, 64, (24, 16), "nearest", 0.0, "mean", "line", 0.27e-3),
    "a5_e16_convex_lin_f1_sum": (5, 16, (24, 16), "linear", 1.0, "sum", "convex", 0.27e-3),
    "a6_e16_convex_small_near_f0_mean": (6, 16, (9, 13), "nearest", 0.0, "mean", "convex", 0.27e-3),
    # a third trip of angles and a third block of elements: the walk is delay-and-sum's, which test_gpu_das_shapes.py takes as far
    "a11_e130_small_lin_f1_mean": (11, 130, (9, 17), "linear", 1.0, "mean", "line", 0.27e-3),
    "a11_e130_small_near_f0_sum": (11, 130, (9, 17), "nearest", 0.0, "sum", "line", 0.27e-3),
}
R_CONVEX, OPEN_CONVEX = 0.04, 60.0


@functools.lru_cache(maxsize=None)
def geometry(name):
    """tables of a case (float32, as the library reads them), the pixels das_util leaves out and N_a [A, nx, nz]"""
    A, E, (nx, nz), interp, fn, compound, probe, xstep = CASES[name]
    ang = np.linspace(-9.0, 9.0, A) if A > 1 else np.zeros(1)
    x = ((np.arange(nx) - (nx - 1) / 2) * xstep + 0.013e-3).astype(np.float32)
    depth = 1.03e-3 + np.arange(nz) * 0.187e-3
    fs = FS
    if probe == "convex":
        # (the elements lie 2.8 mm apart: deeper pixels and a lower sampling rate, so that an f-number of 1 still sees several of them
        # within 160 samples)
        depth, fs = 5.03e-3 + np.arange(nz) * 0.331e-3, FS / 2
        elem = cu.element_table(E, R_CONVEX, OPEN_CONVEX).astype(np.float32)
        tx = cu.tx_delays(elem.astype(np.float64), R_CONVEX, ang, C0).astype(np.float32)
        z = (R_CONVEX + depth).astype(np.float32)
    else:
        elem = ((np.arange(E) - (E - 1) / 2) * 1.0e-4).astype(np.float32)
        tx = cu.linear_delays(elem, ang, C0).astype(np.float32)
        z = depth.astype(np.float32)
    left_out, n_a = nu.margins(tx, elem, x, z, T, fs, C0, f_number=fn, interpolation=interp)
    return dict(A=A, E=E, fs=fs, tx=tx, elem=elem, x=x, z=z, kw=dict(f_number=fn, interpolation=interp, compound=compound), left_out=left_out,
                n_a=n_a)
