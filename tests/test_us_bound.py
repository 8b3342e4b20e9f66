"""The per-bin tolerance of the acquisition tests (tests/us_util.py) on the CPU: the oracle's bin bounds leave its channel buffer
bit for bit as it is and describe it (count, sum |pressure|), and the tolerance flags numpy mutants of the oracle's buffer that model
real kernel bugs at nearly every bin each one touches.  No GPU: the mutants are never built as kernels."""
import numpy as np
import pytest

import us_util as uu

FLAG_MIN = 0.97


@pytest.fixture(scope="module")
def acq(mi, ob, capi):
    """(ref, extra, tol, p) of a small acquisition with echoes over many bins, and of one with CLAMP_TIME whose echoes pile up in
    the last bin"""
    out = {}
    for name, T, q in (("plain", 4000, 0), ("clamp", 900, capi.USQ_CLAMP_TIME)):
        sc = uu.phantom(mi, "few", 24, [-10.0, 0.0, 10.0], T, 64, 5)
        ui = sc.integrator()
        p = ui.us_params(sc, ui.quirks | q)
        ref, _, extra = ob.OracleScene.from_scene(sc).us_acquire(p, 5, 64, bounds=True)
        out[name] = (ref, extra, uu.tolerance(ref, extra, p), p)
    return out


@pytest.mark.parametrize("kind,emitter,quirks", [("plate", False, 0), ("few", False, 0x40), ("few", True, 0), ("bvh", False, 0x100),
                                                ("cone", True, 0), ("bvh", True, 0)])
def test_bounds_leave_the_channel_buffer_bit_for_bit(mi, ob, kind, emitter, quirks):
    sc = uu.phantom(mi, kind, 20, [-8.0, 0.0, 8.0], 3000, 40, 2, emitter=emitter)
    ui = sc.integrator()
    p = ui.us_params(sc, ui.quirks | quirks)
    osc = ob.OracleScene.from_scene(sc)
    plain, tx = osc.us_acquire(p, 2, 40, path_offset=7, norm_paths=50)
    stats = dict(osc.last_stats)
    ref, tx2, extra = osc.us_acquire(p, 2, 40, path_offset=7, norm_paths=50, bounds=True)
    assert np.array_equal(plain.view(np.uint32), ref.view(np.uint32)) and np.array_equal(tx, tx2) and osc.last_stats == stats
    assert (ref != 0).sum() > 100
    cnt, a = extra["count"], extra["abs_sum"]
    assert extra["count"].dtype == np.uint32 and cnt.shape == a.shape == extra["ramp_sum"].shape == ref.shape
    assert 0 < cnt.sum() <= stats["shadow_rays"]                                  # at most one echo per occlusion ray
    assert np.all(np.abs(ref) <= a) and np.all(a >= 0) and np.all(extra["ramp_sum"] >= 0)
    assert np.all(ref[cnt == 0] == 0) and np.all(a[cnt == 0] == 0) and np.all(extra["ramp_sum"][cnt == 0] == 0)
    one = cnt == 1
    assert one.sum() > 50 and np.array_equal(np.abs(ref[one]), a[one])            # one echo: |sum| is its |pressure|, same rounding


def test_count_is_the_number_of_deposited_echoes(mi, ob):
    """max_depth 1 on a lone plate, every echo inside the trace and nothing in the way: every segment deposits exactly one echo"""
    sc = uu.phantom(mi, "plate", 16, [-5.0, 0.0, 5.0], 4000, 48, 1, max_depth=1)
    ui = sc.integrator()
    osc = ob.OracleScene.from_scene(sc)
    ref, _, extra = osc.us_acquire(ui.us_params(sc), 1, 48, bounds=True)
    assert osc.last_stats["segments"] == 3 * 16 * 48
    assert int(extra["count"].sum()) == osc.last_stats["segments"]
    assert extra["abs_sum"].sum(dtype=np.float64) >= np.abs(ref).sum(dtype=np.float64)


def test_the_oracle_is_within_its_own_tolerance(acq):
    for ref, _, tol, _ in acq.values():
        assert np.all(tol >= uu.U32 * np.abs(ref)) and uu.worst_ratio(ref, ref, tol) == 0.0
        assert uu.worst_ratio(ref * np.float32(1 + 2 ** -23), ref, tol) <= 1.0     # one ulp anywhere is inside it


def _mutants(ref, ppr, rng):
    A, E, T = ref.shape
    nz = np.argwhere(ref != 0)
    pick = tuple(nz[rng.choice(len(nz), size=max(1, len(nz) // 20), replace=False)].T)
    r = int(np.argmax((ref != 0).sum(axis=(0, 2))))         # the receiver with the most echoes
    m = {}
    x = ref.copy()
    x[:, r, 1:] = ref[:, r, :-1]
    x[:, r, 0] = 0
    m["shift_one_trace"] = x
    x = np.zeros_like(ref)
    x[:, 1:] = ref[:, :-1]
    m["receiver_plus_one"] = x
    x = ref.copy()
    x[[0, 2]] = ref[[2, 0]]
    m["swap_angles"] = x
    x = ref.copy()
    x[pick] = 0
    m["lost_flush"] = x
    x = ref.copy()
    x[pick] *= np.float32(2)
    m["double_flush"] = x
    m["norm_ppr_plus_one"] = (ref.astype(np.float64) * ppr / (ppr + 1)).astype(np.float32)
    return m


@pytest.mark.parametrize("name", ["shift_one_trace", "receiver_plus_one", "swap_angles", "lost_flush", "double_flush",
                                  "norm_ppr_plus_one", "last_bin_dropped"])
def test_the_tolerance_flags_kernel_bug_mutants(acq, name):
    """a mutant touches the bins where it differs from the oracle's buffer; the tolerance must flag nearly all of them"""
    if name == "last_bin_dropped":
        ref, _, tol, _ = acq["clamp"]
        mut = ref.copy()
        mut[..., -1] = 0
    else:
        ref, _, tol, _ = acq["plain"]
        mut = _mutants(ref, 64, np.random.default_rng(0))[name]
    touched = mut != ref
    assert touched.sum() >= 40
    flagged = (uu.excess(mut, ref, tol) > 1.0) & touched
    frac = flagged.sum() / touched.sum()
    print(f"{name}: {frac:.4f} of {int(touched.sum())} bins flagged")
    assert frac >= FLAG_MIN, f"{name}: only {frac:.4f} of the {int(touched.sum())} bins it touches are flagged"
