"""The rule for non-finite and out-of-range geometry (include/pbrt_hip.h) on the CPU, before anything of it runs on a
device: (a) the integer model of a split sample position never indexes outside a trace and agrees with the float64 rule where both
parts lie inside +-2^31; (b) the stand-in problems of tests/geom_util.py are what a direct float64 statement of the rule makes of the
poisoned tables; (c) the variants are not vacuous on the walk cases that test_gpu_geometry_nonfinite.py runs."""
import itertools

import numpy as np
import pytest

import geom_util as gu
import nlbf_util as nu
from walk_cases import C0, T, geometry

ALL_NAMES = gu.NAMES + (gu.BIG,)


# ---- (a) the index model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tn", [2, 160])
def test_no_pair_of_parts_indexes_outside_the_trace(Tn):
    """Every index the model takes lies in [0, T - 1], for both interpolations and every pair of the set.  Where both parts are below
    2^31 in magnitude AND the receive part is not negative -- it is d fs, d a square root and fs > 0 (bf_request.h) -- the model is the
    float64 rule: the position it reads, i0 + w, is s_tx + s_rx to 2^-21 samples (the float64 sum of two parts below 2^31 is exact to
    2^-23, each float32 fraction to 2^-25, their float32 sum to 2^-24), and it takes a sample iff the rule does, except within 2^-20
    of the two ends 0 and T - 1 of the range, where that difference decides.  (Two NEGATIVE parts near -2^31 would wrap into the trace:
    -(2^31 - 1) twice is index 2.  No kernel forms such a pair; the header says so.)  The nearest arm IS the float64 sum."""
    vals = gu.part_values(Tn)
    taken = agreed = 0
    for s_tx, s_rx in itertools.product(vals, vals):
        idx, w = gu.linear_index(s_tx, s_rx, Tn)
        assert all(0 <= i <= Tn - 1 for i in idx), (s_tx, s_rx, idx)
        near = gu.nearest_index(s_tx, s_rx, Tn)
        assert all(0 <= i <= Tn - 1 for i in near), (s_tx, s_rx, near)
        taken += bool(idx)
        with np.errstate(invalid="ignore"):
            s = np.float64(s_tx) + np.float64(s_rx)
            r = np.rint(s)
        assert near == ((int(r),) if 0 <= r <= Tn - 1 else ()), (s_tx, s_rx)
        if not (abs(s_tx) < 2.0 ** 31 and 0.0 <= s_rx < 2.0 ** 31):
            continue
        want, s = gu.f64_linear(s_tx, s_rx, Tn)
        if min(abs(s), abs(s - (Tn - 1))) > 2.0 ** -20:
            assert bool(idx) == want, (s_tx, s_rx, idx, s)
        if idx:
            pos = idx[0] + float(w) if len(idx) == 2 else float(idx[0])
            assert abs(pos - s) <= 2.0 ** -21, (s_tx, s_rx, idx, w, s)
            agreed += 1
    assert taken >= 8 and agreed >= 8, (taken, agreed)          # (the set holds pairs that are taken)


def test_the_model_saturates_wraps_and_carries():
    assert gu.split(np.nan)[0] == 0 and np.isnan(gu.split(np.nan)[1])
    assert gu.split(np.inf)[0] == gu.I32_MAX and gu.split(-np.inf)[0] == gu.I32_MIN and gu.split(1e300) == (gu.I32_MAX, 0.0)
    assert gu.split(-(2.0 ** -25)) == (0, 0.0)                       # the fraction 1 - 2^-25 rounds to 1 in float32 and is carried
    assert gu.split(7.25) == (7, 0.25)
    # a first arrival of -inf and a receive part inside the trace: 0x80000000 + i, far beyond T - 1 as an unsigned number
    assert gu.linear_index(-np.inf, 17.5, 160)[0] == ()
    # two saturated parts wrap to -2: refused by the unsigned comparison, which a signed one would not do for the sum -2^31 - 2^31 = 0
    assert gu.linear_index(1e300, 1e300, 160)[0] == () and gu.linear_index(np.inf, 3.0, 160)[0] == ()
    # the one corner the header names: a transmit part saturated at -2^31, a receive part of 2^31 - 1 and a carry sum to 0 -- in the trace
    assert gu.linear_index(-(2.0 ** 40) + 0.5, 2.0 ** 31 - 0.5, 160)[0] == (0, 1)
    assert gu.linear_index(-(2.0 ** 40), 2.0 ** 31 - 0.5, 160)[0] == () and gu.linear_index(-np.inf, 2.0 ** 31 - 0.5, 160)[0] == ()
    # a NaN first arrival (a table entry) leaves the receive part alone to index the trace, with a NaN weight
    idx, w = gu.linear_index(np.nan, 17.5, 160)
    assert idx == (17, 18) and np.isnan(w)
    assert gu.nearest_index(np.nan, 17.5, 160) == () and gu.nearest_index(-np.inf, np.inf, 160) == ()


# ---- (b) the stand-ins are the rule ------------------------------------------------------------------------------------------------------
def _variants(name):
    return ("V1", "V2", "V4") + (("V4n",) if geometry(name)["elem"].ndim == 2 else ())


@pytest.mark.parametrize("name", ["a5_e64_lin_f1_sum", "a5_e16_convex_lin_f1_sum", "a6_e16_convex_small_near_f0_mean"])
def test_the_rule_on_poisoned_tables_is_the_restatement_on_the_stand_in(name):
    g = geometry(name)
    for family, f_d in (("das", None), ("iq", gu.F_D)):
        data = gu.case_data(name, family)
        clean, _ = gu.rule_image(data, g, f_d)
        ref_clean, B_clean = gu.restate(family, g, data)
        assert np.all(np.abs(clean - ref_clean) <= 1e-12 * B_clean)                 # (on clean tables it is the restatement itself)
        for variant in _variants(name):
            p, d2 = gu.stand_in(variant, g, data)
            ref, B = gu.restate(family, p, d2)
            for label, bad in gu.poisoned(variant, g).items():
                img, Br = gu.rule_image(data, bad, f_d)
                err = float(np.max(np.abs(img - ref) / np.maximum(B, 1e-300)))
                print(f"\n{name} {family} {variant} {label}: rule against the stand-in, largest |difference| / B = {err:.2e}")
                assert np.isfinite(img).all() and np.all(np.abs(img - ref) <= 1e-12 * B), (name, family, variant, label)
                assert np.all(np.abs(Br - B) <= 1e-12 * B)
                if variant != "V4n" or g["kw"]["f_number"] > 0:
                    assert np.any(img != clean), (name, family, variant)


def test_an_element_without_a_normal_still_bounds_the_first_arrival():
    """V4n on the f# > 0 convex case: the element keeps its place in the minimum.  Deleting it would be another problem wherever it is
    the first to arrive -- the stand-in turns its normal round instead."""
    g = geometry("a5_e16_convex_lin_f1_sum")
    p, _ = gu.stand_in("V4n", g, gu.case_data("a5_e16_convex_lin_f1_sum", "das"))
    assert np.all(p["n_a"] <= g["n_a"]) and p["n_a"].sum() < g["n_a"].sum()
    for (_, use, s_tx, _), (_, _, c_tx, _) in zip(nu._positions(p["tx"], p["elem"], p["x"], p["z"], p["fs"], C0, 0.0, 1.0),
                                                 nu._positions(g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, 0.0, 1.0)):
        assert not use[gu.absent(g)].any() and np.array_equal(s_tx, c_tx)
    d, _ = gu.stand_in("V4", g, gu.case_data("a5_e16_convex_lin_f1_sum", "das"))
    first = [np.array_equal(a[2], b[2]) for a, b in zip(nu._positions(d["tx"], d["elem"], d["x"], d["z"], d["fs"], C0, 0.0, 1.0),
                                                        nu._positions(g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, 0.0, 1.0))]
    print(f"\nfirst arrivals with element {gu.absent(g)} deleted equal the clean ones, per transmission: {first}")
    assert not any(first)


# ---- (c) the variants are not vacuous ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_NAMES)
def test_the_stand_ins_leave_out_at_most_two_per_cent(name):
    g = geometry(name)
    data = gu.case_data(name, "das")
    assert g["left_out"].mean() <= 0.02
    for variant in _variants(name):
        p, _ = gu.stand_in(variant, g, data)
        share = p["left_out"].mean()
        print(f"\n{name} {variant}: {100 * share:.2f} % of the pixels left out, {int((p['n_a'].sum(axis=0) == 0).sum())} use no element")
        assert share <= 0.02, (name, variant, share)
        assert (~p["left_out"] & (p["n_a"].sum(axis=0) > 0)).sum() >= 0.5 * p["left_out"].size


@pytest.mark.parametrize("name", ALL_NAMES)
def test_late_delays_move_the_first_arrival(name):
    """V1: the first arrival of transmission 1 moves by more than one sample on at least 5 % of the pixels; V2: it takes no term"""
    g = geometry(name)
    data = gu.case_data(name, "das")
    fn = g["kw"]["f_number"]
    clean = list(nu._positions(g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, 0.0, fn))[gu.SITE_A][2]
    p1, _ = gu.stand_in("V1", g, data)
    moved = list(nu._positions(p1["tx"], p1["elem"], p1["x"], p1["z"], p1["fs"], C0, 0.0, fn))[gu.SITE_A][2]
    share = float((np.abs(moved - clean) > 1.0).mean())
    print(f"\n{name} V1: the first arrival of transmission {gu.SITE_A} moves by more than one sample on {100 * share:.1f} % of the pixels")
    assert share >= 0.05, (name, share)
    p2, _ = gu.stand_in("V2", g, data)
    assert p2["n_a"][gu.SITE_A].sum() == 0 and g["n_a"][gu.SITE_A].sum() > 0
    others = np.arange(g["A"]) != gu.SITE_A
    assert np.array_equal(p2["n_a"][others], g["n_a"][others])


@pytest.mark.parametrize("name", ALL_NAMES)
def test_the_absent_element_is_in_an_aperture(name):
    """V4: the absent element (3 on a line, 7 of an element table) is used by at least one kept pixel of the clean problem"""
    g = geometry(name)
    used = np.zeros(g["left_out"].shape, bool)
    for _, ok in nu.delayed(np.ones((g["A"], g["E"], T), np.float32), g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, **
                            {k: g["kw"][k] for k in ("f_number", "interpolation")}):
        used |= ok[gu.absent(g)]
    print(f"\n{name} V4: element {gu.absent(g)} is used by {int((used & ~g['left_out']).sum())} kept pixels")
    assert (used & ~g["left_out"]).any()


@pytest.mark.parametrize("name", ALL_NAMES)
def test_the_table_sites_and_the_walked_tiles(name):
    """V6: three sites in three tiles; V3: the clean aperture is not empty somewhere, and every pixel that uses an element lies in a
    tile that is walked (so the header's statement on I/Q covers it)"""
    g = geometry(name)
    sites = gu.table_sites(name)
    assert len(sites) == 3 and len({(ix // 8, iz // 8) for ix, iz in sites}) == 3, sites
    w = gu.walked(g)
    assert np.all(w[g["n_a"].sum(axis=0) > 0]) and np.all(gu.sees(g) <= w)
    for ix, iz in sites:
        assert w[ix, iz] and not g["left_out"][ix, iz]
    print(f"\n{name}: V6 sites {sites}; {int(w.sum())} of {w.size} pixels lie in walked tiles, {int((g['n_a'].sum(axis=0) > 0).sum())} use an element")
