"""GPU parity of the acquisition beyond the 5 x 64 probe: every case against the CPU oracle under the per-bin tolerance of
tests/us_util.py (derived from float32 rounding), and the set of non-zero bins must be the same.

What the shapes reach (csrc/device_math.h, csrc/kernels_us.h, csrc/pbrt_api.hip us_impl):
- n_elements 1, 2, 63, 65, 128, 192, 256: FastDiv's is_one, power-of-two and magic-number paths for ray -> (angle, element) and
  path -> ray;
- n_angles 1, 2, 9 and 64 (PBRT_US_MAX_ANGLES);
- paths per ray at E - 1, E, E + 1: the first-bounce tables switch on at ppr >= E; with them and with PBRT_USQ_NO_FIRST_TABLES;
- time_samples 1, 2, 17 with most echoes past the end (the tf < T drop) and the same with PBRT_USQ_CLAMP_TIME (every echo piles
  into the last bin: many echoes per channel word in the echo table); 2047, 2048, 2049 across the echoes; a 20 000-sample trace;
- emitter primary rays (EMIT instances) at E = 128, A = 1 and E = 33, A = 9, where the region permutation engages, and without it:
  on the spheres and plates (k_us_bounce<., ACCEL_K_BRUTE, true>), beside an analytic cone (<., ACCEL_K_BRUTE_BIG, true>) and on the
  BVH streams (k_us_init_wf writes the emitter's rays, then k_trace + k_us_shade);
- with emitter rays, on the cone and the BVH phantom: the rays through k_us_emit_init and the path state (PBRT_US_EMIT_FUSED=0, brute
  force only), one launch per bounce, the intent set (quirks = 0) and the Dr.Jit variant;
- the generic (run-time quirks) instance and one launch per bounce at a non-default shape;
- the BVH streams (k_trace + k_us_shade) at E = 1 and 128;
- a pass split with a short last pass (div_ppr remade per pass), forced by a failing large allocation."""
import numpy as np
import pytest

import us_util as uu

pytestmark = pytest.mark.gpu
WORST = []      # (case, largest |got - ref| / tol): printed at the end of the module (pytest -s)


def angles(n):
    return [0.0] if n == 1 else list(np.linspace(-20.0, 20.0, n))


def run(mi, ob, case, kind, E, A, T, ppr, seed, quirks=0, emitter=False, max_depth=4, nonzero=True, ui_quirks=None):
    """quirks: switches added to the integrator's set; ui_quirks: the integrator's set itself (None: PBRT_USQ_REFERENCE)"""
    sc = uu.phantom(mi, kind, E, angles(A), T, ppr, seed, max_depth=max_depth, emitter=emitter, quirks=ui_quirks)
    ui = sc.integrator()
    q = ui.quirks | quirks
    buf = ui._acquire(sc, q)
    st = mi.default_context().stats()
    ref, tx, tol = uu.acquire_ref(ob, sc, ui, seed, ppr, quirks=q)
    assert buf.shape == ref.shape == (A, E, T) and np.isfinite(buf).all()
    assert st["samples"] == A * E * ppr and np.array_equal(ui.transmission_delays_buf, tx)
    assert np.array_equal(buf != 0, ref != 0), f"{case}: {int(((buf != 0) != (ref != 0)).sum())} bins differ in being non-zero"
    ratio = uu.worst_ratio(buf, ref, tol)
    WORST.append((case, ratio))
    assert ratio <= 1.0, f"{case}: |got - ref| reaches {ratio:.3g} x the per-bin tolerance"
    if nonzero:
        assert (ref != 0).sum() >= min(50, A * E // 2 + 1), case
    return buf, ref, st


@pytest.mark.parametrize("E,ppr", [(1, 2000), (2, 1000), (63, 200), (65, 200), (128, 100), (192, 100), (256, 100)])
def test_elements(mi, ob, E, ppr):
    run(mi, ob, f"E={E}", "few", E, 3, 4000, ppr, 11)


@pytest.mark.parametrize("A", [1, 2, 9, 64])
def test_angles(mi, ob, A):
    run(mi, ob, f"A={A}", "few", 20, A, 4000, 64, 12)


@pytest.mark.parametrize("tables", [True, False])
@pytest.mark.parametrize("E,dp", [(63, -1), (63, 0), (63, 1), (128, -1), (128, 0), (128, 1)])
def test_first_bounce_table_threshold(mi, ob, capi, E, dp, tables):
    run(mi, ob, f"E={E} ppr=E{dp:+d} tables={tables}", "few", E, 3, 4000, E + dp, 13, quirks=0 if tables else capi.USQ_NO_FIRST_TABLES)


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("T,E,ppr", [(1, 32, 64), (2, 32, 64), (17, 32, 64), (1, 1, 4000)])
def test_short_traces(mi, ob, capi, T, E, ppr, clamp):
    """the phantom's echoes arrive from bin ~800 on: without the clamp they are all dropped (tf < T), with it every echo of an
    (angle, receiver) lands in bin T - 1 -- about a hundred echoes per channel word at E = 32, and with one element every echo of an
    angle (thousands) in one word, through the echo table and its flush"""
    buf, ref, _ = run(mi, ob, f"T={T} E={E} clamp={clamp}", "few", E, 3, T, ppr, 14, quirks=capi.USQ_CLAMP_TIME if clamp else 0,
                      nonzero=clamp)
    if clamp:
        assert np.count_nonzero(ref[..., -1]) >= 0.6 * 3 * E and not ref[..., :-1].any()     # (E = 1: the +20 degree ray misses)
    else:
        assert not buf.any()


@pytest.mark.parametrize("T", [2047, 2048, 2049, 20000])
def test_trace_lengths(mi, ob, T):
    buf, ref, _ = run(mi, ob, f"T={T}", "few", 48, 3, T, 64, 15)
    if T < 3000:
        assert ref[..., T - 50:].any() and (ref != 0).sum() > 500      # echoes up to the end of the trace: the cut runs through them


@pytest.mark.parametrize("permute", [True, False])
@pytest.mark.parametrize("E,A,ppr", [(128, 1, 400), (33, 9, 600)])
def test_emitter_primary_rays(mi, ob, monkeypatch, E, A, ppr, permute):
    """more than 2 n_angles regions of 8192 paths in the pass, so the region permutation engages unless PBRT_US_EMIT_PERMUTE=0"""
    assert -(-A * E * ppr // 8192) > 2 * A
    if not permute:
        monkeypatch.setenv("PBRT_US_EMIT_PERMUTE", "0")
    run(mi, ob, f"emit E={E} A={A} permute={permute}", "few", E, A, 4000, ppr, 16, emitter=True)


@pytest.mark.parametrize("permute", [True, False])
@pytest.mark.parametrize("E,A,ppr", [(128, 1, 400), (33, 9, 600)])
@pytest.mark.parametrize("kind", ["cone", "bvh"])
def test_emitter_primary_rays_on_cone_and_bvh_phantoms(mi, ob, monkeypatch, kind, E, A, ppr, permute):
    """the shapes of test_emitter_primary_rays beside an analytic cone (brute force, the _BIG instances of k_us_bounce draw the rays)
    and on 41 primitives (k_us_init_wf writes them into the path state of the streams)"""
    assert -(-A * E * ppr // 8192) > 2 * A
    if not permute:
        monkeypatch.setenv("PBRT_US_EMIT_PERMUTE", "0")
    _, _, st = run(mi, ob, f"emit {kind} E={E} A={A} permute={permute}", kind, E, A, 4000, ppr, 16, emitter=True)
    assert (st["bounce_launches"] > 1) == (kind == "bvh")


@pytest.mark.parametrize("kind,switch", [("cone", "unfused_rays"), ("cone", "per_bounce"), ("cone", "intent"), ("cone", "drjit"),
                                         ("bvh", "per_bounce"), ("bvh", "intent"), ("bvh", "drjit")])
def test_emitter_primary_rays_under_the_switches(mi, ob, capi, monkeypatch, kind, switch):
    """emitter rays at E = 33, A = 9 with the rays written into the path state first (k_us_emit_init, then k_us_bounce<false, ., true>
    from depth 0; PBRT_US_EMIT_FUSED is read for brute-force scenes only), one launch per bounce, the intent arithmetic and the
    Dr.Jit variant (both through the run-time quirks instance)"""
    if switch == "unfused_rays":
        monkeypatch.setenv("PBRT_US_EMIT_FUSED", "0")
    q = {"per_bounce": capi.USQ_NO_FUSED_BOUNCES, "drjit": capi.USQ_DRJIT_VARIANT}.get(switch, 0)
    _, _, st = run(mi, ob, f"emit {kind} {switch}", kind, 33, 9, 4000, 600, 16, quirks=q, emitter=True,
                   ui_quirks=0 if switch == "intent" else None)
    if kind == "bvh" or switch == "per_bounce":
        assert st["bounce_launches"] > 1


@pytest.mark.parametrize("variant", ["generic", "per_bounce"])
def test_kernel_instances(mi, ob, capi, monkeypatch, variant):
    if variant == "generic":
        monkeypatch.setenv("PBRT_US_GENERIC_KERNEL", "1")
    run(mi, ob, f"{variant} E=65 A=2", "few", 65, 2, 3001, 96, 17,
        quirks=capi.USQ_NO_FUSED_BOUNCES if variant == "per_bounce" else 0)


@pytest.mark.parametrize("E,ppr", [(1, 600), (128, 64), (128, 160)])
def test_streams(mi, ob, E, ppr):
    _, _, st = run(mi, ob, f"streams E={E} ppr={ppr}", "bvh", E, 3, 4000, ppr, 18)
    assert st["bounce_launches"] > 1


def test_passes_with_a_short_last_pass(mi, ob, monkeypatch):
    """65 x 45 000 paths with every request above 80 MB failing: 2.9 M paths (175 MB of state) do not fit, half of them
    (88 MB) neither, the smallest pass (1 Mi paths, 16 131 per ray, 63 MB) does: passes of 16 131, 16 131 and 12 738 paths per ray"""
    ctx = mi.default_context()
    ctx.set_workspace_limit(1)
    ctx.trim()
    ctx.set_workspace_limit(0)
    monkeypatch.setenv("PBRT_DEBUG_ALLOC_FAIL_BYTES", str(80 << 20))
    try:
        _, _, st = run(mi, ob, "passes E=65", "plate", 65, 1, 4000, 45000, 19)
    finally:
        monkeypatch.delenv("PBRT_DEBUG_ALLOC_FAIL_BYTES")
        ctx.set_workspace_limit(1)
        ctx.trim()
        ctx.set_workspace_limit(0)
    assert st["passes"] == 3


def test_zz_report_worst_ratio():
    """(runs last in the module) the largest error-to-tolerance ratio of the cases above"""
    case, r = max(WORST, key=lambda x: x[1], default=("none", 0.0))
    print(f"\nlargest |got - ref| / tol over {len(WORST)} cases: {r:.3g} ({case})")
    assert r <= 1.0
