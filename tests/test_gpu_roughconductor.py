"""Rough and Fresnel conductors on the DEVICE, through the plugin API.  The CPU oracle does not know the two
material types; the yardstick is the float64 restatement of tests/roughconductor_util.py, closed forms through the renderer, and
agreement between the library's own launch structures."""
import math

import numpy as np
import pytest

import roughconductor_util as ru
from test_roughconductor_bsdf import METAL_ETA, METAL_K, prototype_dict

pytestmark = pytest.mark.gpu

ALPHAS = [0.02, 0.1, 0.5, 1.0]
N_REC = 4096


def _accel(capi, name):
    return {"brute": capi.ACCEL_BRUTE, "bvh": capi.ACCEL_BVH, "bvh_global": capi.ACCEL_BVH_GLOBAL}[name]


def _rough(mi, alpha, eta=0.0, k=1.0):
    return mi.RoughConductorBSDF(mi.Properties("roughconductor", dict(distribution="ggx", alpha=alpha, eta=eta, k=k)))


# ---- (a) leaf operators against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS)
def test_sample_eval_pdf_against_the_restatement(mi, alpha):
    """BSDF.sample / eval / pdf of a coloured metal at 4096 seeded (wi, u) records (cos(theta_i) in [0.3, 1]) against the float64
    restatement, on the records whose decision margins (wi.z, |wo.z|, |wi . m|) are at least 1e-2 -- at least 90 % of them
    (tests/test_roughconductor_bsdf.py checks that on the CPU); a record that is decided invalid must come back invalid.

    Tolerance: four times the float32 rounding floor, which is measured here on the same inputs as the error of the restatement
    evaluated in np.float32 against float64 (the device orders its operations differently from NumPy).  wo and weight: largest
    absolute error; pdf and eval: largest relative error.  Floors measured for this seed (alpha: wo, pdf, weight | eval, pdf at a
    given wo):
        0.02: 1.4e-4, 2.6e-4, 3.6e-6 | 9e-7, 7e-7      0.1: 8.3e-6, 1.4e-5, 5.6e-5 | 9e-7, 7e-7
        0.5:  7.1e-7, 7.6e-7, 2.2e-6 | 8e-7, 6e-7      1.0: 5.8e-7, 6.0e-7, 7.8e-7 | 8e-7, 6e-7
    (the sampler's floor grows as alpha falls: a normal drawn near the rim of the projected disk is ill-conditioned in the sample,
    and D varies over |h.xy| ~ alpha).  On the device weight * pdf equals eval within the eval bound, and the pdf a sample
    returns IS pdf(wo), bit for bit."""
    wi, u = ru.draw_inputs(5, N_REC)
    fl, r64, decided, v = ru.sample_floors(alpha, METAL_ETA, METAL_K, wi, u)
    assert decided.mean() >= 0.9
    b = _rough(mi, alpha, METAL_ETA, METAL_K)
    si = mi.SurfaceInteraction3f(wi)
    bs, weight = b.sample(mi.BSDFContext(), si, np.zeros(N_REC, np.float32), u)
    valid = bs.sampled_component != 0xFFFFFFFF
    assert np.array_equal(valid[decided], r64["valid"][decided])
    assert np.all(bs.sampled_type[valid] == mi.BSDFFlags.GlossyReflection)
    err = dict(wo=float(np.abs(bs.wo[v] - r64["wo"][v]).max()), pdf=ru.rel_err(bs.pdf[v], r64["pdf"][v]),
               weight=float(np.abs(weight[v] - r64["weight"][v]).max()))
    print(f"alpha {alpha}: sample floor {fl} device {err}")
    for key in err:
        assert err[key] <= 4 * fl[key], (key, err[key], fl[key])
    # eval / pdf at the device's own directions
    wo = bs.wo[v]
    efl, f64, p64 = ru.eval_floors(alpha, METAL_ETA, METAL_K, wi[v], wo)
    f, p = b.eval_pdf(mi.BSDFContext(), mi.SurfaceInteraction3f(wi[v]), wo)
    eerr = dict(eval=ru.rel_err(f, f64), pdf=ru.rel_err(p, p64))
    print(f"alpha {alpha}: eval floor {efl} device {eerr}")
    assert eerr["eval"] <= 4 * efl["eval"] and eerr["pdf"] <= 4 * efl["pdf"], (eerr, efl)
    assert np.array_equal(p, bs.pdf[v])                                               # sample's pdf == pdf(wo)
    assert ru.rel_err(weight[v] * bs.pdf[v][:, None], f.astype(np.float64)) <= 4 * efl["eval"]
    assert np.array_equal(b.eval(mi.BSDFContext(), mi.SurfaceInteraction3f(wi[v]), wo), f)
    # below the surface on either side: nothing
    f0, p0 = b.eval_pdf(mi.BSDFContext(), mi.SurfaceInteraction3f(wi[:8]), wi[:8] * np.array([1, 1, -1], np.float32))
    assert not f0.any() and not p0.any()
    bs0, w0 = b.sample(mi.BSDFContext(), mi.SurfaceInteraction3f(wi[:8] * np.array([1, 1, -1], np.float32)), np.zeros(8), u[:8])
    assert np.all(bs0.sampled_component == 0xFFFFFFFF) and not w0.any()


# ---- (b) the smooth conductor with eta / k ------------------------------------------------------------------------------------------
def test_fresnel_conductor_weight(mi):
    """type 6: a delta lobe into the mirror direction whose weight is F(wi.z) per channel, within four times the float32 floor of
    the restatement (measured: 6.6e-7 absolute, device 6.0e-7); material 'none' written out (eta = 0, k = 1) weighs exactly 1"""
    wi, u = ru.draw_inputs(9, N_REC)
    b = mi.ConductorBSDF(mi.Properties("conductor", dict(eta=METAL_ETA, k=METAL_K)))
    bs, w = b.sample(mi.BSDFContext(), mi.SurfaceInteraction3f(wi), np.zeros(N_REC, np.float32), u)
    assert np.array_equal(bs.wo, wi * np.array([-1, -1, 1], np.float32)) and np.all(bs.pdf == 1) and np.all(bs.sampled_component == 0)
    F64 = ru.fresnel_conductor(wi[:, 2:3].astype(np.float64), METAL_ETA, METAL_K)
    F32 = ru.fresnel_conductor(wi[:, 2:3], np.float32(METAL_ETA), np.float32(METAL_K), np.float32)
    floor, err = float(np.abs(F32 - F64).max()), float(np.abs(w - F64).max())
    print(f"fresnel floor {floor} device {err}")
    assert err <= 4 * floor
    b1 = mi.ConductorBSDF(mi.Properties("conductor", dict(eta=0.0, k=1.0)))
    assert b1.to_material()[0] == 6
    assert np.all(b1.sample(mi.BSDFContext(), mi.SurfaceInteraction3f(wi), np.zeros(N_REC, np.float32), u)[1] == 1)
    f, p = b.eval_pdf(mi.BSDFContext(), mi.SurfaceInteraction3f(wi), bs.wo)
    assert not f.any() and not p.any()                                                 # a delta lobe evaluates to nothing


def _box(mi, integrator, extra, res=32, spp=64, fov=40.0, D=0.95, Le=0.8, lit=True):
    """six black walls around the origin (emitting Le when lit), a camera at (0, 0, -D) looking along +z"""
    T = mi.ScalarTransform4f
    black = {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.0, 0.0, 0.0]}}
    walls = {
        "zp": T().translate([0, 0, 1]).rotate([0, 1, 0], 180), "zn": T().translate([0, 0, -1]),
        "xp": T().translate([1, 0, 0]).rotate([0, 1, 0], -90), "xn": T().translate([-1, 0, 0]).rotate([0, 1, 0], 90),
        "yp": T().translate([0, 1, 0]).rotate([1, 0, 0], 90), "yn": T().translate([0, -1, 0]).rotate([1, 0, 0], -90)}
    d = {"type": "scene", "integrator": integrator,
         "sensor": {"type": "perspective", "fov": fov, "near_clip": 1e-3, "far_clip": 100.0,
                    "to_world": T().look_at([0, 0, -D], [0, 0, 0], [0, 1, 0]),
                    "sampler": {"type": "independent", "sample_count": spp},
                    "film": {"type": "hdrfilm", "width": res, "height": res, "rfilter": {"type": "box"}}}}
    for k, t in walls.items():
        d[k] = {"type": "rectangle", "to_world": t, "bsdf": black}
        if lit:
            d[k]["emitter"] = {"type": "area", "radiance": {"type": "rgb", "value": [Le] * 3}}
    d.update(extra)
    return mi.load_dict(d)


def test_conductor_given_material_none_renders_the_mirror_film(mi, capi):
    """`conductor` with eta = 0, k = 1 written out (type 6, the instances with the new code) renders the film of the plain
    `conductor` (type 1, the instances every other scene runs), array_equal: F is exactly 1"""
    films = {}
    for name, bsdf in (("plain", {"type": "conductor"}), ("none", {"type": "conductor", "eta": 0.0, "k": 1.0})):
        extra = {"ball": {"type": "sphere", "radius": 0.3, "bsdf": bsdf},
                 "tube": {"type": "cylinder", "p0": [0.5, -0.5, 0.2], "p1": [0.5, 0.5, 0.2], "radius": 0.15,
                          "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.7, 0.5, 0.3]}}}}
        for accel in ("brute", "bvh"):
            sc = _box(mi, {"type": "path", "max_depth": 5}, extra)
            sc.accel = _accel(capi, accel)
            films[name, accel] = mi.render(sc, seed=3, spp=16)
    assert films["plain", "brute"].std() > 0
    for key in films:
        assert np.array_equal(films[key], films["plain", "brute"]), key


# ---- (c) closed form through the renderer ------------------------------------------------------------------------------------------
_E_CACHE = {}


def _plate_expectation(mi, sc, M, alpha, eta, k):
    """pixels whose four corners fall well inside the plate, and E(mu, alpha) at each one's centre ray.  E comes from quadrature
    of the restatement at seven Chebyshev nodes of the plate's mu range (two grid resolutions that agree to 1e-4) and the degree-6
    interpolant through them (held to 1e-5 against quadrature at three other mu)."""
    sens = sc.sensors()[0]
    W, H = sens.film().size()
    Mi = np.linalg.inv(M)
    n = M[:3, :3] @ np.array([0.0, 0.0, 1.0])
    n /= np.linalg.norm(n)
    eta, k = np.broadcast_to(np.asarray(eta, np.float64), 3), np.broadcast_to(np.asarray(k, np.float64), 3)

    def rays(off):
        px = np.arange(W * H)
        pos = np.stack([((px % W) + off[0]) / W, ((px // W) + off[1]) / H], axis=1).astype(np.float32)
        r, _ = sens.sample_ray(0.0, 0.0, pos, None)
        return np.asarray(r["o"], np.float64), np.asarray(r["d"], np.float64)

    inside = np.ones(W * H, bool)
    for off in ((0, 0), (1, 0), (0, 1), (1, 1)):
        o, d = rays(off)
        t = ((M[:3, 3] - o) @ n) / (d @ n)
        q = (np.c_[o + t[:, None] * d, np.ones(len(o))] @ Mi.T)[:, :2]
        inside &= (np.abs(q) <= 0.9).all(axis=1) & (t > 0)
    o, d = rays((0.5, 0.5))
    mu = -(d @ n)
    assert inside.sum() >= 40 and mu[inside].min() > 0.5
    lo, hi = mu[inside].min(), mu[inside].max()
    key = (alpha, tuple(eta), tuple(k), round(lo, 9), round(hi, 9))
    if key not in _E_CACHE:
        x = np.cos((2 * np.arange(7) + 1) * np.pi / 14)
        nodes = 0.5 * (lo + hi) + 0.5 * (hi - lo) * x
        e256 = np.array([ru.albedo(alpha, eta, k, m, 256) for m in nodes])
        e512 = np.array([ru.albedo(alpha, eta, k, m, 512) for m in nodes])
        assert np.abs(e512 - e256).max() < 1e-4
        co = [np.polyfit(x, e512[:, c], 6) for c in range(3)]
        for xt in (-0.77, 0.13, 0.61):
            want = ru.albedo(alpha, eta, k, 0.5 * (lo + hi) + 0.5 * (hi - lo) * xt, 512)
            assert np.abs(np.array([np.polyval(c, xt) for c in co]) - want).max() < 1e-5
        _E_CACHE[key] = co
    co = _E_CACHE[key]
    xs = (mu[inside] - 0.5 * (lo + hi)) / (0.5 * (hi - lo))
    return inside.reshape(H, W), np.stack([np.polyval(c, xs) for c in co], axis=1)


@pytest.mark.parametrize("metal", [False, True])
@pytest.mark.parametrize("alpha", [0.1, 0.5])
@pytest.mark.parametrize("accel", ["brute", "bvh", "bvh_global"])
@pytest.mark.parametrize("integrator", ["path", "direct"])
def test_emitting_box_around_a_rough_plate(mi, capi, integrator, accel, alpha, metal):
    """six black walls emitting Le around a tilted rough-conductor rectangle: a pixel fully on the plate sees Le from every
    direction of the plate's hemisphere, so with `path` at max_depth 2 and with `direct` its expectation is Le E(mu, alpha) per
    channel, E = integral over wo.z > 0 of f cos(theta_o) at the pixel's own mu (quadrature of the restatement).  32 x 32 pixels,
    1024 samples each, seed 2; the mean over the plate's pixels of (film - Le E) is held to five standard errors, estimated from
    the per-pixel spread of that render.  One number that checks eval, pdf, sample, the emitter-sampling branch with its MIS weight,
    the MIS weight at the emitter hit and the pending shadow contribution of the streams together.
    Mutations that must fail it: G1(wo) dropped from the sample weight (alpha 0.5: E rises by several per cent); the MIS weight of
    the emitter-sampling branch dropped (that strategy is then counted in full beside the BSDF strategy)."""
    T = mi.ScalarTransform4f
    Le, spp = 0.8, 1024
    eta, k = (METAL_ETA, METAL_K) if metal else (0.0, 1.0)
    tw = T().rotate([1, 0, 0], 25.0) @ T().rotate([0, 1, 0], 180.0) @ T().scale([0.3, 0.3, 1.0])
    plate = {"plate": {"type": "rectangle", "to_world": tw,
                       "bsdf": {"type": "roughconductor", "distribution": "ggx", "alpha": alpha, "eta": eta if not metal else
                                {"type": "rgb", "value": eta}, "k": k if not metal else {"type": "rgb", "value": k}}}}
    integ = {"type": "path", "max_depth": 2} if integrator == "path" else {"type": "direct"}
    sc = _box(mi, integ, plate, spp=spp, Le=Le)
    sc.accel = _accel(capi, accel)
    img = mi.render(sc, seed=2, spp=spp)
    assert np.isfinite(img).all()
    inside, E = _plate_expectation(mi, sc, np.asarray(tw.matrix, np.float64), alpha, eta, k)
    diff = img[inside].astype(np.float64) - Le * E
    mean, se = diff.mean(axis=0), diff.std(axis=0, ddof=1) / math.sqrt(len(diff))
    print(f"{integrator} {accel} alpha {alpha} metal {metal}: pixels {len(diff)} mean(film) {img[inside].mean(axis=0)} "
          f"mean(Le E) {(Le * E).mean(axis=0)} diff {mean} se {se}")
    assert np.all(se > 0) and np.all(np.abs(mean) <= 5 * se), (mean, se)
    assert np.all(img[~inside][:8] > 0)


# ---- (d) one area light over the plate, `direct` -----------------------------------------------------------------------------------
def _light_expectation(sens, M, Ml, alpha, eta, k, Le, n):
    """per pixel fully on the plate: the integral over the light of f cos(theta_o) Le cos(theta_l) / r^2 dA (nothing occludes), by
    the midpoint rule on n x n points of the light, averaged over 2 x 2 positions in the pixel.  float64, the restatement's f."""
    W, H = sens.film().size()
    Mi = np.linalg.inv(M)
    nrm = M[:3, :3] @ np.array([0.0, 0.0, 1.0])
    nrm /= np.linalg.norm(nrm)
    s = M[:3, 0] / np.linalg.norm(M[:3, 0])
    t = np.cross(nrm, s)
    nl = Ml[:3, :3] @ np.array([0.0, 0.0, 1.0])
    nl /= np.linalg.norm(nl)
    g = (np.arange(n) + 0.5) * (2.0 / n) - 1.0
    uv = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    xl = uv[:, :1] * Ml[:3, 0] + uv[:, 1:] * Ml[:3, 1] + Ml[:3, 3]
    dA = np.linalg.norm(np.cross(Ml[:3, 0], Ml[:3, 1])) * (2.0 / n) ** 2

    def rays(off):
        px = np.arange(W * H)
        pos = np.stack([((px % W) + off[0]) / W, ((px // W) + off[1]) / H], axis=1).astype(np.float32)
        r, _ = sens.sample_ray(0.0, 0.0, pos, None)
        return np.asarray(r["o"], np.float64), np.asarray(r["d"], np.float64)

    inside = np.ones(W * H, bool)
    for off in ((0, 0), (1, 0), (0, 1), (1, 1)):
        o, d = rays(off)
        tt = ((M[:3, 3] - o) @ nrm) / (d @ nrm)
        q = (np.c_[o + tt[:, None] * d, np.ones(len(o))] @ Mi.T)[:, :2]
        inside &= (np.abs(q) <= 0.9).all(axis=1) & (tt > 0)
    out = np.zeros((int(inside.sum()), 3))
    for off in ((0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75)):
        o, d = rays(off)
        o, d = o[inside], d[inside]
        tt = ((M[:3, 3] - o) @ nrm) / (d @ nrm)
        p = o + tt[:, None] * d
        wi = np.stack([-(d @ s), -(d @ t), -(d @ nrm)], axis=1)
        for i in range(len(p)):
            v = xl - p[i]
            r2 = np.sum(v * v, axis=1)
            w = v / np.sqrt(r2)[:, None]
            cosl = np.maximum(-(w @ nl), 0.0)
            wo = np.stack([w @ s, w @ t, w @ nrm], axis=1)
            f = ru.eval_pdf(alpha, eta, k, np.broadcast_to(wi[i], wo.shape), wo)[0]
            out[i] += 0.25 * Le * dA * np.sum(f * (cosl / r2)[:, None], axis=0)
    return inside.reshape(H, W), out


@pytest.mark.parametrize("half", [0.03, 0.25])
@pytest.mark.parametrize("accel", ["brute", "bvh"])
def test_area_light_over_a_rough_plate_direct(mi, capi, accel, half):
    """one square light (half side 0.03: emitter sampling carries the estimate; 0.25: wider than the lobe, BSDF sampling does) in
    the mirror direction of the view over a tilted coloured rough plate (alpha 0.3) in an unlit black box, `direct`: the radiance of
    a pixel on the plate is the integral over the light of f cos Le cos(theta_l) / r^2 (float64 quadrature of the restatement, two
    grids that agree to 1e-3 of the largest pixel).  24 x 24 pixels, 1024 samples, seed 3; the mean over the plate's pixels of
    (film - expectation) is held to five standard errors from the per-pixel spread."""
    T = mi.ScalarTransform4f
    Le, spp, alpha = 5.0, 1024, 0.3
    tw = T().rotate([1, 0, 0], 25.0) @ T().rotate([0, 1, 0], 180.0) @ T().scale([0.3, 0.3, 1.0])
    c25, s50, c50 = math.cos(math.radians(25)), math.sin(math.radians(50)), math.cos(math.radians(50))
    centre = 0.6 * np.array([0.0, s50, -c50])                        # along the mirror image of the view axis about the plate's normal
    tl = T().look_at(list(centre), [0, 0, 0], [1, 0, 0]) @ T().scale([half, half, 1.0])
    extra = {"plate": {"type": "rectangle", "to_world": tw,
                       "bsdf": {"type": "roughconductor", "distribution": "ggx", "alpha": alpha,
                                "eta": {"type": "rgb", "value": METAL_ETA}, "k": {"type": "rgb", "value": METAL_K}}},
             "light": {"type": "rectangle", "to_world": tl, "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0, 0, 0]}},
                       "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [Le] * 3}}}}
    sc = _box(mi, {"type": "direct"}, extra, res=24, spp=spp, lit=False)
    sc.accel = _accel(capi, accel)
    img = mi.render(sc, seed=3, spp=spp)
    M, Ml = np.asarray(tw.matrix, np.float64), np.asarray(tl.matrix, np.float64)
    assert abs(c25 - -(M[:3, :3] @ [0, 0, 1] / np.linalg.norm(M[:3, :3] @ [0, 0, 1]))[2]) < 1e-9
    key = ("light", half)
    if key not in _E_CACHE:
        n = 32 if half < 0.1 else 96
        inside, e1 = _light_expectation(sc.sensors()[0], M, Ml, alpha, METAL_ETA, METAL_K, Le, n)
        _, e2 = _light_expectation(sc.sensors()[0], M, Ml, alpha, METAL_ETA, METAL_K, Le, n // 2)
        assert np.abs(e1 - e2).max() < 1e-3 * e1.max()
        _E_CACHE[key] = (inside, e1)
    inside, want = _E_CACHE[key]
    diff = img[inside].astype(np.float64) - want
    mean, se = diff.mean(axis=0), diff.std(axis=0, ddof=1) / math.sqrt(len(diff))
    print(f"{accel} light {half}: pixels {len(diff)} mean(film) {img[inside].mean(axis=0)} mean(want) {want.mean(axis=0)} diff {mean} se {se}")
    assert want.max() > 1e-3 and np.all(se > 0) and np.all(np.abs(mean) <= 5 * se), (mean, se)


# ---- (e) launch structures -----------------------------------------------------------------------------------------------------------
def _mixed(mi, capi, accel, spp=8, res=40):
    T = mi.ScalarTransform4f
    extra = {"plate": {"type": "rectangle", "to_world": T().rotate([1, 0, 0], 25.0) @ T().rotate([0, 1, 0], 180.0) @ T().scale([0.5, 0.4, 1.0]),
                       "bsdf": {"type": "roughconductor", "distribution": "ggx", "alpha": 0.2,
                                "eta": {"type": "rgb", "value": METAL_ETA}, "k": {"type": "rgb", "value": METAL_K}}},
             "tube": {"type": "cylinder", "p0": [-0.4, -0.6, -0.3], "p1": [-0.4, 0.6, -0.3], "radius": 0.1,
                      "bsdf": {"type": "roughconductor", "distribution": "ggx", "alpha": 0.05}},
             "ball": {"type": "sphere", "center": [0.35, -0.3, -0.4], "radius": 0.12, "bsdf": {"type": "conductor", "eta": 1.2, "k": 2.5}},
             "lamp": {"type": "point", "position": [0.2, 0.6, -0.7], "intensity": {"type": "rgb", "value": [0.5, 0.4, 0.3]}}}
    sc = _box(mi, {"type": "path", "max_depth": 5}, extra, res=res, spp=spp, Le=0.3)
    sc.accel = _accel(capi, accel)
    return sc


def test_launch_structures_and_pass_sizes_agree(mi, capi):
    """a scene with two rough conductors, a Fresnel conductor, area lights and a point light: the brute-force kernels, the BVH
    streams on a tree in LDS and in global memory render array_equal films, whatever the pass size"""
    films = {}
    for accel in ("brute", "bvh", "bvh_global"):
        sc = _mixed(mi, capi, accel)
        integ = sc.integrator()
        films[accel] = integ.render(sc, seed=4, spp=8)
        for pp in (40 * 40 * 3, 1000):
            assert np.array_equal(integ.render(sc, seed=4, spp=8, pass_paths=pp), films[accel]), (accel, pp)
    assert np.isfinite(films["brute"]).all() and films["brute"].std() > 0
    assert np.array_equal(films["bvh"], films["brute"]) and np.array_equal(films["bvh_global"], films["brute"])


@pytest.mark.parametrize("accel", ["brute", "bvh"])
def test_integrator_sample_on_a_renders_own_rays(mi, capi, accel):
    from test_gpu_radiance import _render_rays
    sc = _mixed(mi, capi, accel, spp=1, res=24)
    integ, sens = sc.integrator(), sc.sensors()[0]
    W, H = sens.film().size()
    ray = _render_rays(mi, sc, 9, 2)
    rgb, _, _ = integ.sample(sc, mi.Sampler(mi.Properties("independent", dict(seed=9, sample_index=2))), ray)
    film = integ.render(sc, seed=9, spp=1, sample_offset=2)
    assert film.std() > 0 and np.array_equal(rgb.reshape(H, W, 3), film)


# ---- (f) the prototype scene ---------------------------------------------------------------------------------------------------------
def test_prototype_scene_renders(mi):
    sc = mi.load_dict(prototype_dict(mi))
    img = mi.render(sc, seed=1)
    assert img.shape == (64, 64, 3) and not img.any()                                  # no emitter: exact zeros
    d = prototype_dict(mi)
    d["lamp"] = {"type": "point", "position": [0.5, 0.5, 2.0], "intensity": {"type": "rgb", "value": [3.0, 3.0, 3.0]}}
    img = mi.render(mi.load_dict(d), seed=1)
    assert np.isfinite(img).all()
    # the tube covers the columns |x| < 0.2 at distance 2 (fov 28.8 degrees by default): the centre columns are lit, the margin is not
    assert img[16:48, 30:34].mean() > 1e-3 and not img[:, :8].any() and not img[:, -8:].any()


# ---- (g) parameter update ------------------------------------------------------------------------------------------------------------
def test_alpha_update_reaches_the_device(mi, capi):
    sc = _mixed(mi, capi, "brute")
    a = mi.render(sc, seed=6)
    params = mi.traverse(sc)
    params["plate.bsdf.alpha"] = 0.6
    params.update()
    b = mi.render(sc, seed=6)
    params["plate.bsdf.alpha"] = 0.2
    params.update()
    c = mi.render(sc, seed=6)
    assert not np.array_equal(a, b) and np.array_equal(a, c)


def test_a_material_update_can_bring_the_first_rough_conductor(mi, capi):
    """a scene created without one runs the instances without the code; an update to type 5 must switch it over, and back"""
    for accel in ("brute", "bvh"):
        sc = _box(mi, {"type": "path", "max_depth": 4}, {"ball": {"type": "sphere", "radius": 0.3, "bsdf": {"type": "diffuse"}}})
        sc.accel = _accel(capi, accel)
        a = mi.render(sc, seed=2, spp=8)
        dev = sc.device()
        idx = [i for i, b in enumerate(sc.flatten()["material_objects"]) if isinstance(b, mi.DiffuseBSDF) and b.reflectance[0] == 0.5][0]
        dev.update_material(idx, capi.make_material(capi.MAT_ROUGHCONDUCTOR, [0.3, *METAL_ETA, *METAL_K]))
        b = mi.render(sc, seed=2, spp=8)
        want = _box(mi, {"type": "path", "max_depth": 4}, {"ball": {"type": "sphere", "radius": 0.3, "bsdf": {
            "type": "roughconductor", "distribution": "ggx", "alpha": 0.3, "eta": {"type": "rgb", "value": METAL_ETA},
            "k": {"type": "rgb", "value": METAL_K}}}})
        want.accel = _accel(capi, accel)
        assert np.array_equal(b, mi.render(want, seed=2, spp=8)) and not np.array_equal(a, b)
        dev.update_material(idx, capi.make_material(capi.MAT_DIFFUSE, [0.5, 0.5, 0.5]))
        assert np.array_equal(mi.render(sc, seed=2, spp=8), a)
