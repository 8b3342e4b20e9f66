"""Restatement of the rough / Fresnel conductor materials in NumPy: Mitsuba 3's `roughconductor` with an isotropic
GGX distribution and visible-normal sampling, and `fresnel_conductor`.  Every function takes the dtype it computes in: float64 is
the yardstick of the device tests, float32 the same statements at the device's precision (the rounding floor those tests scale
their tolerance by).  All vectors live in the local shading frame, wi is the side the path came from.  NumPy only."""
import numpy as np

ALPHA_MIN = 1e-3  # records below it are evaluated at it (include/pbrt_hip.h)


def _c(dt, v):
    return np.asarray(v, dtype=dt)


def fresnel_conductor(ci, eta, k, dt=np.float64):
    """Mitsuba fresnel_conductor(cos_theta_i, eta + i k): the exact unpolarised reflectance through a^2 + b^2"""
    ci, eta, k = np.broadcast_arrays(_c(dt, ci), _c(dt, eta), _c(dt, k))
    one, two, four, half = (dt(v) for v in (1, 2, 4, 0.5))
    ci2 = ci * ci
    si2 = one - ci2
    si4 = si2 * si2
    t1 = eta * eta - k * k - si2
    a2pb2 = np.sqrt(np.maximum(t1 * t1 + four * (k * eta) * (k * eta), dt(0)))
    a = np.sqrt(np.maximum(half * (a2pb2 + t1), dt(0)))
    term1, term2 = a2pb2 + ci2, two * (a * ci)
    rs = (term1 - term2) / (term1 + term2)
    term3, term4 = a2pb2 * ci2 + si4, term2 * si2
    den = term3 + term4
    with np.errstate(invalid="ignore", divide="ignore"):
        rp = np.where(den > 0, rs * ((term3 - term4) / np.where(den > 0, den, one)), rs)  # eta = k = 0 at normal incidence
    return half * (rs + rp)


def fresnel_dielectric_reflectance(ci, eta):
    """the unpolarised reflectance the dielectric arm of bsdf_sample computes (float64), for ci > 0 from outside"""
    ci = np.asarray(ci, np.float64)
    ct2 = 1.0 - (1.0 - ci * ci) / (eta * eta)
    ct = np.sqrt(np.maximum(ct2, 0.0))
    a_s = (ci - eta * ct) / (ci + eta * ct)
    a_p = (ct - eta * ci) / (ct + eta * ci)
    return np.where(ct2 > 0, 0.5 * (a_s * a_s + a_p * a_p), 1.0)


def normalize(v, dt=np.float64):
    v = _c(dt, v)
    return v / np.sqrt(np.sum(v * v, axis=-1, keepdims=True))


def ggx_d(a2, h, dt=np.float64):
    """D(h) = a2 / (pi ((a2 - 1) h.z^2 + 1)^2), written as a2 / (pi (a2 h.z^2 + h.x^2 + h.y^2)^2) (|h| = 1)"""
    dd = a2 * h[..., 2] * h[..., 2] + (h[..., 0] * h[..., 0] + h[..., 1] * h[..., 1])
    return a2 / (dt(np.pi) * (dd * dd))


def ggx_g1(a2, v, vh, dt=np.float64):
    """2 / (1 + sqrt(1 + a2 tan^2 theta_v)); zero when v . h and v.z differ in sign"""
    z = v[..., 2]
    ok = vh * z > 0
    zs = np.where(ok, z, dt(1))
    t2 = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) / (zs * zs)
    return np.where(ok, dt(2) / (dt(1) + np.sqrt(a2 * t2 + dt(1))), dt(0))


def terms(alpha, eta, k, wi, wo, dt=np.float64, hemisphere=True):
    """-> F [n, 3], dg = D(h) G1(wi) / (4 wi.z) [n], G1(wo) [n], wi . h [n] with h = normalize(wi + wo); all zero unless
    wi.z > 0 and wo.z > 0 (hemisphere=False: wo.z is not looked at -- the density over the full sphere of wo)"""
    wi, wo = _c(dt, wi), _c(dt, wo)
    alpha = max(dt(alpha), dt(ALPHA_MIN))
    a2 = alpha * alpha
    h = normalize(wi + wo, dt)
    wih, woh = np.sum(wi * h, axis=-1), np.sum(wo * h, axis=-1)
    on = wi[..., 2] > 0
    if hemisphere:
        on = on & (wo[..., 2] > 0)
    wz = np.where(on, wi[..., 2], dt(1))
    dg = np.where(on, ggx_d(a2, h, dt) * ggx_g1(a2, wi, wih, dt) / (dt(4) * wz), dt(0))
    g1o = np.where(on, ggx_g1(a2, wo, woh, dt), dt(0))
    F = fresnel_conductor(wih[..., None], _c(dt, eta), _c(dt, k), dt)
    return F, dg, g1o, wih


def eval_pdf(alpha, eta, k, wi, wo, dt=np.float64):
    """-> f cos(theta_o) [n, 3], pdf(wo) [n]"""
    F, dg, g1o, _ = terms(alpha, eta, k, wi, wo, dt)
    return F * (dg * g1o)[..., None], dg


def square_to_disk(u, dt=np.float64):
    """Mitsuba warp::square_to_uniform_disk_concentric"""
    u = _c(dt, u)
    x, y = dt(2) * u[..., 0] - dt(1), dt(2) * u[..., 1] - dt(1)
    q13 = np.abs(x) < np.abs(y)
    r, rp = np.where(q13, y, x), np.where(q13, x, y)
    zero = (x == 0) & (y == 0)
    a = np.where(zero, dt(0), dt(np.pi / 4) * (rp / np.where(zero, dt(1), r)))
    s, c = np.sin(a), np.cos(a)
    return r * np.where(q13, s, c), r * np.where(q13, c, s)


def sample(alpha, eta, k, wi, u, dt=np.float64):
    """the visible-normal sample of the device (Heitz's hemisphere method; which m a given u picks is a build definition)
    -> dict(wo [n, 3], pdf [n], weight [n, 3], valid [n], m [n, 3], margin [n]); margin = min(wi.z, wo.z, |wi . m|): a record
    whose margin is small sits next to one of the sampler's decisions (valid or not, the sign test of G1)"""
    wi = _c(dt, wi)
    alpha_c = max(dt(alpha), dt(ALPHA_MIN))
    ws = normalize(np.stack([alpha_c * wi[..., 0], alpha_c * wi[..., 1], wi[..., 2]], axis=-1), dt)
    l2 = ws[..., 0] * ws[..., 0] + ws[..., 1] * ws[..., 1]
    inv = dt(1) / np.sqrt(np.where(l2 > 0, l2, dt(1)))
    T1 = np.where((l2 > 0)[..., None], np.stack([-ws[..., 1] * inv, ws[..., 0] * inv, np.zeros_like(inv)], axis=-1),
                  _c(dt, [1, 0, 0]))
    T2 = np.cross(ws, T1).astype(dt)
    dx, dy = square_to_disk(u, dt)
    S = dt(0.5) * (dt(1) + ws[..., 2])
    dy = (dt(1) - S) * np.sqrt(np.maximum(dt(1) - dx * dx, dt(0))) + S * dy
    mz = np.sqrt(np.maximum(dt(1) - (dx * dx + dy * dy), dt(0)))
    ms = T1 * dx[..., None] + T2 * dy[..., None] + ws * mz[..., None]
    m = normalize(np.stack([alpha_c * ms[..., 0], alpha_c * ms[..., 1], np.maximum(ms[..., 2], dt(0))], axis=-1), dt)
    wim = np.sum(wi * m, axis=-1)
    wo = dt(2) * wim[..., None] * m - wi
    valid = (wi[..., 2] > 0) & (wo[..., 2] > 0)
    F, dg, g1o, _ = terms(alpha, eta, k, wi, wo, dt)
    valid = valid & (dg > 0)
    margin = np.minimum(np.minimum(wi[..., 2], np.abs(wo[..., 2])), np.abs(wim))
    return dict(wo=wo, pdf=np.where(valid, dg, dt(0)), weight=np.where(valid[..., None], F * g1o[..., None], dt(0)), valid=valid, m=m,
                margin=margin)


def normal_grid(alpha, n):
    """midpoint grid over the hemisphere of microfacet normals that resolves the GGX peak: tan(theta_m) = alpha tan(s),
    s in (0, pi / 2), phi in (0, 2 pi) -> m [n, 2 n, 3], solid angle per node [n, 2 n]"""
    s = (np.arange(n) + 0.5) * (np.pi / 2 / n)
    phi = (np.arange(2 * n) + 0.5) * (np.pi / n)
    th = np.arctan(alpha * np.tan(s))
    dth = alpha / (np.cos(s) ** 2 + (alpha * np.sin(s)) ** 2)  # d theta / d s
    st, ct = np.sin(th), np.cos(th)
    m = np.stack([st[:, None] * np.cos(phi)[None, :], st[:, None] * np.sin(phi)[None, :], np.broadcast_to(ct[:, None], (n, 2 * n))],
                 axis=-1)
    w = (st * dth)[:, None] * (np.pi / 2 / n) * (np.pi / n) * np.ones((1, 2 * n))
    return m, w


def integrate_over_wo(fn, alpha, wi, n):
    """integral of fn(wo) over the directions wo = reflect(wi, m), m on normal_grid with wi . m > 0: d omega_o = 4 (wi . m)
    d omega_m.  (Every wo of the sphere but -wi is the mirror image of wi about exactly one such m.)"""
    m, w = normal_grid(alpha, n)
    wi = np.asarray(wi, np.float64)
    wim = m @ wi
    wo = 2.0 * wim[..., None] * m - wi
    jac = np.where(wim > 0, 4.0 * wim, 0.0) * w
    v = fn(wo.reshape(-1, 3))
    v = v.reshape(m.shape[:2] + v.shape[1:])
    return np.tensordot(jac, v, axes=([0, 1], [0, 1]))


def albedo(alpha, eta, k, mu, n=512):
    """E(mu, alpha) = integral over wo.z > 0 of f cos(theta_o), per channel, for wi = (sqrt(1 - mu^2), 0, mu)"""
    wi = np.array([np.sqrt(max(1.0 - mu * mu, 0.0)), 0.0, mu])
    return integrate_over_wo(lambda wo: eval_pdf(alpha, eta, k, np.broadcast_to(wi, wo.shape), wo)[0], alpha, wi, n)


def draw_inputs(seed, n):
    """the (wi, u) records of the leaf-operator test: cos(theta_i) uniform in [0.3, 1], any azimuth, u uniform in [0, 1)^2"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.3, 1.0, n)
    ph = rng.uniform(0, 2 * np.pi, n)
    r = np.sqrt(1 - z * z)
    wi = normalize(np.stack([r * np.cos(ph), r * np.sin(ph), z], axis=1).astype(np.float32).astype(np.float64)).astype(np.float32)
    u = rng.random((n, 2)).astype(np.float32)
    return wi, u


def rel_err(a, b):
    """max over the records of |a - b| / max(|b|, tiny), b the float64 side"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30))) if a.size else 0.0


def sample_floors(alpha, eta, k, wi, u, min_margin=1e-2):
    """the float32 rounding floor of sample on these inputs: the restatement in np.float32 against float64 on the records whose
    decision margins are at least min_margin in float64 (`decided`; `valid` of them return a direction).
    -> dict(wo = max abs, pdf = max rel, weight = max abs), the float64 sample, decided, decided & valid"""
    r64 = sample(alpha, eta, k, wi, u, np.float64)
    r32 = sample(alpha, eta, k, wi, u, np.float32)
    decided = r64["margin"] >= min_margin
    v = decided & r64["valid"]
    fl = dict(wo=float(np.max(np.abs(r32["wo"][v] - r64["wo"][v]))), pdf=rel_err(r32["pdf"][v], r64["pdf"][v]),
              weight=float(np.max(np.abs(r32["weight"][v] - r64["weight"][v]))))
    return fl, r64, decided, v


def eval_floors(alpha, eta, k, wi, wo):
    """the float32 rounding floor of eval / pdf at (wi, wo), both float32 inputs: max relative error of the float32 restatement
    -> dict(eval, pdf), the float64 f cos [n, 3] and pdf [n]"""
    f64, p64 = eval_pdf(alpha, eta, k, wi, wo, np.float64)
    f32, p32 = eval_pdf(alpha, eta, k, wi, wo, np.float32)
    return dict(eval=rel_err(f32, f64), pdf=rel_err(p32, p64)), f64, p64
