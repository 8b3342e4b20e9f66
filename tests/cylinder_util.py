"""Float64 restatement of the analytic cylinder (include/pbrt_hip.h PBRT_PRIM_CYLINDER) for the tests.  The CPU
oracle does not know the primitive, so the shape's definition is written out here once more, independently of scene.py and the
kernels: the open unit tube x^2 + y^2 = 1, 0 <= z <= 1 under object -> world = to_world @ translate(p0) @ frame @
scale(radius, radius, L).  The tube is symmetric about its axis, so any right-handed orthonormal frame around (p1 - p0) / L
gives the same surface (Mitsuba's to_frame is one of them)."""
import numpy as np


def axis_frame(a):
    """a right-handed orthonormal basis (u, v, a) around the unit vector a (columns of the returned 3 x 3)"""
    a = np.asarray(a, np.float64)
    h = np.array([1.0, 0.0, 0.0]) if abs(a[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    u = np.cross(h, a)
    u /= np.linalg.norm(u)
    return np.stack([u, np.cross(a, u), a], axis=1)


def object_to_world(p0=(0.0, 0.0, 0.0), p1=(0.0, 0.0, 1.0), radius=1.0, to_world=None):
    """4 x 4 object -> world matrix of the tube (to_world: 4 x 4 array or None)"""
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    L = np.linalg.norm(p1 - p0)
    m = np.eye(4)
    m[:3, :3] = axis_frame((p1 - p0) / L) @ np.diag([radius, radius, L])
    m[:3, 3] = p0
    return (np.eye(4) if to_world is None else np.asarray(to_world, np.float64)) @ m


def surface_points(O, phi, s):
    """world points of the tube at angle phi and height s in [0, 1] (object coordinates (cos phi, sin phi, s))"""
    q = np.stack([np.cos(phi), np.sin(phi), s, np.ones_like(s)], axis=-1)
    return (q @ O.T)[..., :3]


def record_matrix(rec):
    """the 3 x 4 world -> object matrix a PRIM_CYLINDER record carries, in float64"""
    return np.asarray(rec["g"], np.float64).reshape(3, 4)


def intersect(W, o, d, tmax=None):
    """Nearest hit of rays (o, d) [n, 3] with the tube whose world -> object matrix is W (3 x 4), in float64, from the
    definition: the roots of |x_o(t)|^2 + |y_o(t)|^2 = 1 in [0, tmax] whose z_o lies in [0, 1].
    -> dict(valid, t, n (geometric normal, +-M^T (x_o, y_o, 0) by the sign of det(M)), p, margin, chord): `margin` is small where
    the answer is numerically ambiguous for a float32 implementation -- a root near a rim (|z_o| or |z_o - 1|), a ray close to
    tangent (|disc| / A, the squared half chord or squared gap in object units), an origin on the wall (|C| = |x_o^2 + y_o^2 - 1|),
    or a root near 0 / tmax (relative).  `chord` is |disc| / A and `gap` is |C| alone: the float32 t of a near-tangent root carries a
    relative error of about eps sqrt(b^2 / disc), the near root of an origin close to the wall one of about eps / |C|."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n = len(o)
    tmax = np.full(n, np.inf) if tmax is None else np.broadcast_to(np.asarray(tmax, np.float64), (n,))
    M, w = W[:, :3], W[:, 3]
    oo, dd = o @ M.T + w, d @ M.T
    A = dd[:, 0] ** 2 + dd[:, 1] ** 2
    b = oo[:, 0] * dd[:, 0] + oo[:, 1] * dd[:, 1]
    C = oo[:, 0] ** 2 + oo[:, 1] ** 2 - 1.0
    disc = b * b - A * C
    with np.errstate(divide="ignore", invalid="ignore"):
        sq = np.sqrt(np.maximum(disc, 0.0))
        roots = np.stack([(-b - sq) / A, (-b + sq) / A], axis=1)
        z = oo[:, 2:3] + roots * dd[:, 2:3]
        ok = (disc[:, None] >= 0) & (A[:, None] > 0) & (roots >= 0) & (roots <= tmax[:, None]) & (z >= 0) & (z <= 1)
        t = np.where(ok, roots, np.inf).min(axis=1)
        valid = np.isfinite(t)
        tt = np.where(valid, t, 0.0)
        p = o + tt[:, None] * d
        q = p @ M.T + w
        nrm = np.stack([q[:, 0], q[:, 1], np.zeros(n)], axis=1) @ M
        nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
        nrm *= np.sign(np.linalg.det(M))
        cand = (disc[:, None] >= 0) & (A[:, None] > 0) & (roots >= 0)
        rim = np.where(cand, np.minimum(np.abs(z), np.abs(z - 1.0)), np.inf).min(axis=1)
        tang = np.where(A > 0, np.abs(disc) / np.where(A > 0, A, 1.0), 0.0)
        scale = np.maximum(np.abs(roots).max(axis=1, initial=0.0, where=np.isfinite(roots)), 1e-30)
        near0 = np.where(cand, np.abs(roots) / scale[:, None], np.inf).min(axis=1)
        neartm = np.where(np.isfinite(tmax), np.abs(roots - tmax[:, None]).min(axis=1) / np.maximum(tmax, 1e-30), np.inf)
        gap = np.abs(C)
        margin = np.minimum(np.minimum(np.minimum(rim, tang), np.minimum(near0, neartm)), gap)
    return dict(valid=valid, t=np.where(valid, t, np.inf), n=np.where(valid[:, None], nrm, 0.0), p=p, margin=margin, chord=tang, gap=gap)
