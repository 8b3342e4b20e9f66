"""K13: an INDEPENDENT float64 estimator of the radiance film, the scenes it is run on, and the three
criteria that hold a rendered film to it.

Nothing here comes from oracle/, tests/golden/ref_transcription.py or the package's device layer: the geometry is built from the plain
scene dicts below (world-space rectangles, triangles, spheres, materials, lights, a look-at camera), never from Scene.flatten(); the
draws come from numpy's PCG64.  It is a DIFFERENT estimator with the same expectation as the build's path tracer:

  * at every diffuse vertex one next-event sample to EVERY emitter (no emitter pick, no selection factor), with NO multiple importance
    sampling; emitted radiance is therefore counted only at the camera vertex and after a specular bounce;
  * no Russian roulette; plain truncation: hits at indices 0 .. max_depth - 1, next-event estimation at vertex k only if
    k + 1 < max_depth (the rule of shade_step in csrc/kernels_radiance.h);
  * cosine hemisphere by the polar form (sqrt(u), 2 pi v); a point on an emitting triangle mesh by an exact float64 area pick and the
    fold (u, v) -> (1 - u, 1 - v) if u + v > 1; planar primitives are met through their dual basis, not Moeller-Trumbore;
  * diffuse is one-sided, `conductor` a one-sided perfect mirror, `dielectric` picks reflection with probability F and scales radiance
    by eta_ti^2 on refraction (Mitsuba's published plugin); area emitters are one-sided, point emitters radiate I / d^2;
  * Mitsuba's `perspective` sensor: x-fov, d = ((1 - 2 sx) tx, (1 - 2 sy) ty, 1) in the look-at frame (left, up', dir);
  * film: box = a sample lands in its own pixel; tent of radius 1 = sum w L / sum w over the samples within the radius (samples exist
    inside the film only), normalised per batch.

render_batches() returns the batch means [B, H, W, 3].  to_mitsuba_dict() turns a scene dict into the dict load_dict() reads."""
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
MESHES = os.path.join(HERE, "scenes", "meshes")
SCENES = ("box", "box_direct", "box_tent", "meshlight_glass")
T_MIN = 1e-9          # rays leave the surface they start on (scenes of unit size, float64)
SHADOW_SHORTEN = 1e-7  # a shadow segment ends this fraction before the sampled point


# ---------------------------------------------------------------------------------------------------------------------------------
# scene descriptions
# ---------------------------------------------------------------------------------------------------------------------------------
def _translate(v):
    m = np.eye(4)
    m[:3, 3] = v
    return m


def _scale(v):
    v = np.broadcast_to(np.asarray(v, float), (3,))
    return np.diag([v[0], v[1], v[2], 1.0])


def _rotate(axis, deg):
    """Rodrigues rotation about a coordinate axis ('x', 'y', 'z'), right-handed, degrees."""
    k = np.zeros(3)
    k["xyz".index(axis)] = 1.0
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    t = math.radians(deg)
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)
    return m


def _rect(name, chain, material, radiance=None):
    """the square [-1, 1]^2 of the xy-plane (normal +z) under the product of `chain` -> world-space corner and edges"""
    M = np.eye(4)
    for m in chain:
        M = M @ m
    c = (M @ np.array([[-1, -1, 0, 1], [1, -1, 0, 1], [-1, 1, 0, 1.0]]).T).T[:, :3]
    return {"name": name, "p0": c[0].tolist(), "e1": (c[1] - c[0]).tolist(), "e2": (c[2] - c[0]).tolist(), "material": material,
            "radiance": radiance}


def _box_scene(integrator, rfilter):
    """the K13 box: five walls at +-1 open towards the camera, two area lights of different size and colour,
    a point light, a mirror and an occluder"""
    T, R, S = _translate, _rotate, _scale
    return {
        "integrator": integrator,
        "film": {"width": 8, "height": 8, "filter": rfilter},
        "camera": {"origin": [0, 0, 3.6], "target": [0, 0, 0], "up": [0, 1, 0], "fov": 38.0, "near": 1e-3, "far": 100.0},
        "materials": {"grey": {"type": "diffuse", "rgb": [0.7, 0.7, 0.7]}, "red": {"type": "diffuse", "rgb": [0.6, 0.1, 0.1]},
                      "green": {"type": "diffuse", "rgb": [0.1, 0.6, 0.1]}, "black": {"type": "diffuse", "rgb": [0.0, 0.0, 0.0]},
                      "half": {"type": "diffuse", "rgb": [0.5, 0.5, 0.5]},     # Mitsuba's default BSDF, spelled out
                      "bluish": {"type": "diffuse", "rgb": [0.5, 0.5, 0.8]}, "mirror": {"type": "conductor"}},
        "rectangles": [
            _rect("floor", [T([0, -1, 0]), R("x", -90)], "grey"),
            _rect("ceiling", [T([0, 1, 0]), R("x", 90)], "grey"),
            _rect("back", [T([0, 0, -1])], "grey"),
            _rect("left", [T([-1, 0, 0]), R("y", 90)], "red"),
            _rect("right", [T([1, 0, 0]), R("y", -90)], "green"),
            _rect("lamp", [T([0.2, 0.98, -0.1]), R("x", 90), S(0.3)], "black", [9.0, 8.0, 6.0]),
            _rect("lamp2", [T([-0.97, -0.3, 0.2]), R("y", 90), S([0.5, 0.2, 1])], "half", [1.0, 2.0, 3.0]),
            _rect("mirror", [T([0.35, -0.45, -0.3]), R("y", -35), R("x", -20), S([0.4, 0.5, 1])], "mirror"),
            _rect("blocker", [T([-0.3, 0.1, 0]), R("x", 70), S(0.3)], "bluish")],
        "meshes": [], "spheres": [],
        "points": [{"name": "bulb", "position": [0.5, 0.3, 0.6], "intensity": [0.6, 0.5, 0.4]}]}


TRILIGHT_OBJ = "k13_trilight.obj"
# the emitting mesh of `meshlight_glass`: three triangles just under the ceiling, areas 0.16 : 0.31 : 0.62 (1.09 of the ceiling's 4),
# normals -y, nine vertices of their own (no two triangles share an edge, none pairs into a parallelogram)
TRILIGHT = [[[-0.9, 0.98, -0.9], [-0.1, 0.98, -0.9], [-0.8, 0.98, -0.5]],
            [[0.0, 0.98, -0.9], [0.9, 0.98, -0.8], [0.1, 0.98, -0.2]],
            [[-0.8, 0.98, -0.1], [0.8, 0.98, 0.0], [-0.4, 0.98, 0.7]]]


def _meshlight_glass_scene():
    """a closed diffuse room [-1, 1]^3 seen from inside: an emitting mesh of three triangles, a glass and a diffuse sphere, a second,
    rectangular light on the right wall; roulette acts from the second bounce on (rr_depth 2)"""
    T, R, S = _translate, _rotate, _scale
    return {
        "integrator": {"type": "path", "max_depth": 8, "rr_depth": 2},
        "film": {"width": 8, "height": 8, "filter": "box"},
        "camera": {"origin": [0.0, 0.1, 0.9], "target": [0.0, -0.25, -1.0], "up": [0, 1, 0], "fov": 80.0, "near": 1e-3, "far": 100.0},
        "materials": {"grey": {"type": "diffuse", "rgb": [0.7, 0.7, 0.7]}, "red": {"type": "diffuse", "rgb": [0.6, 0.1, 0.1]},
                      "green": {"type": "diffuse", "rgb": [0.1, 0.6, 0.1]}, "black": {"type": "diffuse", "rgb": [0.0, 0.0, 0.0]},
                      "ochre": {"type": "diffuse", "rgb": [0.6, 0.6, 0.3]}, "glass": {"type": "dielectric", "eta": 1.5}},
        "rectangles": [
            _rect("floor", [T([0, -1, 0]), R("x", -90)], "grey"),
            _rect("ceiling", [T([0, 1, 0]), R("x", 90)], "grey"),
            _rect("back", [T([0, 0, -1])], "grey"),
            _rect("front", [T([0, 0, 1]), R("y", 180)], "grey"),
            _rect("left", [T([-1, 0, 0]), R("y", 90)], "red"),
            _rect("right", [T([1, 0, 0]), R("y", -90)], "green"),
            _rect("panel", [T([0.97, 0.2, 0.1]), R("y", -90), S([0.25, 0.15, 1])], "black", [2.0, 3.0, 5.0])],
        "meshes": [{"name": "trilight", "file": TRILIGHT_OBJ, "triangles": TRILIGHT, "material": "black", "radiance": [4.0, 3.5, 3.0]}],
        "spheres": [{"name": "glassball", "center": [-0.4, -0.6, -0.2], "radius": 0.4, "material": "glass"},
                    {"name": "ball", "center": [0.5, -0.7, -0.4], "radius": 0.3, "material": "ochre"}],
        "points": []}


def scene(name):
    if name == "box":
        return _box_scene({"type": "path", "max_depth": 6, "rr_depth": 3}, "box")
    if name == "box_direct":
        return _box_scene({"type": "direct"}, "box")
    if name == "box_tent":
        return _box_scene({"type": "path", "max_depth": 6, "rr_depth": 3}, "tent")
    if name == "meshlight_glass":
        return _meshlight_glass_scene()
    raise KeyError(name)


def depth_budget(sc):
    """hits a path may make: `direct` is one emitter sample and one BSDF sample at the first vertex, i.e. a budget of 2"""
    return 2 if sc["integrator"]["type"] == "direct" else int(sc["integrator"]["max_depth"])


def read_obj_triangles(path):
    """`v` and three-index `f` lines of a Wavefront file -> [n, 3, 3]"""
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            w = line.split()
            if w and w[0] == "v":
                v.append([float(x) for x in w[1:4]])
            elif w and w[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in w[1:4]])
    return np.asarray(v)[np.asarray(f)]


def to_mitsuba_dict(sc, mi, mesh_dir=MESHES):
    """scene dict -> the dict mi.load_dict() reads (rectangles as the unit square under [e1 / 2 | e2 / 2 | n | centre])"""
    def bsdf(m):
        m = sc["materials"][m]
        if m["type"] == "diffuse":
            return {"type": "diffuse", "reflectance": {"type": "rgb", "value": list(m["rgb"])}}
        if m["type"] == "conductor":
            return {"type": "conductor"}
        return {"type": "dielectric", "int_ior": float(m["eta"]), "ext_ior": 1.0}

    def light(rad):
        return {"type": "area", "radiance": {"type": "rgb", "value": list(rad)}}

    cam, film, integ = sc["camera"], sc["film"], dict(sc["integrator"])
    d = {"type": "scene", "integrator": integ,
         "sensor": {"type": "perspective", "fov": cam["fov"], "near_clip": cam["near"], "far_clip": cam["far"],
                    "to_world": mi.ScalarTransform4f().look_at(cam["origin"], cam["target"], cam["up"]),
                    "sampler": {"type": "independent", "sample_count": 4},
                    "film": {"type": "hdrfilm", "width": film["width"], "height": film["height"], "rfilter": {"type": film["filter"]}}}}
    for r in sc["rectangles"]:
        p0, e1, e2 = (np.asarray(r[k], float) for k in ("p0", "e1", "e2"))
        n = np.cross(e1, e2)
        M = np.eye(4)
        M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = e1 / 2, e2 / 2, n / np.linalg.norm(n), p0 + (e1 + e2) / 2
        d[r["name"]] = {"type": "rectangle", "to_world": mi.ScalarTransform4f(M), "bsdf": bsdf(r["material"])}
        if r["radiance"] is not None:
            d[r["name"]]["emitter"] = light(r["radiance"])
    for m in sc["meshes"]:
        d[m["name"]] = {"type": "obj", "filename": os.path.join(mesh_dir, m["file"]), "bsdf": bsdf(m["material"]),
                        "emitter": light(m["radiance"])}
    for s in sc["spheres"]:
        d[s["name"]] = {"type": "sphere", "center": list(s["center"]), "radius": float(s["radius"]), "bsdf": bsdf(s["material"])}
    for p in sc["points"]:
        d[p["name"]] = {"type": "point", "position": list(p["position"]), "intensity": {"type": "rgb", "value": list(p["intensity"])}}
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# the estimator
# ---------------------------------------------------------------------------------------------------------------------------------
DIFFUSE, MIRROR, GLASS = 0, 1, 2


class _Compiled:
    """flat float64 arrays of a scene dict: planar primitives (parallelograms, then triangles) first, spheres after them"""

    def __init__(self, sc):
        mats = sc["materials"]
        planar, self.lights = [], []   # lights: dict(kind, prims, areas, radiance) | dict(kind, position, intensity)
        for r in sc["rectangles"]:
            planar.append((r["p0"], r["e1"], r["e2"], False, r["material"], r["radiance"]))
            if r["radiance"] is not None:
                self.lights.append({"kind": "area", "prims": [len(planar) - 1], "radiance": np.asarray(r["radiance"], float)})
        for m in sc["meshes"]:
            first = len(planar)
            for tri in m["triangles"]:
                v = np.asarray(tri, float)
                planar.append((v[0], v[1] - v[0], v[2] - v[0], True, m["material"], m["radiance"]))
            if m["radiance"] is not None:
                self.lights.append({"kind": "area", "prims": list(range(first, len(planar))), "radiance": np.asarray(m["radiance"], float)})
        for p in sc["points"]:
            self.lights.append({"kind": "point", "position": np.asarray(p["position"], float), "intensity": np.asarray(p["intensity"], float)})
        self.n_planar = len(planar)
        self.P0 = np.array([p[0] for p in planar], float).reshape(-1, 3)
        self.E1 = np.array([p[1] for p in planar], float).reshape(-1, 3)
        self.E2 = np.array([p[2] for p in planar], float).reshape(-1, 3)
        self.tri = np.array([p[3] for p in planar], bool)
        cr = np.cross(self.E1, self.E2)
        ln = np.linalg.norm(cr, axis=1)
        self.N = cr / ln[:, None]
        self.area = np.where(self.tri, 0.5 * ln, ln)
        # dual basis in the primitive's plane: A1 . e1 = 1, A1 . e2 = 0, A2 . e1 = 0, A2 . e2 = 1
        a1, a2 = np.cross(self.E2, self.N), np.cross(self.N, self.E1)
        self.A1 = a1 / np.sum(a1 * self.E1, axis=1, keepdims=True)
        self.A2 = a2 / np.sum(a2 * self.E2, axis=1, keepdims=True)
        self.p0n, self.p0a1, self.p0a2 = (np.sum(self.P0 * x, axis=1) for x in (self.N, self.A1, self.A2))
        self.C = np.array([s["center"] for s in sc["spheres"]], float).reshape(-1, 3)
        self.R = np.array([s["radius"] for s in sc["spheres"]], float)
        names = [p[4] for p in planar] + [s["material"] for s in sc["spheres"]]
        kind = {"diffuse": DIFFUSE, "conductor": MIRROR, "dielectric": GLASS}
        self.mtype = np.array([kind[mats[m]["type"]] for m in names])
        self.rgb = np.array([mats[m].get("rgb", [1.0, 1.0, 1.0]) for m in names], float)
        self.eta = np.array([mats[m].get("eta", 1.0) for m in names], float)
        self.Le = np.array([p[5] if p[5] is not None else [0.0, 0.0, 0.0] for p in planar] + [[0.0, 0.0, 0.0]] * len(self.R), float)
        for L in self.lights:
            if L["kind"] == "area":
                a = self.area[L["prims"]]
                L["area"] = float(a.sum())
                L["cdf"] = np.cumsum(a) / a.sum()

    def closest(self, o, d):
        """-> t [n] (inf: no hit), primitive index [n] (-1: none)"""
        n = len(o)
        best_t, best_p = np.full(n, np.inf), np.full(n, -1)
        if self.n_planar:
            t, ok = self._planar(o, d)
            t = np.where(ok, t, np.inf)
            best_p = np.argmin(t, axis=1)
            best_t = t[np.arange(n), best_p]
            best_p = np.where(np.isfinite(best_t), best_p, -1)
        for j in range(len(self.R)):
            t = self._sphere(j, o, d)
            nearer = t < best_t
            best_t = np.where(nearer, t, best_t)
            best_p = np.where(nearer, self.n_planar + j, best_p)
        return best_t, best_p

    def occluded(self, o, d, tmax):
        """anything within (T_MIN, tmax) along the ray"""
        occ = np.zeros(len(o), bool)
        if self.n_planar:
            t, ok = self._planar(o, d)
            occ = np.any(ok & (t < tmax[:, None]), axis=1)
        for j in range(len(self.R)):
            occ |= self._sphere(j, o, d) < tmax
        return occ

    def _planar(self, o, d):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (self.p0n[None, :] - o @ self.N.T) / (d @ self.N.T)
            u = (o @ self.A1.T - self.p0a1[None, :]) + t * (d @ self.A1.T)
            v = (o @ self.A2.T - self.p0a2[None, :]) + t * (d @ self.A2.T)
            ok = (t > T_MIN) & (u >= 0) & (v >= 0) & np.where(self.tri[None, :], u + v <= 1, (u <= 1) & (v <= 1))
        return t, ok

    def _sphere(self, j, o, d):
        oc = o - self.C[j]
        b = np.sum(oc * d, axis=1)
        disc = b * b - (np.sum(oc * oc, axis=1) - self.R[j] ** 2)
        sq = np.sqrt(np.maximum(disc, 0.0))
        t = np.where(-b - sq > T_MIN, -b - sq, -b + sq)
        return np.where((disc > 0) & (t > T_MIN), t, np.inf)

    def normal(self, prim, p):
        """geometric normal at p on primitive `prim` (outward on spheres)"""
        n = np.empty((len(prim), 3))
        pl = prim < self.n_planar
        n[pl] = self.N[prim[pl]]
        j = prim[~pl] - self.n_planar
        n[~pl] = (p[~pl] - self.C[j]) / self.R[j][:, None]
        return n


def _basis(n):
    """two unit vectors orthogonal to the unit vectors n [k, 3] and to each other"""
    a = np.where(np.abs(n[:, :1]) < 0.6, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    s = np.cross(a, n)
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    return s, np.cross(n, s)


def _radiance(cs, rng, o, d, max_depth, light_scale=None):
    """radiance along the rays (o, d): [n, 3]"""
    n = len(o)
    L = np.zeros((n, 3))
    idx = np.arange(n)
    thr = np.ones((n, 3))
    count_emission = np.ones(n, bool)   # camera vertex, or the previous bounce was specular
    scale = np.ones(len(cs.lights)) if light_scale is None else np.asarray(light_scale, float)
    Le = cs.Le.copy()
    for li, lt in enumerate(cs.lights):
        if lt["kind"] == "area":
            Le[lt["prims"]] *= scale[li]
    for k in range(max_depth):
        t, prim = cs.closest(o, d)
        hit = prim >= 0
        idx, o, d, thr, count_emission, t, prim = (x[hit] for x in (idx, o, d, thr, count_emission, t, prim))
        if not len(idx):
            break
        p = o + t[:, None] * d
        ng = cs.normal(prim, p)
        cos_i = -np.sum(ng * d, axis=1)
        front = cos_i > 0
        em = count_emission & front
        L[idx[em]] += thr[em] * Le[prim[em]]
        if k + 1 >= max_depth:
            break
        mt = cs.mtype[prim]
        nd, nthr = np.zeros_like(d), np.zeros_like(thr)
        go = np.zeros(len(idx), bool)
        # ---- diffuse, one-sided: next-event estimation to every emitter, then a cosine-distributed direction
        df = (mt == DIFFUSE) & front
        if df.any():
            pd, nn, rho, th = p[df], ng[df], cs.rgb[prim[df]], thr[df]
            m = len(pd)
            so, sd, smax, sval, srow = [], [], [], [], []
            for li, lt in enumerate(cs.lights):
                if lt["kind"] == "point":
                    dv = lt["position"][None, :] - pd
                    d2 = np.sum(dv * dv, axis=1)
                    dist = np.sqrt(d2)
                    wd = dv / dist[:, None]
                    g = np.maximum(np.sum(wd * nn, axis=1), 0.0) / d2
                    val = th * rho * (g / math.pi)[:, None] * (lt["intensity"] * scale[li])[None, :]
                else:
                    pk = np.asarray(lt["prims"])[np.minimum(np.searchsorted(lt["cdf"], rng.random(m), side="right"), len(lt["prims"]) - 1)]
                    u, v = rng.random(m), rng.random(m)
                    fold = cs.tri[pk] & (u + v > 1)
                    u, v = np.where(fold, 1 - u, u), np.where(fold, 1 - v, v)
                    q = cs.P0[pk] + u[:, None] * cs.E1[pk] + v[:, None] * cs.E2[pk]
                    dv = q - pd
                    d2 = np.sum(dv * dv, axis=1)
                    dist = np.sqrt(d2)
                    wd = dv / dist[:, None]
                    g = np.maximum(np.sum(wd * nn, axis=1), 0.0) * np.maximum(-np.sum(wd * cs.N[pk], axis=1), 0.0) / d2
                    val = th * rho * (g * lt["area"] / math.pi)[:, None] * (lt["radiance"] * scale[li])[None, :]
                use = np.any(val > 0, axis=1)
                so.append(pd[use]); sd.append(wd[use]); smax.append(dist[use] * (1 - SHADOW_SHORTEN)); sval.append(val[use])
                srow.append(np.nonzero(df)[0][use])
            so, sd, smax, sval, srow = (np.concatenate(x) for x in (so, sd, smax, sval, srow))
            if len(so):
                vis = ~cs.occluded(so, sd, smax)
                np.add.at(L, idx[srow[vis]], sval[vis])
            u, v = rng.random(m), rng.random(m)
            r, phi = np.sqrt(u), 2 * math.pi * v
            s, tt = _basis(nn)
            nd[df] = (r * np.cos(phi))[:, None] * s + (r * np.sin(phi))[:, None] * tt + np.sqrt(np.maximum(1 - u, 0.0))[:, None] * nn
            nthr[df] = th * rho
            go |= df & np.any(nthr > 0, axis=1)
        # ---- perfect mirror, one-sided
        mr = (mt == MIRROR) & front
        if mr.any():
            nd[mr] = d[mr] + 2 * cos_i[mr][:, None] * ng[mr]
            nthr[mr] = thr[mr] * cs.rgb[prim[mr]]
            go |= mr
        # ---- smooth dielectric: reflect with probability F, else refract with radiance scaled by eta_ti^2
        gl = mt == GLASS
        if gl.any():
            ci, nn, dd, eta = cos_i[gl], ng[gl], d[gl], cs.eta[prim[gl]]
            eta_ti = np.where(ci >= 0, 1 / eta, eta)       # 1 / (relative index of the medium entered)
            ct2 = 1 - (1 - ci * ci) * eta_ti * eta_ti
            cia, cta = np.abs(ci), np.sqrt(np.maximum(ct2, 0.0))
            eta_it = 1 / eta_ti
            a_s = (cia - eta_it * cta) / (cia + eta_it * cta)
            a_p = (cta - eta_it * cia) / (cta + eta_it * cia)
            F = np.where(ct2 <= 0, 1.0, 0.5 * (a_s * a_s + a_p * a_p))
            refl = rng.random(len(ci)) < F
            ct = -np.sign(ci) * cta
            nd[gl] = np.where(refl[:, None], dd + 2 * ci[:, None] * nn, eta_ti[:, None] * dd + (eta_ti * ci + ct)[:, None] * nn)
            nthr[gl] = thr[gl] * np.where(refl, 1.0, eta_ti * eta_ti)[:, None]
            go |= gl
        spec = (mt != DIFFUSE)
        idx, o, d, thr, count_emission = idx[go], p[go], nd[go], nthr[go], spec[go]
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        if not len(idx):
            break
    return L


def _camera_rays(cam, W, H, fx, fy):
    o = np.asarray(cam["origin"], float)
    fw = np.asarray(cam["target"], float) - o
    fw /= np.linalg.norm(fw)
    left = np.cross(np.asarray(cam["up"], float), fw)
    left /= np.linalg.norm(left)
    up = np.cross(fw, left)
    tx = math.tan(math.radians(cam["fov"]) / 2)
    ty = tx * H / W
    d = ((1 - 2 * fx / W) * tx)[:, None] * left + ((1 - 2 * fy / H) * ty)[:, None] * up + fw
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.broadcast_to(o, d.shape).copy(), d


def render_batches(sc, batches, spp, seed, max_depth=None, light_scale=None, chunk_spp=2048, progress=None):
    """B independent films of `spp` samples per pixel each: [B, H, W, 3] float64.  light_scale: one factor per light in the order
    rectangles, meshes, points (the negative controls).  chunk_spp bounds the memory only."""
    cs = _Compiled(sc)
    W, H, filt = sc["film"]["width"], sc["film"]["height"], sc["film"]["filter"]
    D = depth_budget(sc) if max_depth is None else max_depth
    rng = np.random.default_rng(seed)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    px, py = px.ravel(), py.ravel()
    out = np.zeros((batches, H, W, 3))
    for b in range(batches):
        num, den = np.zeros((H * W, 3)), np.zeros(H * W)
        for s0 in range(0, spp, chunk_spp):
            ns = min(chunk_spp, spp - s0)
            ix, iy = np.repeat(px, ns), np.repeat(py, ns)
            fx, fy = ix + rng.random(len(ix)), iy + rng.random(len(iy))
            o, d = _camera_rays(sc["camera"], W, H, fx, fy)
            L = _radiance(cs, rng, o, d, D, light_scale)
            if filt == "box":
                for c in range(3):
                    num[:, c] += np.bincount(iy * W + ix, weights=L[:, c], minlength=H * W)
                den += np.bincount(iy * W + ix, minlength=H * W)
            else:   # tent of radius 1 around the pixel centres
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        X, Y = ix + dx, iy + dy
                        w = np.maximum(0.0, 1 - np.abs(X + 0.5 - fx)) * np.maximum(0.0, 1 - np.abs(Y + 0.5 - fy))
                        w = np.where((X >= 0) & (X < W) & (Y >= 0) & (Y < H), w, 0.0)
                        k = np.clip(Y, 0, H - 1) * W + np.clip(X, 0, W - 1)
                        for c in range(3):
                            num[:, c] += np.bincount(k, weights=w * L[:, c], minlength=H * W)
                        den += np.bincount(k, weights=w, minlength=H * W)
        out[b] = (num / den[:, None]).reshape(H, W, 3)
        if progress:
            progress(b)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# fixtures and criteria
# ---------------------------------------------------------------------------------------------------------------------------------
def fixture_path(name):
    return os.path.join(GOLDEN, f"k13_{name}.npz")


_FIXTURES = {}


def load_fixture(name):
    """-> dict(batches [B, H, W, 3] float64, scene, seed, spp, seconds, rel_se [3]); read once, shared, never modified"""
    if name not in _FIXTURES:
        with np.load(fixture_path(name)) as z:
            f = {"batches": z["batches"], "scene": json.loads(str(z["scene"])), "seed": int(z["seed"]), "spp": int(z["spp"]),
                 "seconds": float(z["seconds"]), "rel_se": z["rel_se"]}
        f["batches"].setflags(write=False)
        _FIXTURES[name] = f
    return _FIXTURES[name]


def film_mean_rel_se(films):
    """relative standard error per channel of the film mean over independent films [K, H, W, 3]"""
    m = np.asarray(films, np.float64).mean(axis=(1, 2))
    return m.std(axis=0, ddof=1) / math.sqrt(len(m)) / m.mean(axis=0)


def chi2_quantile(p, k):
    try:
        from scipy import stats
        return float(stats.chi2.ppf(p, k))
    except ImportError:   # Wilson-Hilferty
        from statistics import NormalDist
        z = NormalDist().inv_cdf(p)
        return k * (1 - 2 / (9 * k) + z * math.sqrt(2 / (9 * k))) ** 3


Z_PIXEL, Z_MEAN, CHI2_P = 5.0, 4.0, 1 - 1e-6


def compare(films, batches, stride=1):
    """The three criteria between two sets of independent films, [K, H, W, 3] and [B, H, W, 3], in float64.  Standard error of a set
    = spread over its members / sqrt(members); z = difference / sqrt(sum of the two squares).
      1. every pixel and channel            |z| <= 5
      2. per channel, sum z^2 over pixels   <= the 1 - 1e-6 quantile of chi^2(pixels); stride 2 (tent filter: neighbours share samples)
                                            takes every second pixel in x and y
      3. film mean per channel              |z| <= 4, from the members' own film means (correlated pixels handled by construction)
    -> dict of the figures and `ok` (the three verdicts)"""
    a, b = np.asarray(films, np.float64), np.asarray(batches, np.float64)
    va, vb = a.var(axis=0, ddof=1) / len(a), b.var(axis=0, ddof=1) / len(b)
    dz, sz = a.mean(axis=0) - b.mean(axis=0), np.sqrt(va + vb)
    # a pixel without any spread on either side (a mirror that shows no light under `direct`: 0 everywhere) agrees exactly or not at all
    z = np.where(sz > 0, dz / np.where(sz > 0, sz, 1.0), np.where(dz == 0, 0.0, np.inf))
    zs = z[::stride, ::stride]
    npix = zs.shape[0] * zs.shape[1]
    chi2 = (zs * zs).sum(axis=(0, 1))
    ma, mb = a.mean(axis=(1, 2)), b.mean(axis=(1, 2))
    diff = ma.mean(axis=0) - mb.mean(axis=0)
    se = np.sqrt(ma.var(axis=0, ddof=1) / len(ma) + mb.var(axis=0, ddof=1) / len(mb))
    r = {"z_max": float(np.abs(z).max()), "chi2_per_n": chi2 / npix, "chi2_limit_per_n": chi2_quantile(CHI2_P, npix) / npix,
         "mean_rel_diff": diff / mb.mean(axis=0), "mean_rel_se": se / mb.mean(axis=0), "z_mean": diff / se}
    r["ok"] = (bool(np.all(np.abs(z) <= Z_PIXEL)), bool(np.all(r["chi2_per_n"] <= r["chi2_limit_per_n"])),
               bool(np.all(np.abs(r["z_mean"]) <= Z_MEAN)))
    return r


def report(tag, r):
    f = lambda v: "[" + ", ".join(f"{x:+.3f}" for x in v) + "]"
    print(f"{tag}: max|z| {r['z_max']:.2f}  sum z^2 / n {f(r['chi2_per_n'])} (limit {r['chi2_limit_per_n']:.2f})  "
          f"film mean diff % {f(100 * r['mean_rel_diff'])}  se % {f(100 * r['mean_rel_se'])}  z {f(r['z_mean'])}  ok {r['ok']}")
