"""Non-finite and out-of-range geometry through the beamformers (include/pbrt_hip.h "non-finite and out-of-range geometry", DESIGN.md
D25) for test_geometry_rule_restatement.py (CPU) and test_gpu_geometry_nonfinite.py (GPU).  Written from the header's words and
sharing no text with the kernels.

  split, linear_index, nearest_index    the integer model of a sample position kept as two parts: saturating conversion with NaN -> 0,
                                        the fraction's carry, a wrapping 32-bit add, an unsigned comparison with T - 1
  f64_linear, f64_nearest               the float64 rule the model is held to where both parts lie inside +-2^31
  poisoned                              the tables of a variant V1 .. V5 on a walk case: {label: tables}
  stand_in                              the CLEAN problem that the rule makes of a variant (V1, V2, V4): what the float64 restatements
                                        of nlbf_util, iq_util, apod_util, capon_util, convex_util and scan_util are given
  rule_image                            delay-and-sum and I/Q under the rule, stated directly in float64 (np.fmin, masked comparisons)
  sees, walked                          the pixels whose aperture reaches into the span of a line of elements, and the pixels of the 8 x 8
                                        tiles that hold one: where a transmission with a non-finite first arrival turns I/Q into NaN
  table_sites                           the three pixels of V6, in different tiles
  restated                              the float64 restatement and its float32 floor for a family on a stand-in, made once

A problem is a dict like walk_cases.geometry's: A, E, fs, tx, elem, x, z, kw (+ left_out and n_a once `margins` ran)."""
import functools

import numpy as np

import apod_util as au
import capon_util as ku
import iq_util as iu
import nlbf_util as nu
from walk_cases import C0, T, geometry

F_D = 3.0e6
NAMES = ("a5_e64_lin_f1_sum", "a6_e65_near_f1_mean", "a5_e65_small_near_f0_sum", "a5_e16_convex_lin_f1_sum",
         "a6_e16_convex_small_near_f0_mean")
BIG = "a11_e130_small_near_f0_sum"            # delay-and-sum and Capon only
#            key            method   p    window    capon (l_prop, delta_l)
FAMILIES = {
    "das": ("das", 2.0, "boxcar", None),
    "pdas2": ("pdas", 2.0, "boxcar", None),
    "pdas3": ("pdas", 3.0, "boxcar", None),
    "fdmas": ("fdmas", 2.0, "boxcar", None),
    "iq": ("iq", 2.0, "boxcar", None),
    "hann_das": ("das", 2.0, "hann", None),
    "hann_iq": ("iq", 2.0, "hann", None),
    "capon_half": ("iq", 2.0, "boxcar", (0.5, 0.01)),
    "capon_one": ("iq", 2.0, "boxcar", (0.0, 0.01)),
}
IQ_WALK = ("iq", "hann_iq")                   # the families whose wave 0 turns a transmission's sum by rot_a


def families_of(name):
    """the families a case runs: the windows need an f-number aperture, the large case is delay-and-sum's and Capon's"""
    fn = geometry(name)["kw"]["f_number"]
    for key in FAMILIES:
        if key.startswith("hann") and not fn > 0:
            continue
        if name == BIG and key not in ("das", "capon_half", "capon_one"):
            continue
        yield key


def is_complex(family):
    return FAMILIES[family][0] == "iq"


def case_data(name, family):
    """capon_util's complex normal data of the case, or its real part for the real-valued families"""
    d = ku.case_data(name, "noise")
    return d if is_complex(family) else np.ascontiguousarray(d.real)


# ---- (a) the integer model of a split position ---------------------------------------------------------------------------------------
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def sat_i32(v):
    """float -> int32 as the hardware converts: towards zero, saturating, NaN -> 0"""
    v = float(v)
    if v != v:
        return 0
    if v >= 2.0 ** 31:
        return I32_MAX
    if v <= -2.0 ** 31:
        return I32_MIN
    return int(v)


def wrap_i32(v):
    """a 32-bit add that wraps"""
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def split(s):
    """a float64 position as (whole samples int32, float32 fraction): floor, saturating conversion, the fraction s - floor(s) rounded to
    float32 (NaN for a non-finite s: the comparison below is then false); a fraction that rounds up to 1 is carried"""
    with np.errstate(invalid="ignore"):
        fl = np.floor(np.float64(s))
        i, f = sat_i32(fl), np.float32(np.float64(s) - fl)
    if f >= np.float32(1.0):
        i, f = wrap_i32(i + 1), np.float32(0.0)
    return i, f


def linear_index(s_tx, s_rx, T):
    """-> (the indices read, the weight): () where nothing is taken, (i0, i0 + 1) between two samples, (T - 1,) exactly on the last"""
    (ti, tf), (ri, rf) = split(s_tx), split(s_rx)
    with np.errstate(invalid="ignore"):
        fr = np.float32(tf + rf)
        fl = np.floor(fr)
        w = np.float32(fr - fl)
    i0 = (ti + ri + sat_i32(fl)) % 2 ** 32               # the wrapping sum, read as unsigned
    if i0 < T - 1:
        return (i0, i0 + 1), w
    if i0 == T - 1 and w == 0.0:
        return (T - 1,), w
    return (), w


def nearest_index(s_tx, s_rx, T):
    """nearest interpolation decides on the float64 sum: rint, two comparisons (false for NaN), then the conversion"""
    with np.errstate(invalid="ignore"):
        r = np.rint(np.float64(s_tx) + np.float64(s_rx))
    return (int(r),) if (r >= 0.0 and r <= float(T - 1)) else ()


def f64_linear(s_tx, s_rx, T):
    """the float64 rule: floor(s) in [0, T - 1), or s == T - 1 -> (taken, s)"""
    s = float(s_tx) + float(s_rx)
    f = np.floor(s)
    return bool((0 <= f < T - 1) or s == T - 1), s


def part_values(T):
    """the parts of section (a): NaN, +-inf, +-1e300, +-(2^31 +- 1), +-2^32, -1, 0, T - 2, T - 1, T, each with the fractions 0 and 1 - 2^-25"""
    bases = [np.nan, np.inf, -np.inf, 1e300, -1e300]
    for sign in (1.0, -1.0):
        bases += [sign * (2.0 ** 31 + 1), sign * (2.0 ** 31 - 1), sign * 2.0 ** 32]
    bases += [-1.0, 0.0, T - 2.0, T - 1.0, float(T)]
    with np.errstate(invalid="ignore"):
        return [np.float64(b) + np.float64(fr) for b in bases for fr in (0.0, 1.0 - 2.0 ** -25)]


# ---- (b) variants and their stand-ins ------------------------------------------------------------------------------------------------
SITE_A, SITE_E = 1, 3                       # the transmission and the element that the variants poison
SITE_E_CONVEX = 7                           # V4 on the element tables: element 3 lies in no aperture of the f# = 1 case, 7 in many, and
#                                             it is the first to arrive at half of the pixels (test_geometry_rule_restatement.py)
BAD_PIXELS = (((2, 5), "x", np.nan), ((4, 7), "z", np.nan), ((6, 1), "z", np.inf), ((1, 3), "x", -np.inf), ((0, 0), "x", 3.0e5))


def problem(g, **changes):
    """a copy of the tables of a problem with some replaced (no margins: `with_margins`)"""
    out = {k: g[k] for k in ("A", "E", "fs", "tx", "elem", "x", "z", "kw")}
    out.update(changes)
    return out


def with_margins(p, t0=0.0):
    left_out, n_a = nu.margins(p["tx"], p["elem"], p["x"], p["z"], T, p["fs"], C0, t0=t0, f_number=p["kw"]["f_number"],
                               interpolation=p["kw"]["interpolation"])
    return dict(p, left_out=left_out, n_a=n_a)


def _convex(g):
    return g["elem"].ndim == 2


def absent(g):
    """the element V4 takes away"""
    return SITE_E_CONVEX if _convex(g) else SITE_E


def poisoned(variant, g):
    """{label: problem} -- the copies of one variant, which must all give the same image"""
    tx, elem = g["tx"], g["elem"]
    E = g["E"]

    def put(a, idx, v):
        a = np.array(a, copy=True)
        a[idx] = v
        return a

    if variant == "V1":
        return {k: problem(g, tx=put(tx, (SITE_A, slice(0, E // 2)), v)) for k, v in (("nan", np.nan), ("+inf", np.inf))}
    if variant == "V2":
        return {"nan": problem(g, tx=put(tx, (SITE_A, slice(None)), np.nan))}
    if variant == "V3":
        return {"-inf": problem(g, tx=put(tx, (SITE_A, SITE_E), -np.inf))}
    if variant == "V4":
        if _convex(g):
            return {"nan": problem(g, elem=put(elem, (absent(g), slice(None)), np.nan))}
        return {k: problem(g, elem=put(elem, absent(g), v)) for k, v in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf))}
    if variant == "V4n":                    # convex only: the two components of the normal
        return {"nan": problem(g, elem=put(elem, (absent(g), slice(2, 4)), np.nan))}
    if variant == "V5":
        return {"axes": problem(g, x=put(g["x"], 2, np.nan), z=put(g["z"], 5, np.inf))}
    raise ValueError(variant)


def bad_pixel_tables(g):
    """V5 on pixel tables: np.meshgrid(x, z) with the five entries of BAD_PIXELS -> (px, pz, bad [nx, nz])"""
    px, pz = (np.array(t, np.float32) for t in np.meshgrid(g["x"], g["z"], indexing="ij"))
    bad = np.zeros(px.shape, bool)
    for (ix, iz), which, v in BAD_PIXELS:
        (px if which == "x" else pz)[ix, iz] = v
        bad[ix, iz] = True
    return px, pz, bad


def stand_in(variant, g, data):
    """-> (problem with margins, data): the clean problem a variant is under the rule.
      V1, V2   the poisoned delays are 1e30: no minimum, and alone they put every position beyond the trace
      V4       element absent(g) deleted from the tables and from the traces (E - 1 elements)
      V4n      (convex) f# > 0: the element keeps its place in the first arrival and receives nothing -- its normal turned round, so that
               d_n > 0 fails at every pixel in front of it; f# <= 0: the normals are not read, the clean problem"""
    tx, elem, E = g["tx"], g["elem"], g["E"]
    if variant in ("V1", "V2"):
        t = np.array(tx, copy=True)
        t[SITE_A, :(E // 2 if variant == "V1" else E)] = 1e30
        return with_margins(problem(g, tx=t)), data
    if variant == "V4":
        keep = np.arange(E) != absent(g)
        return with_margins(problem(g, E=E - 1, tx=np.ascontiguousarray(tx[:, keep]), elem=np.ascontiguousarray(elem[keep]))), \
            np.ascontiguousarray(np.asarray(data)[:, keep])
    if variant == "V4n":
        if not g["kw"]["f_number"] > 0:
            return with_margins(problem(g)), data
        el = np.array(elem, copy=True)
        el[absent(g), 2:4] = -el[absent(g), 2:4]
        return with_margins(problem(g, elem=el)), data
    raise ValueError(variant)


# ---- the rule, stated directly (delay-and-sum and I/Q) -------------------------------------------------------------------------------
def rule_image(data, p, f_d=None, t0=0.0):
    """delay-and-sum (f_d None) or I/Q of possibly poisoned tables under the header's rule, in float64 -> (image, B).
    first arrival: the minimum over the elements whose tx + d / c is not NaN, 1e300 where there is none; a term (a, e) is taken iff the
    aperture comparison holds and the position lies in the trace (both false for NaN); linear interpolation refuses a position of which
    a part lies beyond +-2^31 samples"""
    f64 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    data = np.asarray(data)
    A, E, Tn = data.shape
    tx, el, gx, gz = f64(p["tx"]), f64(p["elem"]), f64(p["x"]).ravel(), f64(p["z"]).ravel()
    kw = p["kw"]
    fs, c, fn, t0 = float(np.float32(p["fs"])), float(np.float32(C0)), float(np.float32(kw["f_number"] or 0.0)), float(np.float32(t0))
    X, Z = np.meshgrid(gx, gz, indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        if el.ndim == 2:
            dx, dz = X[None] - el[:, 0, None, None], Z[None] - el[:, 1, None, None]
            dn = dx * el[:, 2, None, None] + dz * el[:, 3, None, None]
            dt = dx * el[:, 3, None, None] - dz * el[:, 2, None, None]
            ap = (dn > 0) & (2.0 * fn * np.abs(dt) <= dn) if fn > 0 else np.ones(dx.shape, bool)
        else:
            dx, dz = X[None] - el[:, None, None], np.broadcast_to(Z[None], (E,) + X.shape)
            ap = np.abs(dx) <= (Z[None] / (2.0 * fn) if fn > 0 else 1e300)
        d = np.sqrt(dx * dx + dz * dz) / c
        ee = np.arange(E)[:, None, None]
        img = np.zeros(X.shape, np.complex128 if f_d is not None else np.float64)
        B = np.zeros(X.shape)
        for a in range(A):
            t_tx = np.fmin.reduce(tx[a][:, None, None] + d, axis=0, initial=1e300)
            s_tx, s_rx = (t_tx - t0) * fs, d * fs
            s = (t_tx[None] + d - t0) * fs
            if kw["interpolation"] == "nearest":
                r = np.rint(s)
                ok = ap & (r >= 0) & (r <= Tn - 1)
                val = data[a][ee, np.where(ok, r, 0).astype(int)].astype(img.dtype)
            else:
                f = np.floor(s)
                ok = ap & (np.abs(s_tx)[None] < 2.0 ** 31) & (np.abs(s_rx) < 2.0 ** 31) & (((f >= 0) & (f < Tn - 1)) | (s == Tn - 1))
                i0 = np.where(ok, f, 0).astype(int)
                w = np.where(ok, s - f, 0.0).astype(np.float32).astype(np.float64)
                v0, v1 = data[a][ee, i0].astype(img.dtype), data[a][ee, np.minimum(i0 + 1, Tn - 1)].astype(img.dtype)
                val = v0 + w * (v1 - v0)
            val = np.where(ok, val, 0)
            B += np.abs(val).sum(axis=0)
            if f_d is None:
                img += val.sum(axis=0)
            else:
                fd = float(np.float32(f_d))
                rot_e = np.exp(2j * np.pi * np.where(ok, fd * d - np.floor(fd * d), 0.0))
                rot_a = np.exp(2j * np.pi * (fd * t_tx - np.floor(fd * t_tx)))
                img += rot_a * (rot_e * val).sum(axis=0)
    if kw["compound"] == "mean":
        img, B = img / A, B / A
    return img, B


# ---- where the I/Q walk turns a sum -------------------------------------------------------------------------------------------------
def sees(p):
    """[nx, nz]: the pixel's aperture reaches into the span of the line of elements, x + half >= min x_e and x - half <= max x_e with
    half = z / (2 f#) (1e300 without an f-number), in float64 of the float32 tables; NaN elements bound nothing; an element table: every
    pixel"""
    x, z = np.asarray(p["x"], np.float32).astype(np.float64), np.asarray(p["z"], np.float32).astype(np.float64)
    X, Z = np.meshgrid(x, z, indexing="ij")
    if _convex(p):
        return np.ones(X.shape, bool)
    fn = float(np.float32(p["kw"]["f_number"] or 0.0))
    with np.errstate(invalid="ignore"):
        half = Z / (2.0 * fn) if fn > 0 else np.full(X.shape, 1e300)
        ex = np.asarray(p["elem"], np.float32)
        lo, hi = float(np.fmin.reduce(ex, initial=np.float32(3.0e38))), float(np.fmax.reduce(ex, initial=np.float32(-3.0e38)))
        return (X + half >= lo) & (X - half <= hi)


def walked(p):
    """[nx, nz]: the pixels of the 8 x 8 tiles in which some pixel `sees`"""
    s = sees(p)
    out = np.zeros(s.shape, bool)
    for i in range(0, s.shape[0], 8):
        for j in range(0, s.shape[1], 8):
            out[i:i + 8, j:j + 8] = s[i:i + 8, j:j + 8].any()
    return out


@functools.lru_cache(maxsize=None)
def table_sites(name):
    """V6: three pixels in three different tiles, kept by the margins, at which transmission SITE_A of the clean problem takes a term
    and -- linear interpolation, where a NaN entry leaves the receive part alone to index the trace -- some element of the aperture has
    its receive part d fs at least two samples inside the trace.  -> ((ix, iz), ...) in the order NaN, +inf, -inf"""
    g = geometry(name)
    ok = ~g["left_out"] & (g["n_a"][SITE_A] > 0)
    for _, use, _, s_rx in nu._positions(g["tx"], g["elem"], g["x"], g["z"], g["fs"], C0, 0.0, g["kw"]["f_number"]):
        ok &= (use & (s_rx >= 1.0) & (s_rx <= T - 3.0)).any(axis=0)
        break
    sites = []
    for i in range(0, ok.shape[0], 8):
        for j in range(0, ok.shape[1], 8):
            hit = np.argwhere(ok[i:i + 8, j:j + 8])
            if len(hit) and len(sites) < 3:
                sites.append((i + int(hit[len(hit) // 2][0]), j + int(hit[len(hit) // 2][1])))
    return tuple(sites)


# ---- the restatements on a stand-in, made once --------------------------------------------------------------------------------------
def restate(family, p, data, dtype=np.float64, order=0):
    """the float64 (or float32) restatement of a family on a clean problem -> (image, B)"""
    method, pw, window, capon = FAMILIES[family]
    args = (data, p["tx"], p["elem"], p["x"], p["z"], p["fs"], C0)
    if capon is not None:
        return ku.capon(*args, F_D, capon[0], capon[1], dtype=dtype, order=order, **p["kw"])
    if window != "boxcar":
        return au.beamform(method, *args, window, 0.5, p=pw, f_d=F_D, dtype=dtype, **p["kw"])
    if method == "iq":
        return iu.iq_beamform(*args, F_D, dtype=dtype, **p["kw"])
    return nu.beamform(method, *args, p=pw, dtype=dtype, **p["kw"])


@functools.lru_cache(maxsize=None)
def restated(name, family, variant):
    """-> (stand-in problem, ref, B, used, floor): the float64 restatement of the family on the variant's stand-in, the pixels compared
    (kept by the margins, B > 0) and the restatement's own float32 floor there, max |f32 - f64| / B -- for Capon the larger of the two
    orders of its sums (capon_util.floor_of), as in the tests of each family"""
    g = geometry(name)
    p, data = stand_in(variant, g, case_data(name, family))
    ref, B = restate(family, p, data)
    used = ~p["left_out"] & (B > 0)
    orders = (0, 1) if FAMILIES[family][3] is not None else (0,)
    floor = max(float((np.abs(restate(family, p, data, np.float32, o)[0].astype(ref.dtype) - ref)[used] / B[used]).max()) for o in orders)
    for a in (ref, B, used):
        a.setflags(write=False)
    return p, ref, B, used, floor


def bound(family, floor):
    """the bound of the family's own GPU test: 4 x the float32 floor (D19, D20, D23), plus the bound of a weight with a window (D22)"""
    return 4.0 * floor + (au.WEIGHT_BOUND if FAMILIES[family][2] != "boxcar" else 0.0)
