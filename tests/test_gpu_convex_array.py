"""The convex (curved) array of DESIGN.md D18 on the device: acquisition (PBRT_US_ARRAY_CONVEX: arc origins, receive connection and
receive directivity against the element's own normal), both kernel families, emitter primaries, the large-radius limit, the
delay-and-sum on an element table, and us_render end to end.  The CPU oracle does not know the array: the reference is the float64
restatement of tests/convex_util.py.

Common acquisition: 3 angles (-8, 0, 8 degrees), 16 elements on R = 40 mm over 40 degrees, c = 1540 m/s, fs = 50 MHz, 2048 samples,
256 paths per ray, a steel plate 20 mm beyond the apex tilted 5 degrees about y (DESIGN D12 forbids exact normal incidence).  The
sensor transform moves the apex to the world's origin."""
import ctypes as C

import numpy as np
import pytest

import convex_util as cu
import das_util as du

pytestmark = pytest.mark.gpu

R, OPEN, N, C0, FS, TS, PPR = 0.04, 40.0, 16, 1540.0, 50e6, 2048, 256
ANGLES = (-8.0, 0.0, 8.0)
AM, AC = 10.0, 25.0
DEPTH, TILT = 0.02, 5.0


def _bsdf():
    return {"type": "ultrasound_bsdf", "impedance": 7.8, "roughness": 0.8}


def _plate_matrix(mi, depth=DEPTH, tilt=TILT, half=0.06):
    T = mi.ScalarTransform4f
    return np.asarray((T().translate([0, 0, depth]) @ T().rotate([0, 1, 0], tilt) @ T().rotate([1, 0, 0], 180) @ T().scale([half, half, 1])).matrix,
                      np.float64)


def _plate_of(M):
    """(p0, e1, e2) of the `rectangle` [-1, 1]^2 under the 4 x 4 matrix M"""
    M = np.asarray(M, np.float64)
    p = lambda x, y: M[:3, :3] @ np.array([x, y, 0.0]) + M[:3, 3]   # noqa: E731
    return p(-1, -1), p(1, -1) - p(-1, -1), p(-1, 1) - p(-1, -1)


def _scene(mi, plate=None, radius=R, opening=OPEN, apex_z=0.0, emitter=None, max_depth=1, quirks=None, shape=None, **integ):
    T = mi.ScalarTransform4f
    d = {"type": "scene",
         "integrator": {"type": "ultrasound_integrator", "max_depth": max_depth, "sampling_rate": FS, "frequency": 5e6, "sound_speed": C0,
                        "attenuation": 0.5, "main_beam_angle": AM, "cutoff_angle": AC, "n_elements": N, "pitch": 3e-4, "time_samples": TS,
                        "angles": np.asarray(ANGLES, np.float32), "paths_per_ray": PPR, "seed": 3, "radius": radius, "opening_angle": opening,
                        **({} if quirks is None else {"quirks": quirks}), **integ},
         # the centre of curvature sits `radius` behind the apex, the apex at (0, 0, apex_z) of the world
         "sensor": {"type": "ultrasound_sensor", "to_world": T().translate([0, 0, apex_z - radius])}}
    if emitter is not None:
        d["emitter"] = {"type": "ultrasound_emitter", "number_of_elements": N, "pitch": 3e-4, "element_width": 0.0, "element_height": 0.0,
                        "number_of_rays_per_element": 1, "speed_of_sound": C0, "radius": radius, "opening_angle": opening, **emitter}
        d["integrator"]["primary_rays"] = "emitter"
    d["plate"] = shape if shape is not None else {"type": "rectangle", "to_world": T(_plate_matrix(mi) if plate is None else plate),
                                                  "bsdf": _bsdf()}
    return mi.load_dict(d)


def _model(sc, plate, **kw):
    ui = sc.integrator()
    p = ui.us_params(sc)
    elem = cu.element_table(N, float(np.float32(ui.radius)), float(np.float32(ui.opening_angle)))
    return cu.echo_model(np.asarray(list(p.sensor_to_world), np.float64), elem, float(np.float32(ui.radius)), ANGLES, C0, FS, AM, AC, plate, **kw)


def _check_words(buf, model, label):
    sure, unsure, share = cu.predicted_words(model, TS)
    got = cu.words_of(buf)
    print(f"\n{label}: {len(sure)} predicted words, {len(got)} found, {len(unsure)} candidate words of pairs left out ({share:.2%} of the pairs)")
    assert share <= 0.02
    assert model["hit"].all() and len(sure) > 300
    missing, extra = sure - got - unsure, got - sure - unsure
    assert not missing and not extra, (sorted(missing)[:5], sorted(extra)[:5])


def test_arrival_bins_closed_form(mi):
    """One bounce, the integrator's own rays started on the arc: the non-zero words of the channel buffer are the words the float64
    model predicts -- first hit of the arc-origin ray, bin rint((tx + t_hit + |p - target| / c) fs), kept where the directivity factor
    against the RECEIVE ELEMENT'S normal is non-zero.  Pairs within 1e-3 samples of a rounding tie or within 1e-4 rad of the cut-off
    are left out: 0.26 % of the 768 pairs at this depth and tilt.  With a main beam of
    10 and a cut-off of 25 degrees the model with the array axis as the normal predicts another set (asserted below), so a kernel that
    uses the transducer normal fails."""
    sc = _scene(mi)
    plate = _plate_of(_plate_matrix(mi))
    model = _model(sc, plate)
    wrong = _model(sc, plate, axis_normal=True)
    cut_by_normal_only = (model["D"] == 0) & (wrong["D"] != 0)
    kept_by_normal_only = (model["D"] != 0) & (wrong["D"] == 0)
    assert cut_by_normal_only.sum() > 20 and kept_by_normal_only.sum() > 0       # (111 and 11 of the 768 pairs)
    sure_w, unsure_w, _ = cu.predicted_words(wrong, TS)
    ui = sc.integrator()
    buf = ui._acquire(sc, ui.quirks)
    assert buf.shape == (len(ANGLES), N, TS) and np.isfinite(buf).all()
    want_tx = cu.tx_delays(cu.element_table(N, R, OPEN), R, ANGLES, C0)
    assert np.abs(ui.transmission_delays_buf.reshape(len(ANGLES), N) - want_tx).max() <= 16 * 2.0 ** -24 * R / C0
    _check_words(buf, model, "element rays")
    got = cu.words_of(buf)
    assert (sure_w - got - unsure_w) or (got - sure_w - unsure_w)      # ... and they are NOT the words of the array-axis model


def _snapped_plate():
    """the plate of the common acquisition on a lattice of 2^-20 m, so that a 4 x 4 mesh of it consists of exact float32
    parallelograms (the loader merges such triangle pairs into quads whose first edge -- the shading frame's tangent -- is the
    rectangle's): tilt 5 degrees to within 2^-20 m over a 15.6 mm cell (< 0.01 degrees), centre (0, 0, 20 mm - 90 lattice steps) =
    19.914 mm.  The depth is the lattice point near 20 mm at which the float64 model keeps every first-bounce arrival furthest from
    a rounding tie, for the integrator's rays and for emitter rays steered to 6 degrees alike (2.6e-3 samples and more, 768 pairs
    each; at 20 mm itself two pairs lie within 1e-3): the two kernel families find the hit with different intersection routines, and
    a pair on a tie could land in either bin."""
    q = 2.0 ** -20
    cell = 2.0 ** -6
    th = np.deg2rad(TILT)
    U = np.round(np.array([np.cos(th), 0.0, -np.sin(th)]) * cell / q) * q
    V = np.array([0.0, -cell, 0.0])
    c = np.array([0.0, 0.0, (np.round(DEPTH / q) - 90) * q])
    p0 = c - 2 * U - 2 * V
    return p0, U, V


def _write_plate_obj(path, p0, U, V, n=4):
    idx = lambda i, j: j * (n + 1) + i + 1   # noqa: E731
    with open(path, "w") as f:
        for j in range(n + 1):
            for i in range(n + 1):
                v = p0 + i * U + j * V
                f.write(f"v {v[0]:.17g} {v[1]:.17g} {v[2]:.17g}\n")
        for j in range(n):
            for i in range(n):
                a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
                f.write(f"f {a} {b} {c}\nf {a} {c} {d}\n")


@pytest.mark.parametrize("tables,emitter", [(True, False), (False, False), (False, True)], ids=["tables", "no-tables", "emitter"])
def test_kernel_families_agree(mi, capi, tmp_path, tables, emitter):
    """The same plate as one parallelogram (brute force: k_us_bounce<.., CONVEX>) and as a mesh of 32 triangles through the BVH streams
    (k_us_init_wf<CONVEX> / k_us_first<.., CONVEX>, k_trace, k_us_shade<.., CONVEX>), four bounces: DESIGN section 3's ultrasound
    tolerance on the whole buffer, rel. L2 <= 1e-3 and the same non-zero words.  With the first-bounce tables and without; with
    emitter primaries as well (they never have tables; point elements steered to 6 degrees).  The plate's depth keeps every arrival
    away from a rounding tie (_snapped_plate; asserted)."""
    p0, U, V = _snapped_plate()
    n = np.cross(U, V)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = 2 * U, 2 * V, n / np.linalg.norm(n), p0 + 2 * U + 2 * V
    _write_plate_obj(str(tmp_path / "plate.obj"), p0, U, V)
    q = capi.USQ_REFERENCE | (0 if tables else capi.USQ_NO_FIRST_TABLES)
    em = {"steering_angle_min": 6.0, "steering_angle_max": 6.0} if emitter else None
    brute = _scene(mi, plate=M, max_depth=4, quirks=q, emitter=em)
    brute.accel = capi.ACCEL_BRUTE
    mesh = _scene(mi, max_depth=4, quirks=q, emitter=em, shape={"type": "obj", "filename": str(tmp_path / "plate.obj"), "bsdf": _bsdf()})
    mesh.accel = capi.ACCEL_BVH
    P = mesh.flatten()["prims"]
    assert len(P) == 16 and (P["type"] == capi.PRIM_PARALLELOGRAM).all()
    a = brute.integrator()._acquire(brute, q)
    st_a = mi.default_context().stats()
    b = mesh.integrator()._acquire(mesh, q)
    st_b = mi.default_context().stats()
    assert st_a["segments"] == st_b["segments"] > 0 and st_a["samples"] == st_b["samples"] == len(ANGLES) * N * PPR
    model = _model(brute, (p0, 4 * U, 4 * V), emitter_psi_deg=6.0 if emitter else None)
    assert not cu.predicted_words(model, TS)[1] and np.nanmin(np.abs(model["s"] - np.floor(model["s"]) - 0.5)) > 2.5e-3
    rel = float(np.linalg.norm(a - b) / np.linalg.norm(a))
    differ = int(((a != 0) != (b != 0)).sum())
    print(f"\ntables={tables} emitter={emitter}: rel. L2 {rel:.3g}, {differ} words differ in being non-zero, {int((a != 0).sum())} non-zero")
    assert (a != 0).sum() > 300
    assert np.array_equal(a != 0, b != 0) and rel <= 1e-3


def test_large_radius_limit(mi, capi):
    """R = 10 m, the apex moved onto the linear array's plane by the sensor transform, the opening angle giving the linear pitch along
    the arc, echoes as plain amplitudes (PBRT_USQ_NO_CARRIER): the channel buffer against the linear acquisition of the same scene.
    What separates them: the sagitta of the arc, R (1 - cos(span / 2)) = 2.5e-7 m -- below the float32 grid 10 m from the sensor's
    origin, so the table's z_e is exactly R and the elements lie on the line; x_e = R sin(th_e) against pitch (e - 7.5), 2e-10 m; and
    the tilt of the outer elements' normals, 2.2e-4 rad, which moves the directivity factor of the pairs on its ramp (15 degrees
    wide) by up to 1e-3 of the full weight.  The float64 model (convex_util.echo_model on the float32-rounded tables: directivity
    factor into the bin of every pair) predicts rel. L2 2.6e-4 and no pair in another bin (arrivals move by < 1e-5 samples); four
    times the prediction is allowed.  Both figures are printed."""
    Rl, pitch = 10.0, 3e-4
    opening = float(np.rad2deg((N - 1) * pitch / Rl))
    q = capi.USQ_REFERENCE | capi.USQ_NO_CARRIER
    plate = _plate_of(_plate_matrix(mi))
    conv = _scene(mi, radius=Rl, opening=opening, quirks=q)
    lin = _scene(mi, radius=0.0, opening=0.0, quirks=q)
    assert lin.integrator().us_params(lin).primary == capi.US_PRIMARY_ELEMENT
    # the model's two buffers: directivity factor into the bin of every pair
    pc = conv.integrator().us_params(conv)
    e_conv = cu.element_table(N, Rl, np.float32(opening)).astype(np.float32).astype(np.float64)
    x_lin = (np.float64(np.float32(pitch)) * (np.arange(N) - (N - 1) / 2)).astype(np.float32).astype(np.float64)
    e_lin = np.stack([x_lin, np.zeros(N), np.zeros(N), np.ones(N)], axis=1)
    m_conv = cu.echo_model(np.asarray(list(pc.sensor_to_world), np.float64), e_conv, Rl, ANGLES, C0, FS, AM, AC, plate)
    m_lin = cu.echo_model(np.asarray(list(lin.integrator().us_params(lin).sensor_to_world), np.float64), e_lin, 0.0, ANGLES, C0, FS, AM, AC, plate)

    def image(m):
        img = np.zeros((len(ANGLES), N, TS))
        for a, e, r in np.argwhere(m["D"] != 0):
            img[a, r, int(np.rint(m["s"][a, e, r]))] += m["D"][a, e, r]
        return img

    i_conv, i_lin = image(m_conv), image(m_lin)
    predicted = float(np.linalg.norm(i_conv - i_lin) / np.linalg.norm(i_lin))
    a = conv.integrator()._acquire(conv, q)
    b = lin.integrator()._acquire(lin, q)
    measured = float(np.linalg.norm(a - b) / np.linalg.norm(b))
    print(f"\nlarge radius: model predicts rel. L2 {predicted:.3g}, measured {measured:.3g}; "
          f"{int(((a != 0) != (b != 0)).sum())} of {int((b != 0).sum())} words differ in being non-zero")
    assert 0 < predicted < 0.5 and (b != 0).sum() > 300
    assert measured <= 4 * predicted


def test_emitter_primaries_on_the_arc(mi, capi):
    """PBRT_US_PRIMARY_EMITTER | PBRT_US_ARRAY_CONVEX without jitter (point elements, steering_angle_min == max = 6 degrees): every path
    of element e is the ray from (x_e, 0, z_e) along (sin psi, 0, cos psi) with the emitter's own emission time -(x_e sin psi) / c
    (CustomEmmitter.py:93; the tx table is not added), whatever the angle index -- the words of test_arrival_bins_closed_form's model
    under that delay convention."""
    psi = 6.0
    sc = _scene(mi, emitter={"steering_angle_min": psi, "steering_angle_max": psi})
    ui = sc.integrator()
    assert ui.us_params(sc).primary == (capi.US_PRIMARY_EMITTER | capi.US_ARRAY_CONVEX)
    buf = ui._acquire(sc, ui.quirks)
    assert np.isfinite(buf).all()
    _check_words(buf, _model(sc, _plate_of(_plate_matrix(mi)), emitter_psi_deg=psi), "emitter rays")
    assert np.array_equal(buf[0] != 0, buf[1] != 0) and np.array_equal(buf[0] != 0, buf[2] != 0)


@pytest.mark.parametrize("n,radius,opening", [(16, R, OPEN), (70, 0.06, 89.0), (1, R, OPEN)])
def test_emitter_origins_are_the_table(mi, capi, n, radius, opening):
    """D18: transmit and receive positions of an element are the same floats -- the origins CustomEmitter.sample_ray gives without
    jitter on the device (k_us_emitter_sample_ray) against the host's table (pbrt_us_array_elements), bit for bit, up to the 45
    degrees of half span that the shared polynomial covers."""
    em = mi.load_dict({"type": "ultrasound_emitter", "number_of_elements": n, "element_width": 0.0, "element_height": 0.0,
                       "radius": radius, "opening_angle": opening, "steering_angle_min": 0.0, "steering_angle_max": 0.0})
    s1 = ((np.arange(n) + 0.5) / n).astype(np.float32)
    ray, _ = em.sample_ray(np.zeros(n, np.float32), s1, np.full((n, 2), 0.5, np.float32), np.zeros(n, np.float32))
    from importlib import import_module
    bf = import_module(mi.__name__ + ".beamform")
    table = bf.array_elements(bf.convex_params(n, radius, opening))
    o = np.asarray(ray["o"], np.float32)
    assert np.array_equal(o[:, 0], table[:, 0]) and np.array_equal(o[:, 2], table[:, 1]) and not o[:, 1].any()


def test_setup_refusals(mi, capi):
    """What pbrt_us_acquire refuses before anything is launched: the hole (emitter on an arc, no PBRT_US_ARRAY_CONVEX) is
    PBRT_E_UNSUPPORTED (-4), a bad array PBRT_E_INVALID (-1)."""
    sc = _scene(mi, emitter={"steering_angle_min": 0.0, "steering_angle_max": 0.0})
    ui, dev = sc.integrator(), sc.device()
    buf = np.zeros((len(ANGLES), N, TS), np.float32)

    def rc_of(edit):
        p = ui.us_params(sc)
        edit(p)
        rc = dev.ctx.lib.pbrt_us_acquire(dev.handle, C.byref(p), 1, 4, 0, 4, capi.addr(buf), None)
        return rc, (dev.ctx.lib.pbrt_last_error(dev.ctx.handle) or b"").decode()

    def drop_bit(p):
        p.primary = capi.US_PRIMARY_EMITTER

    rc, msg = rc_of(drop_bit)
    assert rc == -4 and "PBRT_US_ARRAY_CONVEX" in msg

    def setter(**kw):
        def edit(p):
            for k, v in kw.items():
                setattr(p.emitter, k, v)
        return edit

    for kw in (dict(number_of_elements=N - 1), dict(radius=0.0), dict(radius=-R), dict(radius=float("inf")), dict(opening_angle=180.0),
               dict(opening_angle=0.0), dict(opening_angle=float("nan"))):
        for primary in (capi.US_PRIMARY_EMITTER, capi.US_PRIMARY_ELEMENT):
            def edit(p, kw=kw, primary=primary):
                setter(**kw)(p)
                p.primary = primary | capi.US_ARRAY_CONVEX
            assert rc_of(edit)[0] == -1, (kw, primary)
    assert rc_of(lambda p: setattr(p, "primary", 2 | capi.US_ARRAY_CONVEX))[0] == -1
    assert not buf.any()                                        # nothing ran


def _das_case(seed, A, E):
    """random traces on a 24 x 40 grid (no multiple of the 8 x 8 tile) in front of an E-element arc of R = 40 mm over 60 degrees; z is
    measured from the centre of curvature, the grid starts 1 mm beyond the apex and reaches past both ends of the array"""
    rng = np.random.default_rng(seed)
    T = 1500
    elem = cu.element_table(E, R, 60.0).astype(np.float32)
    ang = np.linspace(-10.0, 10.0, A)
    tx = cu.tx_delays(elem.astype(np.float64), R, ang, C0).astype(np.float32)
    x = np.linspace(-0.03, 0.03, 24).astype(np.float32)
    z = np.linspace(R + 1e-3, R + 0.03, 40).astype(np.float32)
    longest = 2 * np.hypot(0.05, 0.03) / C0 + float(np.abs(tx).max())
    fs = 1.3 * (T - 1) / longest
    data = rng.normal(size=(A, E, T)).astype(np.float32)
    return data, tx, elem, x, z, fs


@pytest.mark.parametrize("interp", ["nearest", "linear"])
@pytest.mark.parametrize("fnum", [0.0, 1.0])
@pytest.mark.parametrize("A", [3, 7])
@pytest.mark.parametrize("E", [16, 70])
def test_das_on_the_element_table_against_float64(mi, E, A, fnum, interp):
    """pbrt_das_beamform_probe, its _dev form and the table form (first arrival made once) on seeded random traces: bit-equal to one
    another, and every pixel within the tolerance tests/test_gpu_das_shapes.py holds the linear kernel to -- (n_terms + 16) 2^-24 x the
    sum of the terms' sizes -- of the float64 restatement (convex_util.das: distances to (x_e, z_e), the aperture 2 f# |d_t| <= d_n in
    the element's frame).  E = 70 crosses the 64-element block, A = 7 the five angles of a trip."""
    data, tx, elem, x, z, fs = _das_case(100 * E + 10 * A, A, E)
    kw = dict(t0=0.0, f_number=fnum, interpolation=interp, compound="sum")
    cx = mi.default_context()
    d_x, d_z = mi.DeviceBuffer.from_host(cx, x), mi.DeviceBuffer.from_host(cx, z)
    d_data = mi.DeviceBuffer.from_host(cx, data)
    host = mi.das_beamform(data, tx, elem, x, z, fs, C0, **kw)
    dev = mi.das_beamform(d_data, tx, elem, d_x, d_z, fs, C0, out=mi.DeviceBuffer.from_host(cx, np.full((24, 40), np.nan, np.float32)), **kw).numpy()
    tab = mi.das_first_arrival(tx, elem, d_x, d_z, C0)
    tabled = mi.das_beamform(d_data, tx, elem, d_x, d_z, fs, C0, table=tab, **kw).numpy()
    assert np.array_equal(dev, tabled) and np.array_equal(host, dev) and not np.isnan(dev).any()
    # the first-arrival table against float64 (the bound of test_gpu_das_shapes.py)
    e64 = du.f64(elem)
    X, Z = np.meshgrid(du.f64(x), du.f64(z), indexing="ij")
    dist = np.sqrt((X[None] - e64[:, 0, None, None]) ** 2 + (Z[None] - e64[:, 1, None, None]) ** 2)
    t_ref = np.stack([np.min(du.f64(tx)[a][:, None, None] + dist / float(np.float32(C0)), axis=0) for a in range(A)])
    assert (np.abs(tab.numpy() - t_ref) <= 1e-15 * (np.abs(t_ref) + np.abs(du.f64(tx)).max())).all()
    ref, n_terms, excluded, ties = cu.das(data, tx, elem, x, z, fs, C0, **kw)
    tol, _ = cu.das_tolerance(data, tx, elem, x, z, fs, C0, **kw)
    keep = ~excluded & ~ties
    assert keep.mean() > 0.97 and n_terms.max() > 0
    if fnum > 0:
        assert (n_terms < A * E).any() and (n_terms == 0).any()     # the aperture cuts, and some pixels see no element
    err = np.abs(dev.astype(np.float64) - ref)
    over = keep & (err > tol)
    assert not over.any(), (np.argwhere(over)[:5].tolist(), err[over][:5], tol[over][:5])
    assert (dev[keep & (n_terms == 0)] == 0).all()
    live = keep & (n_terms > 0)
    print(f"\nE={E} A={A} f#={fnum} {interp}: with terms {int(live.sum())}, excluded {int((~keep).sum())}, "
          f"max err / tol {float((err[live] / tol[live]).max()):.3g}")


def test_bmode_end_to_end(mi):
    """us_render with the curved array on the plate: the envelope of the central column peaks within one wavelength of the plate's
    depth below the apex (z is measured from the centre of curvature: R + 20 mm), and the third call replays its recording with the
    same image (at the tolerance of f32 atomics, as tests/test_gpu_beamform.py holds the linear chain)."""
    sc = _scene(mi, max_depth=2)
    ui = sc.integrator()
    lam = C0 / ui.frequency
    kw = dict(x_range=(-0.01, 0.01), z_range=(R + 0.005, R + 0.03))
    imgs, flags = [], []
    for _ in range(3):
        tm = {}
        disp, bmode, (xs, zs) = mi.us_render(sc, timing=tm, **kw)
        imgs.append(bmode)
        flags.append(tm["replayed"])
    assert flags == [False, False, True]
    assert imgs[0].shape == (len(xs), len(zs)) and np.isfinite(imgs[0]).all() and disp.min() >= 0 and disp.max() <= 1
    assert ui.transmission_delays_buf.shape == (len(ANGLES) * N,)
    ix = int(np.argmin(np.abs(xs)))
    z_peak = zs[int(np.argmax(imgs[0][ix]))]
    # the plate passes through (0, 0, 20 mm) of the world = (0, 0, R + 20 mm) of the sensor's frame, tilted: at x = xs[ix] it lies at
    z_plate = R + DEPTH - np.tan(np.deg2rad(TILT)) * xs[ix]
    print(f"\nB-mode: envelope peak of column x = {xs[ix]:.2e} at z = {z_peak:.5f}, plate at {z_plate:.5f} (lambda {lam:.2e})")
    assert abs(z_peak - z_plate) <= lam
    assert np.allclose(imgs[2], imgs[1], rtol=0, atol=2e-5 * imgs[1].max()) and np.allclose(imgs[2], imgs[0], rtol=0, atol=2e-5 * imgs[0].max())
    plain = mi.us_render(sc, graph=False, **kw)[1]
    assert np.allclose(imgs[2], plain, rtol=0, atol=2e-5 * plain.max())
