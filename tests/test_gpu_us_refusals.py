"""The argument rules of an acquisition as the device entry points keep them (csrc/us_request.h; the whole table is held on the CPU
by tests/test_us_request_host.py): one refusal per rule group through pbrt_us_acquire_dev, each with its code and a message that
names the field, then a valid acquisition on the same context -- a refusal leaves nothing behind -- and the queueing form, which
must not leave an acquisition pending.  Nothing here launches more than the one small valid acquisition: us_plate.xml with 2 angles
x 4 elements x 64 samples (the sampling rate lowered so that the plate's echoes arrive within the 64 samples) at one path per ray."""
import ctypes as C

import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -4
NA, NE, T = 2, 4, 64
UNSUPPORTED_TEXT = "emitter.radius != 0 transmits from an arc: set PBRT_US_ARRAY_CONVEX in pbrt_us_params.primary"


def _scene(mi):
    sc = mi.load_file(scene_path("us_plate.xml"))
    ui = sc.integrator()
    ui.angles, ui.n_angles, ui.n_elements, ui.time_samples, ui.fs = np.asarray([-7.5, 7.5], np.float32), NA, NE, T, 0.8e6
    return sc, ui


def _emitter(p, **kw):
    """a valid CustomEmitter block for the acquisition's elements, then the edits"""
    p.primary = 1                                                    # PBRT_US_PRIMARY_EMITTER
    e = p.emitter
    e.number_of_elements, e.pitch, e.element_width, e.element_height = NE, 1.2e-4, 1e-4, 4e-4
    e.radius, e.opening_angle, e.number_of_rays_per_element, e.speed_of_sound = 0.0, 0.0, 1, 1540.0
    e.steering_angle_min, e.steering_angle_max = -12.0, 12.0
    for k, v in kw.items():
        setattr(e, k, v)


def _convex(p, **kw):
    p.primary |= 0x100                                               # PBRT_US_ARRAY_CONVEX
    p.emitter.number_of_elements, p.emitter.radius, p.emitter.opening_angle = NE, 0.03, 40.0
    for k, v in kw.items():
        setattr(p.emitter, k, v)


# one case per rule group: (name, edit of the valid block, code, what the message holds)
CASES = [
    ("a count of zero", lambda p: setattr(p, "n_angles", 0), E_INVALID, "n_angles"),
    ("too many angles", lambda p: setattr(p, "n_angles", 65), E_INVALID, "n_angles"),
    # 3 x 21845 x 65537 = 2^32 - 1 bins: the first count the 32-bit channel index cannot address
    ("channel index", lambda p: (setattr(p, "n_angles", 3), setattr(p, "n_elements", 21845), setattr(p, "time_samples", 65537)),
     E_INVALID, "time_samples"),
    ("max_depth", lambda p: setattr(p, "max_depth", 0x40000000), E_INVALID, "max_depth"),
    ("sampling rate", lambda p: setattr(p, "fs", 0.0), E_INVALID, "fs"),
    ("sound speed", lambda p: setattr(p, "sound_speed", -1540.0), E_INVALID, "sound_speed"),
    ("primary", lambda p: setattr(p, "primary", 2), E_INVALID, "primary"),
    ("emitter field", lambda p: _emitter(p, element_width=float("nan")), E_INVALID, "element_width"),
    ("emitter elements", lambda p: _emitter(p, number_of_elements=NE + 1), E_INVALID, "number_of_elements"),
    ("array radius", lambda p: _convex(p, radius=0.0), E_INVALID, "radius"),
    ("array opening angle", lambda p: _convex(p, opening_angle=180.0), E_INVALID, "opening_angle"),
    ("array elements", lambda p: _convex(p, number_of_elements=NE - 1), E_INVALID, "number_of_elements"),
    ("arc without the array bit", lambda p: _emitter(p, radius=0.03), E_UNSUPPORTED, UNSUPPORTED_TEXT),
]


def _acquire(lib, handle, p, d, fn="pbrt_us_acquire_dev"):
    """one path per ray, norm_paths = 1: each bin holds at most a few echoes and no scale pass runs"""
    return getattr(lib, fn)(handle, C.byref(p), 7, 1, 0, 1, C.c_void_p(int(d.ptr)), None)


def test_refusals_name_the_field_and_leave_the_context_as_it_was(mi, capi):
    sc, ui = _scene(mi)
    dev = sc.device()
    ctx, lib = dev.ctx, dev.ctx.lib
    # the same acquisition on a context that has seen nothing else
    fresh = mi.Context()
    f = sc.flatten()
    fdev = capi.DeviceScene(fresh, f["prims"], f["materials"], f["emitters"], f["light_prims"], f["light_cdf"], sc.accel, f["vertex_normals"])
    fd = mi.DeviceBuffer(fresh, (NA, NE, T))
    d = mi.DeviceBuffer(ctx, (NA, NE, T))
    try:
        assert _acquire(lib, fdev.handle, ui.us_params(sc), fd) == 0, lib.pbrt_last_error(fresh.handle)
        want = fd.numpy()
        assert want.any()                                           # (the echoes do arrive within the 64 samples)
        for name, edit, code, text in CASES:
            p = ui.us_params(sc)
            edit(p)
            assert _acquire(lib, dev.handle, p, d) == code, name
            msg = lib.pbrt_last_error(ctx.handle).decode()
            if code == E_UNSUPPORTED:
                assert msg == text, name
            else:
                assert msg.startswith("invalid argument: ") and text in msg, (name, msg)
        assert lib.pbrt_us_acquire_dev(dev.handle, None, 7, 1, 0, 1, C.c_void_p(int(d.ptr)), None) == E_INVALID
        assert lib.pbrt_last_error(ctx.handle).decode().startswith("invalid argument: ")
        assert lib.pbrt_us_acquire_dev(dev.handle, C.byref(ui.us_params(sc)), 7, 1, 0, 1, None, None) == E_INVALID
        assert lib.pbrt_last_error(ctx.handle).decode().startswith("invalid argument: ")
        # the context that refused all of these acquires what the fresh one did, bit for bit
        assert _acquire(lib, dev.handle, ui.us_params(sc), d) == 0, lib.pbrt_last_error(ctx.handle)
        assert np.array_equal(d.numpy(), want)
    finally:
        d.close()
        fd.close()
        fdev.close()
        fresh.close()


def test_a_refused_queued_acquisition_is_not_pending(mi):
    sc, ui = _scene(mi)
    dev = sc.device()
    ctx, lib = dev.ctx, dev.ctx.lib
    d = mi.DeviceBuffer(ctx, (NA, NE, T))
    try:
        ctx.synchronize()                                           # (nothing of an earlier test is pending)
        for name, edit, code, text in (CASES[0], CASES[7], CASES[-1]):
            p = ui.us_params(sc)
            edit(p)
            assert _acquire(lib, dev.handle, p, d, "pbrt_us_acquire_queue_dev") == code, name
            assert lib.pbrt_ctx_synchronize(ctx.handle) == 0, name   # no acquisition to finish: nothing waits, nothing fails
        assert _acquire(lib, dev.handle, ui.us_params(sc), d, "pbrt_us_acquire_queue_dev") == 0
        assert lib.pbrt_ctx_synchronize(ctx.handle) == 0
        assert ctx.stats()["samples"] == NA * NE
    finally:
        d.close()
