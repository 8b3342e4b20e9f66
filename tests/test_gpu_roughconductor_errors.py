"""Invalid ROUGHCONDUCTOR / CONDUCTOR_FRESNEL records through the C-ABI: PBRT_E_INVALID from pbrt_scene_create,
pbrt_scene_update_material and the BSDF leaf operators (include/pbrt_hip.h)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAD = [(5, [0.0, 0, 0, 0, 1, 1, 1]), (5, [-0.1, 0, 0, 0, 1, 1, 1]), (5, [np.nan, 0, 0, 0, 1, 1, 1]), (5, [np.inf, 0, 0, 0, 1, 1, 1]),
       (5, [0.1, -1e-3, 0, 0, 1, 1, 1]), (5, [0.1, 0, np.nan, 0, 1, 1, 1]), (5, [0.1, 0, 0, 0, 1, -2.0, 1]),
       (5, [0.1, 0, 0, 0, 1, 1, np.inf]), (6, [0.0, -1.0, 0, 0, 1, 1, 1]), (6, [0.0, 0, 0, 0, np.nan, 1, 1])]
GOOD = [(5, [1e-6, 0, 0, 0, 1, 1, 1]), (5, [0.1, 0.2, 0.9, 1.1, 3.9, 2.4, 2.2]), (6, [0.0, 0, 0, 0, 0, 0, 0]), (6, [-5.0, 1, 1, 1, 2, 2, 2])]


def _scene_parts(mi):
    return mi.load_dict({"type": "scene", "s": {"type": "sphere", "bsdf": {"type": "diffuse"}}}).flatten()


def _create(capi, f, mats):
    return capi.DeviceScene(capi.default_context(), f["prims"], mats, np.zeros(0, dtype=capi.EMITTER_DTYPE), np.zeros(0, np.uint32),
                            np.zeros(0, np.float32))


@pytest.mark.parametrize("t,p", BAD)
def test_invalid_records_are_refused(mi, capi, t, p):
    f = _scene_parts(mi)
    mats = f["materials"].copy()
    mats["type"][0], mats["p"][0] = t, p
    with pytest.raises(RuntimeError, match="rc=-1"):
        _create(capi, f, mats)
    dev = _create(capi, f, f["materials"])
    with pytest.raises(RuntimeError, match="rc=-1"):
        dev.update_material(0, capi.make_material(t, p))
    dev.close()
    cx = capi.default_context()
    m = capi.make_material(t, p)
    wi = capi.f32(np.array([[0.0], [0.0], [1.0]]))
    one, two, out3, out1, lobe = capi.f32(np.zeros(1)), capi.f32(np.zeros((2, 1))), np.empty((3, 1), np.float32), np.empty(1, np.float32), np.empty(1, np.uint32)
    rc = cx.lib.pbrt_bsdf_sample(cx.handle, C.byref(m), 0, 1, capi.addr(wi), None, None, None, capi.addr(one), capi.addr(two),
                                 capi.addr(out3), capi.addr(out1), capi.addr(out3.copy()), capi.addr(lobe))
    assert rc == -1
    rc = cx.lib.pbrt_bsdf_eval_pdf(cx.handle, C.byref(m), 1, capi.addr(wi), capi.addr(wi), capi.addr(out3), capi.addr(out1))
    assert rc == -1


@pytest.mark.parametrize("t,p", GOOD)
def test_valid_records_are_taken(mi, capi, t, p):
    """(an alpha below 1e-3 is valid and used as 1e-3; type 6 does not read p[0])"""
    f = _scene_parts(mi)
    mats = f["materials"].copy()
    mats["type"][0], mats["p"][0] = t, p
    dev = _create(capi, f, mats)
    dev.update_material(0, capi.make_material(t, p))
    dev.close()
