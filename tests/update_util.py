"""Scenes as dicts, and one case per traversed parameter, for test_param_updates.py (CPU) and test_gpu_param_updates.py (GPU).

The reference's loop is params = traverse(scene); params[key] = v; params.update(); render again (USMain.py:262-289).  What an
updated scene is held to is a scene BUILT with the value: build(name, overrides) writes the overrides into the dict and calls
load_dict, so the "fresh" scene never sees traverse / update or a cache of the updated one.  ENTRY maps the traversed keys whose
dict entry has another name; every other key "a.b.c" is d["a"]["b"]["c"], through a {"type": "ref"} where there is one.

CASES[name] maps every key traverse() exposes on the scene to its cases (value, consumer):
  "film"    a radiance render reads it: the film after the update differs from the film before
  "acq"     the acquisition reads it: the channel data differ
  "bytes"   it reaches the acquisition's parameter block or the material array, but no statement of the acquisition reads it in this
            scene (a linear array does not read an opening angle, a curved array does not read the pitch, no ray of the integrator
            reaches the deepest plate): what the library is handed differs, the data do not
  "unread"  nothing reads it in this scene (the integrator's opening_angle at radius 0; CustomSensor's element size and sound speed,
            which put_data never reads, CustomSensor.py:29-59)
  "rx"      CustomSensor.put_data reads it
  "raises"  the value cannot be honoured: update() raises ValueError and the scene stays as it was
The values that end in a bit comparison are exact in float32."""
import copy

import numpy as np

import us_util as uu

SEED, SPP = 5, 2
US_E, US_ANGLES, US_T, US_SEED, US_PITCH = 8, (-10.0, 10.0), 4000, 5, 2e-3


class _Capture:
    """stands in for the package where a scene builder of the tests calls load_dict: the dict is edited first"""

    def __init__(self, mi, edit):
        self._mi, self._edit = mi, edit
        self.ScalarTransform4f, self._capi = mi.ScalarTransform4f, mi._capi

    def load_dict(self, d):
        self._edit(d)
        return self._mi.load_dict(d)


def _rgb(r, g=None, b=None):
    return [r, r if g is None else g, r if b is None else b]


def room_dict(mi, glossy=False):
    """the unit room, open towards the camera at z = 3.6: five diffuse walls (floor and ceiling share the BSDF 'white'), a mirror and
    a glass ball, a rectangle light under the ceiling and a point light.  glossy: the mirror has eta / k, and a rough panel hangs on
    the right wall."""
    T = mi.ScalarTransform4f
    diffuse = lambda *c: {"type": "diffuse", "reflectance": {"type": "rgb", "value": _rgb(*c)}}   # noqa: E731
    d = {"type": "scene",
         "integrator": {"type": "path", "max_depth": 4},
         "camera": {"type": "perspective", "fov": 40.0, "fov_axis": "x", "to_world": T().look_at([0, 0, 3.6], [0, 0, 0], [0, 1, 0]),
                    "film": {"type": "hdrfilm", "width": 16, "height": 12, "rfilter": {"type": "tent"}},
                    "sampler": {"type": "independent", "sample_count": SPP}},
         "white": {"type": "diffuse", "id": "white", "reflectance": {"type": "rgb", "value": _rgb(0.75)}},
         "floor": {"type": "rectangle", "to_world": T().translate([0, -1, 0]) @ T().rotate([1, 0, 0], -90), "bsdf": {"type": "ref", "id": "white"}},
         "ceiling": {"type": "rectangle", "to_world": T().translate([0, 1, 0]) @ T().rotate([1, 0, 0], 90), "bsdf": {"type": "ref", "id": "white"}},
         "back": {"type": "rectangle", "to_world": T().translate([0, 0, -1]), "bsdf": diffuse(0.5)},
         "left": {"type": "rectangle", "to_world": T().translate([-1, 0, 0]) @ T().rotate([0, 1, 0], 90), "bsdf": diffuse(0.625, 0.125, 0.125)},
         "right": {"type": "rectangle", "to_world": T().translate([1, 0, 0]) @ T().rotate([0, 1, 0], -90), "bsdf": diffuse(0.125, 0.5, 0.125)},
         "mirror": {"type": "rectangle", "to_world": T().translate([-0.4, 0, -0.9375]) @ T().scale([0.375, 0.5, 1]),
                    "bsdf": {"type": "conductor", "specular_reflectance": {"type": "rgb", "value": _rgb(0.75)}}},
         "ball": {"type": "sphere", "center": [0.5, -0.625, 0.25], "radius": 0.375, "bsdf": {"type": "dielectric", "int_ior": 1.5, "ext_ior": 1.0}},
         "lamp": {"type": "rectangle", "to_world": T().translate([0, 0.96875, 0]) @ T().rotate([1, 0, 0], 90) @ T().scale([0.375, 0.375, 1]),
                  "bsdf": diffuse(0.25), "emitter": {"type": "area", "radiance": {"type": "rgb", "value": _rgb(8.0)}}},
         "bulb": {"type": "point", "position": [0.5, 0.5, 0.5], "intensity": {"type": "rgb", "value": _rgb(2.0)}}}
    if glossy:
        d["mirror"]["bsdf"] = {"type": "conductor", "eta": {"type": "rgb", "value": [0.25, 1.0, 1.5]}, "k": {"type": "rgb", "value": [3.5, 2.5, 2.0]}}
        d["panel"] = {"type": "rectangle", "to_world": T().translate([0.9375, 0.25, 0]) @ T().rotate([0, 1, 0], -90) @ T().scale([0.5, 0.5, 1]),
                      "bsdf": {"type": "roughconductor", "distribution": "ggx", "alpha": 0.25, "eta": {"type": "rgb", "value": [0.5, 0.5, 1.0]},
                               "k": {"type": "rgb", "value": [2.0, 3.0, 2.5]}}}
    return d


# ---- traversed key -> dict entries ---------------------------------------------------------------------------------------------------
ENTRY = {
    "camera.x_fov": lambda v: [(("camera", "fov"), float(v)), (("camera", "fov_axis"), "x")],
    "ball.bsdf.eta": lambda v: [(("ball", "bsdf", "int_ior"), float(v)), (("ball", "bsdf", "ext_ior"), 1.0)],
    "emitter.rays_per_element": lambda v: [(("emitter", "number_of_rays_per_element"), v)],
}


def apply_overrides(d, overrides):
    """write {traversed key: value} into the scene dict d (in place)"""
    for key, v in overrides.items():
        entries = ENTRY[key](v) if key in ENTRY else [(tuple(key.split(".")), v)]
        for path, val in entries:
            node = d
            for name in path[:-1]:
                node = node[name]
                if isinstance(node, dict) and node.get("type") == "ref":   # the shared BSDF: the entry of the object it names
                    node = next(o for o in d.values() if isinstance(o, dict) and o.get("id") == node["id"])
            old = node.get(path[-1])
            if isinstance(old, dict) and old.get("type") == "rgb":
                val = {"type": "rgb", "value": [float(c) for c in np.asarray(val).ravel()]}
            node[path[-1]] = val
    return d


SCENES = ("room", "room_glossy", "phantom", "phantom_plain", "phantom_convex")


def build(mi, name, overrides={}, ppr=1, quirks=None):
    """the scene `name` built with the overrides in its dict.  ppr / quirks: of an ultrasound integrator"""
    if name in ("room", "room_glossy"):
        return mi.load_dict(apply_overrides(room_dict(mi, glossy=name == "room_glossy"), overrides))
    edit = lambda d: apply_overrides(d, overrides)   # noqa: E731
    if name == "phantom":          # emitter rays
        return uu.phantom(_Capture(mi, edit), "few", US_E, US_ANGLES, US_T, ppr, US_SEED, emitter=True, pitch=US_PITCH, quirks=quirks)
    if name == "phantom_plain":    # the integrator's own rays, and a custom_sensor beside the transducer
        def edit_rx(d):
            d["rx"] = {"type": "custom_sensor", "number_of_elements": US_E, "pitch": US_PITCH, "sample_rate": 40e6, "time_samples": 64}
            apply_overrides(d, overrides)
        return uu.phantom(_Capture(mi, edit_rx), "few", US_E, US_ANGLES, US_T, ppr, US_SEED, pitch=US_PITCH, quirks=quirks)
    if name == "phantom_convex":
        from test_gpu_convex_array import _scene
        return _scene(_Capture(mi, edit), max_depth=2, paths_per_ray=ppr, quirks=quirks)
    raise KeyError(name)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _arr(*c):
    return np.array(_rgb(*c), np.float64)


_ROOM_COMMON = {
    "integrator.max_depth": [(2, "film"), (9, "film")],
    "camera.x_fov": [(25.0, "film")],
    "white.reflectance": [(_arr(0.25), "film")],
    "floor.bsdf.reflectance": [(_arr(0.5, 0.25, 0.125), "film")],      # (aliases of white.reflectance)
    "ceiling.bsdf.reflectance": [(_arr(0.375), "film")],
    "back.bsdf.reflectance": [(_arr(0.25, 0.5, 0.75), "film")],
    "left.bsdf.reflectance": [(_arr(0.125, 0.125, 0.625), "film")],
    "right.bsdf.reflectance": [(_arr(0.75), "film")],
    "ball.bsdf.eta": [(1.25, "film")],
    "lamp.bsdf.reflectance": [(_arr(0.875), "film")],
    "lamp.emitter.radiance": [(_arr(16.0), "film"), (_arr(8.0, 2.0, 0.5), "film")],
    "bulb.intensity": [(_arr(4.0), "film")],
    "bulb.position": [(np.array([0.25, 0.5, 0.5]), "film")],
}
# (impedance: under the reference's quirks an interface is entered from the side of `impedance` into the medium of 1.2 (CustomBSDF.py:
# 104-107), and above 1.2 nearly every incidence is a total reflection of amplitude 1 -- a value below 1.2 is one the echoes depend on)
_SHAPES_US = {f"{s}.bsdf.{k}": [(v, "acq")] for s in ("s0", "s1", "p0", "p1", "p2") for k, v in (("impedance", 0.625), ("roughness", 0.4))}
CASES = {
    "room": {**_ROOM_COMMON, "mirror.bsdf.specular_reflectance": [(_arr(0.5, 0.75, 0.25), "film")]},
    "room_glossy": {**_ROOM_COMMON,
                    "mirror.bsdf.eta": [(_arr(1.5, 0.5, 0.25), "film")],
                    "mirror.bsdf.k": [(_arr(1.0, 2.0, 4.0), "film"), (_arr(-1.0), "raises")],
                    "panel.bsdf.alpha": [(0.5, "film"), (0.03125, "film"), (0.0, "raises")],
                    "panel.bsdf.eta": [(_arr(1.5), "film")],
                    "panel.bsdf.k": [(_arr(0.5, 1.0, 4.0), "film")]},
    "phantom": {**_SHAPES_US,
                "integrator.pitch": [(2.5e-3, "acq")],
                "integrator.radius": [(0.04, "raises")],               # the emitter stays a line
                "integrator.opening_angle": [(30.0, "unread")],
                "emitter.number_of_elements": [(US_E - 1, "raises")],  # the integrator keeps its count
                "emitter.pitch": [(2.5e-3, "acq")],
                "emitter.element_width": [(4e-4, "acq")],
                "emitter.element_height": [(2e-3, "acq")],
                "emitter.radius": [(0.04, "raises")],
                "emitter.opening_angle": [(30.0, "bytes")],
                "emitter.steering_angle_min": [(-4.0, "acq")],
                "emitter.steering_angle_max": [(20.0, "acq")],
                "emitter.speed_of_sound": [(1540.0, "acq")],
                "emitter.rays_per_element": [(2, "acq")]},
    "phantom_plain": {**_SHAPES_US,
                      # (the integrator's own rays, unlike the emitter's, never reach the deepest plate: its record changes, no echo does)
                      "p2.bsdf.impedance": [(0.625, "bytes")], "p2.bsdf.roughness": [(0.4, "bytes")],
                      "integrator.pitch": [(2.5e-3, "acq")],
                      "integrator.radius": [(0.04, "raises")],          # an arc of 0 degrees: convex_params refuses it
                      "integrator.opening_angle": [(30.0, "unread")],
                      "rx.number_of_elements": [(US_E + 3, "rx")],
                      "rx.pitch": [(1e-3, "rx")],
                      "rx.element_width": [(1e-4, "unread")],
                      "rx.element_height": [(1e-3, "unread")],
                      "rx.sample_rate": [(20e6, "rx")],
                      "rx.speed_of_sound": [(1500.0, "unread")]},
    "phantom_convex": {"integrator.pitch": [(5e-4, "bytes")],
                       "integrator.radius": [(0.0425, "acq"), (-0.04, "raises")],
                       "integrator.opening_angle": [(30.0, "acq"), (180.0, "raises")],
                       "plate.bsdf.impedance": [(3.0, "acq")],
                       "plate.bsdf.roughness": [(0.4, "acq")]},
}


def cases(name, consumers=None):
    """[(key, value, consumer)] of a scene, for pytest.mark.parametrize"""
    return [(k, v, c) for k, lst in CASES[name].items() for v, c in lst if consumers is None or c in consumers]


def case_id(case):
    key, v, c = case
    return f"{key}={np.asarray(v).ravel().tolist()}".replace(" ", "")


def same_value(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64))


def is_light_key(key):
    return ".emitter." in key or key.startswith("bulb.")


# ---- what a scene hands to the library, as bytes --------------------------------------------------------------------------------------
FLAT = ("prims", "materials", "emitters", "light_prims", "light_cdf", "vertex_normals")


def flat_bytes(sc):
    f = sc.flatten()
    return {k: (None if f[k] is None else (f[k].dtype.str, f[k].shape, f[k].tobytes())) for k in FLAT}


def request_bytes(sc, seed=SEED):
    """the parameter blocks of the scene's requests: camera and film description (radiance), pbrt_us_params (ultrasound)"""
    integ, out = sc.integrator(), {}
    for i, s in enumerate(sc.sensors()):
        if hasattr(s, "camera"):
            out[f"camera{i}"] = bytes(s.camera())
            out[f"film{i}"] = bytes(integ._film_desc(sc, s, seed, 0))
    if hasattr(integ, "us_params"):
        out["us_params"] = bytes(integ.us_params(sc))
    return out


def snapshot(sc):
    return copy.deepcopy((flat_bytes(sc), request_bytes(sc)))


def rx_rays(n=24):
    """rays for CustomSensor.put_data whose (element, bin) pairs are distinct at every pitch / sample rate of the cases: one
    deposit per bin, so the result does not depend on the order of the adds"""
    k = np.arange(n, dtype=np.float32)
    o = np.stack([(k - n / 2) * np.float32(6e-4), np.zeros(n, np.float32), np.zeros(n, np.float32)], axis=1)
    d = np.tile(np.array([[0.0, 0.0, -1.0]], np.float32), (n, 1))
    return dict(o=o, d=d, time=((k + 3) * np.float32(1.1e-7)).astype(np.float32)), (1.0 + k / 8).astype(np.float32)
