"""AOV TWIN binding -- TEST INFRASTRUCTURE ONLY (see aov_twin.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", _HERE])
        L = C.CDLL(os.path.join(_HERE, "libaovtwin.so"))
        L.aov_twin_last_error.restype = C.c_char_p
        L.aov_twin_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def aov_rows(render_scene, camera, diff_scale, pfilm):
    """aov_twin_rows: pt::aov_item<FEAT_FULL> behind camera_ray and bvh_trace for every p_film row (n x 2) -> (n x 12): albedo,
    coverage, normal, depth, position, the triangle id's bits."""
    desc = render_scene.desc()
    cam = camera.to_abi()
    pf = np.ascontiguousarray(pfilm, dtype=np.float32).reshape(-1, 2)
    out = np.zeros((pf.shape[0], 12), dtype=np.float32)
    rc = lib().aov_twin_rows(C.byref(desc), C.byref(cam), float(diff_scale), pf.shape[0], C.c_void_p(pf.ctypes.data), C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise RuntimeError("aov twin error %d: %s" % (rc, lib().aov_twin_last_error().decode()))
    return out
