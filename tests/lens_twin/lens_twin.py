"""LENS TWIN binding -- TEST INFRASTRUCTURE ONLY (see lens_twin.cpp)."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
abi = importlib.import_module("pathtracer-rs_amd.abi")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", _HERE])
        L = C.CDLL(os.path.join(_HERE, "liblenstwin.so"))
        L.lens_twin_rays.argtypes = [C.c_void_p, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.lens_twin_aov_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def _lens_abi(camera):
    cl = abi.PtrsCameraLens()
    camera._fill_abi(cl.camera)
    cl.lens_radius, cl.focal_distance = camera.lens_radius, camera.focal_distance
    return cl


def aov_rows(render_scene, camera, diff_scale, pfilm, ulens):
    """lens_twin_aov_rows: pt::aov_item<FEAT_FULL> behind lens_ray and bvh_trace, handed the generated ray as k_aov hands it, for every
    (p_film, u_lens) row -> (n x 12): albedo, coverage, normal, depth, position, the triangle id's bits."""
    desc = render_scene.desc()
    cl = _lens_abi(camera)
    pf = np.ascontiguousarray(pfilm, dtype=np.float32).reshape(-1, 2)
    ul = np.ascontiguousarray(ulens, dtype=np.float32).reshape(-1, 2)
    assert pf.shape == ul.shape
    out = np.zeros((pf.shape[0], 12), dtype=np.float32)
    rc = lib().lens_twin_aov_rows(C.byref(desc), C.byref(cl), float(diff_scale), pf.shape[0], C.c_void_p(pf.ctypes.data), C.c_void_p(ul.ctypes.data), C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise RuntimeError("lens twin error %d" % rc)
    return out


def lens_rays(camera, diff_scale, pfilm, ulens):
    """lens_twin_rays: pt::lens_ray of the camera's lens for every (p_film, u_lens) row (n x 2 each) -> (n x 12): o, d, rx_d, ry_d."""
    cl = _lens_abi(camera)
    pf = np.ascontiguousarray(pfilm, dtype=np.float32).reshape(-1, 2)
    ul = np.ascontiguousarray(ulens, dtype=np.float32).reshape(-1, 2)
    assert pf.shape == ul.shape
    out = np.zeros((pf.shape[0], 12), dtype=np.float32)
    rc = lib().lens_twin_rays(C.byref(cl), float(diff_scale), pf.shape[0], C.c_void_p(pf.ctypes.data), C.c_void_p(ul.ctypes.data), C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise RuntimeError("lens twin error %d" % rc)
    return out
