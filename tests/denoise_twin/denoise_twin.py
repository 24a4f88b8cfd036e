"""DENOISE TWIN binding -- TEST INFRASTRUCTURE ONLY (see denoise_twin.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
FILM_DTYPE = np.dtype([("rgb", "<f4", 3), ("weight", "<f4")])


class Params(C.Structure):  # PtrsDenoiseParams
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("flags", C.c_uint32)]


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", _HERE])
        L = C.CDLL(os.path.join(_HERE, "libdenoisetwin.so"))
        L.denoise_twin_last_error.restype = C.c_char_p
        L.denoise_twin_run.argtypes = [C.c_int32, C.c_int32, C.c_void_p] + [C.c_void_p] * 5
        _lib = L
    return _lib


def denoise(beauty, planes, iterations=5, sigma_color=0.25, sigma_normal=0.3, sigma_depth=0.1, demodulate=True):
    """denoise_twin_run: pt::dn_prepare / dn_atrous / dn_finish over (H, W) FILM_DTYPE films -- beauty and planes["albedo" | "normal" |
    "depth"] -> the denoised (H, W) FILM_DTYPE film."""
    films = [np.ascontiguousarray(f, dtype=FILM_DTYPE) for f in (beauty, planes["albedo"], planes["normal"], planes["depth"])]
    H, W = films[0].shape
    assert all(f.shape == (H, W) for f in films)
    p = Params(int(iterations), float(sigma_color), float(sigma_normal), float(sigma_depth), 1 if demodulate else 0)
    out = np.zeros((H, W), dtype=FILM_DTYPE)
    rc = lib().denoise_twin_run(W, H, C.byref(p), *[C.c_void_p(f.ctypes.data) for f in films], C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise RuntimeError("denoise twin error %d: %s" % (rc, lib().denoise_twin_last_error().decode()))
    return out
