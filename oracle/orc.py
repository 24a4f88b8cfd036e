"""ORACLE -- TEST INFRASTRUCTURE ONLY.  ctypes binding of oracle/liboracle.so (the CPU restatement
of the reference hot path).  Imported only by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg -- never by the product package.  Parity unpinned (see orc_math.h)."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
abi = importlib.import_module("pathtracer-rs_amd.abi")  # the neutral ABI structs (include/ptrs.h)

_lib = None


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE])


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(_HERE, "liboracle.so")
        if not os.path.exists(so):
            build()
        L = C.CDLL(so)
        L.orc_last_error.restype = C.c_char_p
        L.orc_next_float_up.restype = C.c_float
        L.orc_next_float_down.restype = C.c_float
        L.orc_next_float_up.argtypes = [C.c_float]
        L.orc_next_float_down.argtypes = [C.c_float]
        L.orc_detmath.restype = C.c_float
        L.orc_detmath.argtypes = [C.c_int, C.c_float, C.c_float]
        L.orc_log2_int.restype = C.c_uint32
        L.orc_log2_int.argtypes = [C.c_uint64]
        rc = L.orc_load_tables(os.path.join(_ROOT, "data", "sobol_tables.bin").encode())
        if rc != 0:
            raise RuntimeError(L.orc_last_error().decode())
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise RuntimeError("oracle error %d: %s" % (rc, lib().orc_last_error().decode()))


def make_params(width, height, spp, max_depth, row_begin=0, row_end=0, flags=0, paths_per_pass=0, sampler=0, n_sampled_dimensions=0):
    p = abi.PtrsRenderParams()
    p.sampler, p.n_sampled_dimensions = sampler, n_sampled_dimensions
    p.width, p.height, p.spp, p.max_depth = width, height, spp, max_depth
    p.rr_threshold, p.rr_start_depth, p.rr_enable = 1.0, 3, 1  # integrator.rs:240-242
    p.row_begin, p.row_end = row_begin, (row_end if row_end else height)
    p.device, p.paths_per_pass, p.flags = 0, paths_per_pass, flags
    return p


def round_up_pow2(v):
    return 1 << max(0, (int(v) - 1).bit_length())


class OracleScene:
    def __init__(self, render_scene):
        self._rs = render_scene
        self._h = C.c_void_p()
        desc = render_scene.desc()
        _check(lib().orc_scene_create(C.byref(desc), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().orc_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        n, d, t = C.c_uint64(), C.c_uint64(), C.c_uint64()
        lib().orc_scene_info(self._h, C.byref(n), C.byref(d), C.byref(t))
        return dict(bvh_nodes=n.value, bvh_max_depth=d.value, n_tris=t.value)

    def texture_probe(self, tex, rows):
        """orc_texture_probe: rows (n x 6: uv, dudx, dvdx, dudy, dvdy) -> (n x 8), rgb in the layout of csrc/pt_probe.h (diagnostics 0)."""
        rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 6)
        out = np.zeros((rows.shape[0], 8), dtype=np.float32)
        _check(lib().orc_texture_probe(self._h, int(tex), rows.shape[0], C.c_void_p(rows.ctypes.data), C.c_void_p(out.ctypes.data)))
        return out

    def surface_probe(self, prim, rows):
        """orc_surface_probe: rows (n x 16: o, d, t_max, rx_d, ry_d, w) -> (n x 64) in the layout of csrc/pt_probe.h surface_probe_row."""
        rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 16)
        out = np.zeros((rows.shape[0], 64), dtype=np.float32)
        _check(lib().orc_surface_probe(self._h, int(prim), rows.shape[0], C.c_void_p(rows.ctypes.data), C.c_void_p(out.ctypes.data)))
        return out

    def get_bvh(self):
        i = self.info()
        nodes = np.zeros(i["bvh_nodes"], dtype=np.dtype([("p_min", "<f4", 3), ("p_max", "<f4", 3), ("offset", "<u4"), ("num_prims", "<u2"), ("axis", "u1"), ("pad", "u1")]))
        prims = np.zeros(i["n_tris"], dtype=np.uint32)
        _check(lib().orc_scene_get_bvh(self._h, C.c_void_p(nodes.ctypes.data), C.c_void_p(prims.ctypes.data)))
        return nodes, prims

    def render(self, camera, params, n_threads=1, want_samples=False, film=None):
        W, H = params.width, params.height
        if film is None:
            film = np.zeros((H, W), dtype=abi.FILM_DTYPE)
        spp = params.spp if params.sampler == abi.SAMPLER_STRATIFIED else round_up_pow2(params.spp)
        samples = np.zeros(((H + 4), (W + 4), spp, 3), dtype=np.float32) if want_samples else None
        stats = abi.PtrsStats()
        cam = camera.to_abi()
        _check(lib().orc_render(self._h, C.byref(cam), C.byref(params), C.c_void_p(film.ctypes.data),
                                C.c_void_p(samples.ctypes.data) if want_samples else None, int(n_threads), C.byref(stats)))
        return film, samples, stats

    def render_single_pixel(self, camera, params, px, py):
        out = np.zeros((round_up_pow2(params.spp), 3), dtype=np.float32)
        cam = camera.to_abi()
        _check(lib().orc_render_single_pixel(self._h, C.byref(cam), C.byref(params), int(px), int(py), C.c_void_p(out.ctypes.data)))
        return out

    def trace_rays(self, rays, any_hit=False, brute_force=False):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 7)
        hits = np.zeros(rays.shape[0], dtype=abi.HIT_DTYPE)
        stats = abi.PtrsStats()
        _check(lib().orc_trace_rays(self._h, rays.shape[0], C.c_void_p(rays.ctypes.data), int(any_hit), int(brute_force), C.c_void_p(hits.ctypes.data), C.byref(stats)))
        return hits, stats


def stratified_tile(seed, tile_w, tile_h, dim_pixel_samples, n_dims):
    """The StratifiedSampler's tables for a tile seeded `seed`: (tile_w*tile_h pixels in x-major order, [n_dims*spp 1-D | n_dims*spp*2 2-D])."""
    spp = dim_pixel_samples * dim_pixel_samples
    out = np.zeros((tile_w * tile_h, n_dims * spp * 3), dtype=np.float32)
    L = lib()
    L.orc_stratified_tile.argtypes = [C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    _check(L.orc_stratified_tile(int(seed), tile_w, tile_h, dim_pixel_samples, n_dims, C.c_void_p(out.ctypes.data)))
    return out


def pcg64mcg(state, n):
    out = np.zeros(n, dtype=np.uint64)
    L = lib()
    L.orc_pcg64mcg.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]
    L.orc_pcg64mcg.restype = None
    L.orc_pcg64mcg(int(state) & 0xFFFFFFFFFFFFFFFF, int(state) >> 64, n, C.c_void_p(out.ctypes.data))
    return out


def sobol_samples(params, px, py, sample_nums, dims):
    px = np.ascontiguousarray(px, dtype=np.int32)
    py = np.ascontiguousarray(py, dtype=np.int32)
    sn = np.ascontiguousarray(sample_nums, dtype=np.uint64)
    dm = np.ascontiguousarray(dims, dtype=np.uint32)
    out = np.zeros(px.shape[0], dtype=np.float32)
    idx = np.zeros(px.shape[0], dtype=np.uint64)
    _check(lib().orc_sobol_samples(C.byref(params), px.shape[0], C.c_void_p(px.ctypes.data), C.c_void_p(py.ctypes.data), C.c_void_p(sn.ctypes.data),
                                   C.c_void_p(dm.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(idx.ctypes.data)))
    return out, idx


def bsdf_eval(material, tex_values, wo, u):
    m = abi.PtrsMaterial()
    m.kind = material["kind"]
    tx = list(material.get("tex", [])) + [-1] * 6
    m.tex[:] = tx[:6]
    m.flags = material.get("flags", 0)
    m.inner = -1
    tv = np.zeros((6, 3), dtype=np.float32)
    if len(tex_values):
        tv[: len(tex_values)] = np.asarray(tex_values, dtype=np.float32)
    wo = np.ascontiguousarray(wo, dtype=np.float32).reshape(-1, 3)
    u = np.ascontiguousarray(u, dtype=np.float32).reshape(-1, 2)
    out = np.zeros((wo.shape[0], 8), dtype=np.float32)
    _check(lib().orc_bsdf_eval(C.byref(m), C.c_void_p(tv.ctypes.data), wo.shape[0], C.c_void_p(wo.ctypes.data), C.c_void_p(u.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out


def bsdf_probe(material, tex_values, frame, rows):
    """orc_bsdf_probe: rows (n x 8: wo, wi, u) at a hit with frame (ng, ns, dpdu) -> (n x 16) in the layout of csrc/pt_probe.h."""
    m = abi.PtrsMaterial()
    m.kind = material["kind"]
    tx = list(material.get("tex", [])) + [-1] * 6
    m.tex[:] = tx[:6]
    m.flags = material.get("flags", 0)
    m.inner = -1
    tv = np.zeros((6, 3), dtype=np.float32)
    if len(tex_values):
        tv[: len(tex_values)] = np.asarray(tex_values, dtype=np.float32)
    fr = np.ascontiguousarray(frame, dtype=np.float32).reshape(9)
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 8)
    out = np.zeros((rows.shape[0], 16), dtype=np.float32)
    _check(lib().orc_bsdf_probe(C.byref(m), C.c_void_p(tv.ctypes.data), C.c_void_p(fr.ctypes.data), rows.shape[0], C.c_void_p(rows.ctypes.data),
                                C.c_void_p(out.ctypes.data)))
    return out


def filter_table():
    t = np.zeros(256, dtype=np.float32)
    lib().orc_filter_table(C.c_void_p(t.ctypes.data))
    return t.reshape(16, 16)
