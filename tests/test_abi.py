"""The C-ABI shared library: loads, exports every symbol include/ptrs.h declares, agrees with the
ctypes mirror on struct sizes, and fails loudly (never silently falls back) without a GPU."""
import ctypes as C
import os
import re

import pytest

from conftest import CORNELL, ROOT


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "ptrs.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ptrs_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(ptrs):
    L = ptrs.load_library()
    names = _declared_functions()
    assert len(names) >= 12
    for n in names:
        assert hasattr(L, n), n
    assert L.ptrs_abi_version() == 4


def test_struct_sizes_match_binding(ptrs):
    L = ptrs.load_library()
    a = ptrs.abi
    for i, s in enumerate([a.PtrsTexture, a.PtrsMaterial, a.PtrsMesh, a.PtrsLight, a.PtrsBvhNode, a.PtrsSceneDesc, a.PtrsCamera, a.PtrsRenderParams, a.PtrsStats, a.PtrsHit]):
        assert L.ptrs_abi_sizeof(i) == C.sizeof(s), s.__name__
    assert L.ptrs_abi_sizeof(10) == 16 and a.FILM_DTYPE.itemsize == 16 and a.HIT_DTYPE.itemsize == 20


def test_no_cpu_fallback(ptrs):
    """Without a GPU the product path must raise (this container has none).  On a GPU box the same
    call succeeds, which the -m gpu tests cover."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cam, scene = ptrs.import_scene(CORNELL, (8, 8))
    integ = ptrs.PathIntegrator(ptrs.SamplerBuilder(1, cam.film.get_sample_bounds()), 2)
    with pytest.raises(Exception) as e:
        integ.render(cam, scene)
    assert "no HIP device" in str(e.value)


def test_sampler_builder_mirror(ptrs):
    """SobolSamplerBuilder::new (sobol.rs:35-60): spp rounded up to a power of two (Q4),
    resolution = round_up_pow2(max extent), log2."""
    with pytest.warns(UserWarning):
        sb = ptrs.SamplerBuilder(100, (-2, -2, 1026, 1026))
    assert (sb.samples_per_pixel, sb.resolution, sb.log_2_resolution) == (128, 2048, 11)
    sb = ptrs.SamplerBuilder(16, (-2, -2, 258, 258))
    assert (sb.samples_per_pixel, sb.resolution, sb.log_2_resolution) == (16, 512, 9)


def test_options_api():
    """ptrs_set_option / ptrs_get_option: known names round-trip, ranges are enforced, unknown names are errors -- no GPU needed.
    (The library reads no environment variables; these knobs replace the getenv switches of round 1.)"""
    import importlib
    ptrs = importlib.import_module("pathtracer-rs_amd")
    L = ptrs.load_library()
    defaults = {"lanes": 0, "grid_pct": 0, "refill": -1, "refill_connect": -1, "vote": -1, "shade_lds": 1, "fused_epilogue": 1, "fused_resolve": 1, "stack_lds": 8, "grid_mult": 0, "persist": 1, "whole_rounds": 0, "node_order": 0, "peer_copy": 1, "env_presample": 1, "node_form": 0, "workspace_pct": 40, "tail": 1, "tail_at": -1, "tail_paths": 0, "deal": 0, "segments": 0}
    for k, v in defaults.items():
        assert ptrs.get_option(k) == v, k
    with ptrs.options(lanes=1, vote=0):
        assert ptrs.get_option("lanes") == 1 and ptrs.get_option("vote") == 0
    assert ptrs.get_option("lanes") == 0 and ptrs.get_option("vote") == -1
    with ptrs.options(segments=1 << 20):  # (the test hook that caps a pass's queue segments: 0 .. 2^20)
        assert ptrs.get_option("segments") == 1 << 20
    assert ptrs.get_option("segments") == 0
    for name, bad in (("lanes", -1), ("lanes", 9), ("workspace_pct", 0), ("vote", 3), ("no_such_option", 1), ("segments", -1), ("segments", (1 << 20) + 1)):
        assert L.ptrs_set_option(name.encode(), bad) != 0
        assert L.ptrs_last_error()
    import ctypes as C
    assert L.ptrs_get_option(b"no_such_option", C.byref(C.c_int64())) != 0


def test_new_entry_points_check_their_arguments(ptrs):
    """ABI 4's additions refuse bad arguments before they touch a device (no GPU needed): the band planner's probe, the division
    self-test, and the build id is the hash of this tree's kernel sources and flags."""
    import importlib
    L = ptrs.load_library()
    assert L.ptrs_render_row_cost(None, None, None, None, None) != 0 and b"null" in L.ptrs_last_error()
    bad = C.c_uint64(0)
    L.ptrs_selftest_div3.argtypes = [C.c_int32, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]
    assert L.ptrs_selftest_div3(0, 9, 1, 1, C.byref(bad), None, None) != 0   # no such mode
    assert L.ptrs_selftest_div3(0, 0, 0, 1, C.byref(bad), None, None) != 0   # nothing to test
    assert L.ptrs_selftest_div3(0, 0, 1, 1, None, None, None) != 0           # nowhere to put the answer
    assert ptrs.build_id() == importlib.import_module("pathtracer-rs_amd.build").source_hash()
    assert len(ptrs.build_id()) == 16


def test_probe_entry_points_check_their_arguments(ptrs):
    """ptrs_probe_bsdf / ptrs_probe_light (known-answer probes of csrc/pt_probe.h) refuse a missing scene, frame / reference point
    or row buffers before they touch a device (no GPU needed)."""
    L = ptrs.load_library()
    L.ptrs_probe_bsdf.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.ptrs_probe_light.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    buf = (C.c_float * 64)()
    for fn in (L.ptrs_probe_bsdf, L.ptrs_probe_light):
        assert fn(None, 0, buf, 1, buf, buf) != 0 and b"null" in L.ptrs_last_error()     # no scene
        assert fn(None, 0, None, 0, None, None) != 0 and b"null" in L.ptrs_last_error()   # no frame / reference point
    import numpy as np
    import twin
    scene = ptrs.RenderScene()
    m = scene.add_material(ptrs.abi.MAT_MATTE, [scene.const_rgb([0.5, 0.5, 0.5])])
    scene.add_mesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32), m)
    ts = twin.TwinScene(scene)
    # the host twin's copies of the entry points make the checks that need a scene
    T = twin.lib()
    T.twin_bsdf_probe.argtypes = T.twin_light_probe.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    assert T.twin_bsdf_probe(ts._h, 1, buf, 1, buf, buf) != 0              # no such material
    assert T.twin_bsdf_probe(ts._h, 0, buf, 1, None, buf) != 0             # rows missing
    assert T.twin_bsdf_probe(ts._h, 0, buf, (1 << 24) + 1, buf, buf) != 0  # more rows than one launch takes
    assert T.twin_light_probe(ts._h, 0, buf, 1, buf, buf) != 0             # the scene has no light
    assert T.twin_bsdf_probe(ts._h, 0, buf, 1, buf, buf) == 0


def test_texture_and_surface_probes_check_their_arguments(ptrs):
    """ptrs_probe_texture / ptrs_probe_surface refuse a missing scene or row buffers before they touch a device; the host twin's
    copies make the checks that need a scene (texture / triangle index, material chain) -- no GPU needed."""
    L = ptrs.load_library()
    L.ptrs_probe_texture.argtypes = L.ptrs_probe_surface.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
    buf = (C.c_float * 64)()
    for fn in (L.ptrs_probe_texture, L.ptrs_probe_surface):
        assert fn(None, 0, 1, buf, buf) != 0 and b"null" in L.ptrs_last_error()
    import numpy as np
    import twin
    scene = ptrs.RenderScene()
    m = scene.add_material(ptrs.abi.MAT_MATTE, [scene.const_rgb([0.5, 0.5, 0.5])])
    scene.add_mesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32), m)
    ts = twin.TwinScene(scene)
    T = twin.lib()
    T.twin_texture_probe.argtypes = T.twin_surface_probe.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
    assert T.twin_texture_probe(ts._h, 1, 1, buf, buf) != 0                # no such texture
    assert T.twin_texture_probe(ts._h, -1, 1, buf, buf) != 0
    assert T.twin_texture_probe(ts._h, 0, 1, None, buf) != 0               # rows missing
    assert T.twin_texture_probe(ts._h, 0, (1 << 24) + 1, buf, buf) != 0    # more rows than one launch takes
    assert T.twin_surface_probe(ts._h, 1, 1, buf, buf) != 0                # no such triangle
    assert T.twin_surface_probe(ts._h, 0, 1, buf, None) != 0               # out missing
    assert T.twin_texture_probe(ts._h, 0, 1, buf, buf) == 0 and T.twin_surface_probe(ts._h, 0, 1, buf, buf) == 0


def test_shade_table_probe_checks_its_arguments(ptrs):
    """ptrs_probe_shade_tables refuses NULL buffers, no rows, too many rows, an unknown op, a batch size other than 1, 2, 3, 8, a
    dimension past the tables, a u outside [0, 1), a round above 65535 and a missing scene or parameters before it touches a device (no GPU needed); the
    binding's op and route lists end where the header file's do."""
    import numpy as np
    assert "ptrs_probe_shade_tables" in _declared_functions()
    L = ptrs.load_library()
    a = ptrs.abi
    L.ptrs_probe_shade_tables.argtypes = a.PROBE_SHADE_ARGTYPES
    prm = a.PtrsRenderParams()
    prm.width, prm.height, prm.spp, prm.max_depth = 64, 64, 4, 4
    hdr = (C.c_uint32 * 12)()
    out = (C.c_uint32 * 12)()
    row = np.zeros(12, np.uint32)
    row[3], row[4] = 1, 7
    rp = lambda r: C.c_void_p(r.ctypes.data)
    fn = L.ptrs_probe_shade_tables
    assert fn(None, C.byref(prm), 0, 0, 1, None, out, hdr) != 0 and b"null" in L.ptrs_last_error()         # rows missing
    assert fn(None, C.byref(prm), 0, 0, 1, rp(row), None, hdr) != 0 and b"null" in L.ptrs_last_error()     # out missing
    assert fn(None, C.byref(prm), 0, 0, 1, rp(row), out, None) != 0 and b"null" in L.ptrs_last_error()     # header missing
    assert fn(None, C.byref(prm), 0, 0, 0, rp(row), out, hdr) != 0 and b"null" in L.ptrs_last_error()      # nothing to do
    assert fn(None, C.byref(prm), 0, 0, (1 << 24) + 1, rp(row), out, hdr) != 0 and b"too many probe rows" in L.ptrs_last_error()
    for op in (a.PROBE_SHADE_NUM_OPS, 0xffffffff):
        assert fn(None, C.byref(prm), 0, op, 1, rp(row), out, hdr) != 0 and b"unknown shade-table probe op" in L.ptrs_last_error()
    for bad_n in (0, 4, 5, 7, 9, 0xffffffff):
        r = row.copy()
        r[3] = bad_n
        assert fn(None, C.byref(prm), 0, 0, 1, rp(r), out, hdr) != 0 and b"1, 2, 3 or 8" in L.ptrs_last_error(), bad_n
    r = row.copy()
    r[3], r[4:12] = 8, np.arange(1017, 1025)
    assert fn(None, C.byref(prm), 0, 0, 1, rp(r), out, hdr) != 0 and b"1024 dimensions" in L.ptrs_last_error()  # the batch's last dimension
    for u in ((1.0, 0.5), (0.5, 1.0), (-1e-9, 0.5), (np.nan, 0.5)):
        r = np.zeros(12, np.uint32)
        r[0:2] = np.array(u, np.float32).view(np.uint32)
        assert fn(None, C.byref(prm), 0, 1, 1, rp(r), out, hdr) != 0 and b"u outside" in L.ptrs_last_error(), u
    for bad_it in (0x10000, 0xffffffff):
        assert fn(None, C.byref(prm), bad_it, 0, 1, rp(row), out, hdr) != 0 and b"round out of range" in L.ptrs_last_error(), bad_it
    # the rows and the round are in order: what is left is the scene, then the parameters
    assert fn(None, C.byref(prm), 0, 0, 1, rp(row), out, hdr) != 0 and b"null" in L.ptrs_last_error()
    assert fn(None, None, 0, 0, 1, rp(row), out, hdr) != 0 and b"null" in L.ptrs_last_error()
    text = open(os.path.join(ROOT, "pathtracer-rs_amd", "csrc", "pt_probe.h")).read()
    assert re.search(r"PROBE_SHADE_SOBOL = 0, PROBE_SHADE_ENV = 1, PROBE_SHADE_NUM_OPS\b", text) and a.PROBE_SHADE_NUM_OPS == 2
    assert re.search(r"PROBE_SHADE_IN = %d, PROBE_SHADE_OUT = %d, PROBE_SHADE_HEADER = 12\b" % (a.PROBE_SHADE_WIDTH, a.PROBE_SHADE_WIDTH), text)
    assert len(a.PROBE_SHADE_HEADER) <= 12


def test_math_probe_checks_its_arguments(ptrs):
    """ptrs_probe_math refuses a missing buffer, no rows, an unknown op and too many rows before it touches a device (no GPU needed);
    the host twin's copy makes the same checks, and the binding's op list ends where the header's does."""
    assert "ptrs_probe_math" in _declared_functions()
    L = ptrs.load_library()
    L.ptrs_probe_math.argtypes = ptrs.abi.PROBE_MATH_ARGTYPES
    import twin
    T = twin.lib()
    T.twin_math_probe.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    buf = (C.c_float * 16)()
    n_ops = ptrs.abi.MATH_NUM_OPS
    for fn in (lambda *a: L.ptrs_probe_math(0, *a), T.twin_math_probe):
        assert fn(0, 1, None, buf) != 0                # rows missing
        assert fn(0, 1, buf, None) != 0                # out missing
        assert fn(0, 0, buf, buf) != 0                 # nothing to do
        assert fn(n_ops, 1, buf, buf) != 0             # no such op
        assert fn(0xffffffff, 1, buf, buf) != 0
        assert fn(0, (1 << 24) + 1, buf, buf) != 0     # more rows than one launch takes
    for err in (L.ptrs_last_error(), T.twin_last_error()):
        assert b"too many probe rows" in err
    assert L.ptrs_probe_math(0, n_ops, 1, buf, buf) != 0 and b"bad math probe request" in L.ptrs_last_error()
    assert T.twin_math_probe(n_ops - 1, 1, buf, buf) == 0 and T.twin_math_probe(0, 1, buf, buf) == 0
    text = open(os.path.join(ROOT, "pathtracer-rs_amd", "csrc", "pt_probe.h")).read()
    ops = re.search(r"MATH_SIN = 0,(.*?)MATH_NUM_OPS", text, flags=re.S).group(1)
    assert len(re.findall(r"\bMATH_[A-Z0-9_]+\b", "MATH_SIN," + re.sub(r"//.*", "", ops))) == n_ops
