"""The thin-lens camera (PtrsCameraLens, PTRS_FLAG_THIN_LENS): known answers from outside the device code.

The reference has no lens (CameraSample holds p_film alone, sampler/mod.rs:162-166), so there is no oracle.  What holds the feature:
  * pt::lens_ray (the host-compiled function of tests/lens_twin) against a float64 restatement of the definition with the running
    rounding bound of tests/test_camera_film_kat.py (class B: every binary32 operation adds 2^-24 |result| to its operands' bounds),
    and against the geometry that needs no formula: every lens ray of one p_film passes through the point where the pinhole ray
    crosses the plane in focus;
  * a lens of radius 0 is the pinhole render bit for bit, flag or no flag;
  * under -m gpu: the device's generated rays, a depth-0 render of coloured emissive quads and the first-hit positions against
    float64 lens rays made from the Sobol' values of the generator matrices; device == host twin per sample on every kernel form
    the lens touches; the entry points against each other; one closed-form radiance that does not depend on the camera ray.
The two-dimension shift of the path's Sobol' counter has no implementation from outside to be pinned against: it is held by the
definition (dimensions 2 and 3 behind the film sample) and by device == twin.
"""
import ctypes as C
import importlib
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import twin
from conftest import CORNELL, ROOT
from test_camera_film_kat import B, CAMERAS, EPS, F32, b_normalize, b_rotate, bits, outside_pfilm, pfilm_rows, ref_camera_rays, sorted_rows, stack_e, stack_v

sys.path.insert(0, os.path.join(ROOT, "tests", "lens_twin"))
import lens_twin  # noqa: E402
import shade_cases as sc  # noqa: E402

ptrs = importlib.import_module("pathtracer-rs_amd")
A = ptrs.abi
CLI = os.path.join(ROOT, "pathtracer-rs_amd", "ptrs_headless")
PI_4, PI_2 = float(F32(math.pi / 4)), float(F32(math.pi / 2))  # the binary32 constants of the disk mapping
ONE_MINUS_EPS = float.fromhex("0x1.fffffep-1")
ERR_INVALID, ERR_UNSUPPORTED = -1, -2


# ---- the definition in float64, with and without the running bound ---------------------------------------------------------------
def b_where(m, a, b):
    return B(np.where(m, a.v, b.v), np.where(m, a.e, b.e))


def b_sincos(t):
    """sin and cos of a bounded angle: |sin x - sin y| <= |x - y|, then one rounding (pt_sincosf rounds the binary64 value, itself
    within 2^-48 relative: 2^-47 absolute is added for the double rounding)."""
    return B._round(np.sin(t.v), t.e + 2.0 ** -47), B._round(np.cos(t.v), t.e + 2.0 ** -47)


def b_disk(ul):
    """Shirley's concentric map (sampling.rs concentric_sample_disk) of binary32 u: (x, y) as B.  The branch is taken by the binary32
    offsets, as any binary32 evaluation takes it; on the diagonal both branches give the same point."""
    u32 = np.asarray(ul, F32)
    o32 = F32(2) * u32 - F32(1)
    first = np.abs(o32[:, 0]) > np.abs(o32[:, 1])
    zero = (o32[:, 0] == 0) & (o32[:, 1] == 0)
    u = u32.astype(np.float64)
    ox, oy = B(u[:, 0]) * 2.0 - 1.0, B(u[:, 1]) * 2.0 - 1.0
    with np.errstate(all="ignore"):
        ta = B(PI_4) * (oy / ox)
        tb = B(PI_2) - B(PI_4) * (ox / oy)
    theta, r = b_where(first, ta, tb), b_where(first, ox, oy)
    theta = b_where(zero, B(np.zeros(len(u))), theta)
    sn, cs = b_sincos(theta)
    x, y = r * cs, r * sn
    z = B(np.zeros(len(u)))
    return b_where(zero, z, x), b_where(zero, z, y)


def b_camera_point(cam, pf):
    """p_camera of a raster point (the head of ref_camera_rays: Affine3 * Point3, Perspective3::unproject_point)."""
    pf = np.asarray(pf, F32).astype(np.float64)
    x, y = B(pf[:, 0]), B(pf[:, 1])
    m = cam.raster_to_screen.astype(np.float64)
    s = [((B(m[i, 0]) * x + B(m[i, 1]) * y) + B(m[i, 2]) * 0.0) + B(m[i, 3]) for i in range(3)]
    inv = B(float(cam.m23)) / (s[2] + B(float(cam.m22)))
    return [s[0] * inv / B(float(cam.m00)), s[1] * inv / B(float(cam.m11)), -inv]


def ref_lens_rays(cam, diff_scale, pf, ul):
    """The issue's definition, operation by operation: dir = normalize(pc); pl = disk(u) * R; ft = f / -dir.z; oc = (pl, 0);
    o = rot * oc + trans; d = normalize(rot * (dir * ft - oc)); rx_d = d + (pin.rx_d - pin.d), ry_d likewise.  dict of lists of three B."""
    pin = ref_camera_rays(cam, diff_scale, pf)
    R, f = B(float(F32(cam.lens_radius))), B(float(F32(cam.focal_distance)))
    dirc = b_normalize(b_camera_point(cam, pf))
    dx, dy = b_disk(ul)
    n = len(np.asarray(pf).reshape(-1, 2))
    oc = [dx * R, dy * R, B(np.zeros(n))]
    ft = f / (-dirc[2])
    q = cam.rot.astype(np.float64)
    ro = b_rotate(q, oc)
    o = [ro[k] + B(float(cam.trans[k])) for k in range(3)]
    d = b_normalize(b_rotate(q, [dirc[k] * ft - oc[k] for k in range(3)]))
    out = dict(o=o, d=d, pin=pin, dirc=dirc)
    for key in ("rx_d", "ry_d"):
        out[key] = [d[k] + (pin[key][k] - pin["d"][k]) for k in range(3)]
    return out


def rot64(q, v):
    qv = q[:3]
    t = 2.0 * np.cross(qv, v)
    return v + q[3] * t + np.cross(qv, t)


def disk64(u):
    u = np.asarray(u, np.float64)
    ox, oy = 2.0 * u[:, 0] - 1.0, 2.0 * u[:, 1] - 1.0
    first = np.abs(ox) > np.abs(oy)
    with np.errstate(all="ignore"):
        theta = np.where(first, (math.pi / 4) * (oy / ox), math.pi / 2 - (math.pi / 4) * (ox / oy))
    r = np.where(first, ox, oy)
    zero = (ox == 0) & (oy == 0)
    theta, r = np.where(zero, 0.0, theta), np.where(zero, 0.0, r)
    return np.stack([r * np.cos(theta), r * np.sin(theta)], axis=1)


def lens_rays64(cam, pf, ul):
    """The lens ray in plain float64 (o, d): the render tests' reference."""
    pf = np.asarray(pf, np.float64).reshape(-1, 2)
    m = cam.raster_to_screen.astype(np.float64)
    s = pf[:, :1] * m[:3, 0] + pf[:, 1:] * m[:3, 1] + m[:3, 3]
    inv = float(cam.m23) / (s[:, 2] + float(cam.m22))
    pc = np.stack([s[:, 0] * inv / float(cam.m00), s[:, 1] * inv / float(cam.m11), -inv], axis=1)
    dirc = pc / np.linalg.norm(pc, axis=1, keepdims=True)
    pl = disk64(ul) * float(F32(cam.lens_radius))
    oc = np.concatenate([pl, np.zeros((len(pl), 1))], axis=1)
    ft = float(F32(cam.focal_distance)) / (-dirc[:, 2:3])
    q = cam.rot.astype(np.float64)
    o = rot64(q, oc) + cam.trans.astype(np.float64)
    d = rot64(q, dirc * ft - oc)
    return o, d / np.linalg.norm(d, axis=1, keepdims=True)


def ulens_grid():
    g = [0.0, 0.125, 0.25, 0.5, 0.7, ONE_MINUS_EPS]
    rows = [(a, b) for a in g for b in g] + [(0.5, 0.5), (0.75, 0.25), (0.25, 0.75), (0.3, 0.3), (0.5, 0.9), (0.9, 0.5)]
    return np.array(rows, F32)


def crossed(pf, ul):
    return np.repeat(pf, len(ul), axis=0), np.tile(ul, (len(pf), 1))


LENS_CASES = [("identity_24x16_fov50", 0.05, 2.5), ("generic_37x21_fov120", 0.3, 1.0), ("matrix_generic_17x31_fov20", 0.02, 40.0), ("turned180_17x31_fov20", 1.5, 6.0)]


def lens_case(name, radius, focal):
    cam, fovy, fwd, ds = CAMERAS[name]
    return cam.with_lens(radius, focal), fwd, ds


# ---- CPU: the lens ray -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,radius,focal", LENS_CASES)
def test_lens_ray_against_float64(name, radius, focal):
    """o, d, rx_d, ry_d of pt::lens_ray against the float64 restatement with its running bound, over the p_film grid of the pinhole
    test crossed with a grid of lens samples (corners, centre, both branches of the disk mapping and its diagonal).  The bound is built
    from operation counts; two conditions keep it from hiding a failure: at most 2^-15 on d, and o within 2^-18 of the lens radius
    plus one rounding of the camera's position."""
    cam, fwd, ds = lens_case(name, radius, focal)
    pf, ul = crossed(pfilm_rows(cam.film.width, cam.film.height)[::3], ulens_grid())
    got = lens_twin.lens_rays(cam, ds, pf, ul).astype(np.float64)
    ref = ref_lens_rays(cam, ds, pf, ul)
    worst = 0.0
    for k, key in enumerate(("o", "d", "rx_d", "ry_d")):
        v, e = stack_v(ref[key]), stack_e(ref[key])
        err = np.abs(got[:, 3 * k:3 * k + 3] - v)
        bad = (err > e).any(axis=1)
        assert not bad.any(), "%s %s: %d rays outside the bound, first (p_film %s, u %s): %s vs %s (bound %s)" % (
            name, key, bad.sum(), pf[bad][0], ul[bad][0], got[bad][0, 3 * k:3 * k + 3], v[bad][0], e[bad][0])
        worst = max(worst, float((err / np.maximum(e, 1e-300)).max()))
    print("%s: worst |twin - f64| / bound = %.3f, bound on d <= %.3g" % (name, worst, stack_e(ref["d"]).max()))
    assert stack_e(ref["d"]).max() <= 2.0 ** -15
    assert (stack_e(ref["o"]) <= 2.0 ** -18 * radius + EPS * np.abs(cam.trans.astype(np.float64)) * 1.01).all()
    # the differentials are the pinhole's offsets: rx_d - d is pin.rx_d - pin.d up to the two roundings of forming rx_d and the difference
    pin = twin.camera_rays(cam.with_lens(0, 0), ds, pf).astype(np.float64)
    for k in (6, 9):
        lhs, rhs = got[:, k:k + 3] - got[:, 3:6], pin[:, k:k + 3] - pin[:, 3:6]
        assert (np.abs(lhs - rhs) <= EPS * (np.abs(got[:, k:k + 3]) + np.abs(rhs)) * 1.01).all(), name


@pytest.mark.parametrize("name,radius,focal", LENS_CASES)
def test_lens_geometry_without_formula(name, radius, focal):
    """All lens rays of one p_film meet where the pinhole ray crosses the plane at camera depth focal_distance; their origins lie in
    the lens plane within lens_radius of the camera's position; the lens centre (u = 1/2, 1/2) is the camera's position.
    The plane is taken from outside the camera's fields: the forward axis `fwd` of the test's own look-at / matrix, which the camera
    holds within 18 * 2^-24 (test_camera_geometry_without_formula).  P = eye + d_pin f / (d_pin . fwd): its error is t (e_pin + the
    relative error of t) with t = f / cos, d(t) / t <= (18 * 2^-24 + e_pin) / cos.  A lens ray (o, d) passes P within |P - o| e_d + e_o + err(P),
    e_o, e_d, e_pin the running bounds of the float64 test (norms over the components)."""
    cam, fwd, ds = lens_case(name, radius, focal)
    pf, ul = crossed(pfilm_rows(cam.film.width, cam.film.height)[::7], ulens_grid())
    got = lens_twin.lens_rays(cam, ds, pf, ul).astype(np.float64)
    ref = ref_lens_rays(cam, ds, pf, ul)
    e_o, e_d, e_pin = (np.linalg.norm(stack_e(v), axis=1) for v in (ref["o"], ref["d"], ref["pin"]["d"]))
    eye = cam.trans.astype(np.float64)
    f = float(F32(focal))
    d_pin = twin.camera_rays(cam.with_lens(0, 0), ds, pf).astype(np.float64)[:, 3:6]
    cos = d_pin @ fwd
    assert (cos > 0.05).all()
    t = f / cos
    P = eye + d_pin * t[:, None]
    err_P = t * e_pin + t * (18 * EPS + e_pin) / cos
    o, d = got[:, 0:3], got[:, 3:6]
    w = P - o
    dist = np.linalg.norm(w - (w * d).sum(axis=1, keepdims=True) * d, axis=1)
    tol = np.linalg.norm(w, axis=1) * e_d + e_o + err_P
    assert (dist <= tol).all(), (name, float((dist / tol).max()))
    assert (tol <= 1e-4 * f).all()  # the allowance itself stays far below the blur a lens makes: radius * |depth - f| / f
    print("%s: worst distance from the focus point / allowance = %.3f" % (name, float((dist / tol).max())))
    # the lens plane and the disk: (o - eye) . fwd = 0 and |o - eye| <= radius, up to the bound on o and the axis' 18 * 2^-24
    rel = o - eye
    assert (np.abs(rel @ fwd) <= e_o + 18 * EPS * radius).all()
    assert (np.linalg.norm(rel, axis=1) <= radius * (1 + 4 * EPS) + e_o).all()
    assert np.linalg.norm(rel, axis=1).max() >= 0.99 * radius  # the grid's corners reach the rim
    centre = (ul == F32(0.5)).all(axis=1)
    assert centre.any() and np.array_equal(bits(got[centre, 0:3]), bits(np.broadcast_to(cam.trans, (centre.sum(), 3))))
    # a ray through the lens centre is the pinhole ray's direction up to the bound (its focus point is on the pinhole ray)
    assert (np.linalg.norm(d[centre] - d_pin[centre], axis=1) <= (e_d + e_pin)[centre]).all()


# ---- CPU: radius 0, refusals, ABI, importers, the stratified requirement -----------------------------------------------------------
def lens_abi(cam, radius, focal):
    cl = A.PtrsCameraLens()
    cam._fill_abi(cl.camera)
    cl.lens_radius, cl.focal_distance = radius, focal
    return cl


def twin_render_raw(tscene, cam_abi, p):
    """twin_render with the camera struct as given (a PtrsCameraLens under the flag): per-sample radiance and the statistics."""
    film = np.zeros((p.height, p.width), dtype=A.FILM_DTYPE)
    spp = p.spp if p.sampler == A.SAMPLER_STRATIFIED else twin.round_up_pow2(p.spp)
    samples = np.zeros((p.height + 4, p.width + 4, spp, 3), dtype=np.float32)
    st = A.PtrsStats()
    rc = twin.lib().twin_render(tscene._h, C.byref(cam_abi), C.byref(p), C.c_void_p(film.ctypes.data), C.c_void_p(samples.ctypes.data), C.byref(st))
    return rc, film, samples, st


def test_lens_of_radius_zero_is_the_pinhole(orc):
    """Cornell 16 x 16, 4 spp, depth 4: with the flag set and lens_radius 0 (whatever focal_distance says) the twin's samples, film
    and ray counts are those of the unflagged render, which are the oracle's."""
    cam, scene = ptrs.import_scene(CORNELL, (16, 16))
    t = twin.TwinScene(scene)
    p = orc.make_params(16, 16, 4, 4)
    f0, s0, st0 = t.render(cam, p, want_samples=True)
    _, so, sto = orc.OracleScene(scene).render(cam, p, n_threads=4, want_samples=True)
    assert np.array_equal(bits(s0), bits(so)) and (st0.rays_extension, st0.rays_shadow, st0.rays_mis) == (sto.rays_extension, sto.rays_shadow, sto.rays_mis)
    pl = orc.make_params(16, 16, 4, 4, flags=A.FLAG_THIN_LENS)
    for focal in (0.0, 3.0, float("nan")):
        rc, f1, s1, st1 = twin_render_raw(t, lens_abi(cam, 0.0, focal), pl)
        assert rc == 0
        assert np.array_equal(bits(s1), bits(s0)) and np.array_equal(f1.view(np.uint32), f0.view(np.uint32))
        assert (st1.rays_extension, st1.rays_shadow, st1.rays_mis) == (st0.rays_extension, st0.rays_shadow, st0.rays_mis)
    # and a lens that is one changes the samples (the flag is read)
    rc, _, s2, _ = twin_render_raw(t, lens_abi(cam, 0.2, 5.0), pl)
    assert rc == 0 and not np.array_equal(bits(s2), bits(s0))
    # the Python host sets the flag exactly when there is a lens
    integ = ptrs.PathIntegrator(ptrs.SamplerBuilder(4, cam.film.get_sample_bounds()), 4)
    assert integ.params(cam).flags & A.FLAG_THIN_LENS == 0 and isinstance(cam.to_abi(), A.PtrsCamera)
    cl = cam.with_lens(0.2, 5.0)
    assert integ.params(cl).flags & A.FLAG_THIN_LENS and isinstance(cl.to_abi(), A.PtrsCameraLens)
    assert bytes(cl.to_abi())[:C.sizeof(A.PtrsCamera)] == bytes(cam.to_abi())
    back = cl.with_lens(0.0, 7.0)
    assert (back.lens_radius, back.focal_distance) == (0.0, 0.0) and isinstance(back.to_abi(), A.PtrsCamera)


BAD_LENSES = [(-0.1, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (0.1, 0.0), (0.1, -2.0), (0.1, float("nan")), (0.1, float("inf"))]
# sizeof of the structs before the lens, by ptrs_abi_sizeof index (ABI version 4 as it stood)
SIZES_V4 = [80, 36, 64, 240, 32, 88, 132, 56, 464, 20, 16, 20, 8, 24, 272, 12, 408]


def test_bad_lens_is_refused_without_a_device():
    """Every (camera, params) entry point answers a bad lens with PTRS_ERR_INVALID before it looks at anything else -- no scene, no
    film, no device is needed to be told so; the same calls with a good lens get as far as the null scene."""
    L = ptrs.load_library()
    L.ptrs_last_error.restype = C.c_char_p
    cam, _ = ptrs.import_scene(CORNELL, (16, 16))
    p = ptrs.PathIntegrator(ptrs.SamplerBuilder(4, cam.film.get_sample_bounds()), 2).params(cam)
    p.flags |= A.FLAG_THIN_LENS
    N = None
    u32, f32 = C.c_uint32, C.c_float

    def calls(cl):
        c, q = C.byref(cl), C.byref(p)
        z = u32(0)
        return {
            "render": lambda: L.ptrs_render(N, c, q, N, N),
            "render_device": lambda: L.ptrs_render_device(N, c, q, N, N, N),
            "render_samples": lambda: L.ptrs_render_samples(N, c, q, N, N, N),
            "render_progressive": lambda: L.ptrs_render_progressive(N, c, q, N, N, N, N),
            "render_multi": lambda: L.ptrs_render_multi(N, z, c, q, N, N, N),
            "render_row_cost": lambda: L.ptrs_render_row_cost(N, c, q, N, N),
            "render_single_pixel": lambda: L.ptrs_render_single_pixel(N, c, q, C.c_int32(0), C.c_int32(0), N),
            "render_dump_rays": lambda: L.ptrs_render_dump_rays(N, c, q, z, z, N, N),
            "render_aov": lambda: L.ptrs_render_aov(N, c, q, u32(7), N, N, N),
            "render_aov_device": lambda: L.ptrs_render_aov_device(N, c, q, u32(7), N, N, N, N),
            "render_range": lambda: L.ptrs_render_range(N, c, q, z, u32(1), N, N, N, N),
            "render_range_device": lambda: L.ptrs_render_range_device(N, c, q, z, u32(1), N, N, N, N),
            "render_tiles": lambda: L.ptrs_render_tiles(N, c, q, z, u32(1), N, N, N, N, N),
            "render_tiles_device": lambda: L.ptrs_render_tiles_device(N, c, q, z, u32(1), N, N, N, N, N),
            "render_converged": lambda: L.ptrs_render_converged(N, c, q, f32(0.1), u32(2), N, N, N, N),
            "render_adaptive": lambda: L.ptrs_render_adaptive(N, c, q, f32(0.1), u32(2), N, N, N, N, N),
            "render_aov_range": lambda: L.ptrs_render_aov_range(N, c, q, z, u32(1), u32(7), N, N, N),
            "render_aov_range_device": lambda: L.ptrs_render_aov_range_device(N, c, q, z, u32(1), u32(7), N, N, N, N),
            "render_aov_tiles": lambda: L.ptrs_render_aov_tiles(N, c, q, z, u32(1), N, u32(7), N, N, N),
            "render_aov_tiles_device": lambda: L.ptrs_render_aov_tiles_device(N, c, q, z, u32(1), N, u32(7), N, N, N, N),
            "render_aov_adaptive": lambda: L.ptrs_render_aov_adaptive(N, c, q, u32(2), N, u32(7), N, N),
            "render_aov_adaptive_device": lambda: L.ptrs_render_aov_adaptive_device(N, c, q, u32(2), N, u32(7), N, N, N),
        }
    for r, f in BAD_LENSES:
        for name, call in calls(lens_abi(cam, r, f)).items():
            assert call() == ERR_INVALID, (name, r, f)
            assert b"thin lens" in L.ptrs_last_error(), (name, r, f, L.ptrs_last_error())
    for r, f in ((0.0, float("nan")), (0.1, 2.0)):  # good lenses: refused for the null scene, not for the lens
        for name, call in calls(lens_abi(cam, r, f)).items():
            assert call() == ERR_INVALID, name
            assert b"thin lens" not in L.ptrs_last_error(), (name, L.ptrs_last_error())
    # the host twin's set-up (render_setup) refuses the same lenses
    t = twin.TwinScene(ptrs.import_scene(CORNELL, (16, 16))[1])
    for r, f in BAD_LENSES:
        rc, _, _, _ = twin_render_raw(t, lens_abi(cam, r, f), p)
        assert rc == ERR_INVALID, (r, f)
    # Camera.with_lens refuses them before any call
    for r, f in BAD_LENSES:
        with pytest.raises(ValueError):
            cam.with_lens(r, f)


def test_abi_grows_by_new_symbols_only():
    L = ptrs.load_library()
    assert L.ptrs_abi_version() == 4
    assert [L.ptrs_abi_sizeof(k) for k in range(len(SIZES_V4))] == SIZES_V4
    assert L.ptrs_abi_sizeof(17) == C.sizeof(A.PtrsCameraLens) == C.sizeof(A.PtrsCamera) + 8 == 140
    assert L.ptrs_abi_sizeof(18) == -1
    assert A.PtrsCameraLens.camera.offset == 0 and A.PtrsCameraLens.lens_radius.offset == 132 and A.PtrsCameraLens.focal_distance.offset == 136
    assert A.FLAG_THIN_LENS == 8
    assert hasattr(L, "ptrs_camera_focus_distance")


SENSOR = """<?xml version="1.0" encoding="utf-8"?>
<scene version="0.5.0" >
	<sensor type="%s" >
		<float name="fov" value="24" />%s
		<transform name="toWorld" ><matrix value="-1 0 0 0 0 1 0 1 0 0 -1 6.8 0 0 0 1"/></transform>
		<film type="ldrfilm" ><integer name="width" value="96" /><integer name="height" value="64" /></film>
	</sensor>
	<shape type="rectangle" >
		<transform name="toWorld" ><matrix value="2 0 0 0 0 0 2 0 0 -2 0 0 0 0 0 1"/></transform>
		<bsdf type="diffuse" ><rgb name="reflectance" value="0.5, 0.5, 0.5"/></bsdf>
	</shape>
	<shape type="rectangle" >
		<transform name="toWorld" ><matrix value="0.4 0 0 0 0 0.4 0 1 0 0 0.4 3 0 0 0 1"/></transform>
		<bsdf type="diffuse" ><rgb name="reflectance" value="0.5, 0.5, 0.5"/></bsdf>
		<emitter type="area" ><rgb name="radiance" value="3, 2, 1"/></emitter>
	</shape>
</scene>
"""
LENS_FLOATS = """
		<float name="aperture_radius" value="0.125" />
		<float name="focus_distance" value="6.75" />"""


def read_dump_lens(path):
    b = open(path, "rb").read()
    assert b[:8] == b"PTRSDUMP" and b[-12:-8] == b"LENS"
    return struct.unpack("<ff", b[-8:]), b[8:8 + C.sizeof(A.PtrsCamera)]


def test_importers_read_the_thinlens_sensor(tmp_path):
    """<sensor type="thinlens"> gives the camera aperture_radius and focus_distance in the Python importer and in the C++ importer
    (through ptrs_headless --dump-scene, whose dump ends in the lens); the same scene as `perspective` gives 0, 0 and the same
    PtrsCamera."""
    importlib.import_module("pathtracer-rs_amd.build").build_host()
    paths = {}
    for kind, extra in (("thinlens", LENS_FLOATS), ("perspective", ""), ("perspective_with_floats", LENS_FLOATS)):
        paths[kind] = str(tmp_path / (kind + ".xml"))
        with open(paths[kind], "w") as f:
            f.write(SENSOR % (kind.split("_")[0], extra))
    cams, dumps = {}, {}
    for kind, path in paths.items():
        cams[kind], _ = ptrs.import_scene(path, (48, 32))
        dump = str(tmp_path / (kind + ".dump"))
        subprocess.check_call([CLI, path, "--dump-scene", dump, "-r", "48x32"])
        dumps[kind] = read_dump_lens(dump)
    assert (cams["thinlens"].lens_radius, cams["thinlens"].focal_distance) == (0.125, 6.75)
    assert dumps["thinlens"][0] == (0.125, 6.75)
    for kind in ("perspective", "perspective_with_floats"):  # a pinhole sensor has no lens, whatever else it carries
        assert (cams[kind].lens_radius, cams[kind].focal_distance) == (0.0, 0.0)
        assert dumps[kind][0] == (0.0, 0.0)
    pin = bytes(cams["perspective"].to_abi())
    assert bytes(cams["thinlens"].to_abi())[:len(pin)] == pin == dumps["thinlens"][1] == dumps["perspective"][1]
    # a thinlens sensor without its two floats is an error in both, not a silent pinhole
    bad = str(tmp_path / "bad.xml")
    with open(bad, "w") as f:
        f.write(SENSOR % ("thinlens", ""))
    with pytest.raises(ValueError, match="thinlens"):
        ptrs.import_scene(bad, (48, 32))
    r = subprocess.run([CLI, bad, "--dump-scene", str(tmp_path / "bad.dump")], capture_output=True, text=True)
    assert r.returncode != 0 and "thinlens" in r.stderr


def test_cli_lens_flags_are_checked(tmp_path):
    """--aperture / --focus / --focus_at: malformed values and a lens without a focus distance are errors before anything is rendered."""
    importlib.import_module("pathtracer-rs_amd.build").build_host()
    out = str(tmp_path)
    for args, word in ((["--focus_at", "12"], "X,Y"), (["--focus_at", "1,2", "--focus", "3"], "exclude"), (["--aperture"], "needs a value")):
        r = subprocess.run([CLI, CORNELL, "-o", out] + args, capture_output=True, text=True)
        assert r.returncode == 2 and word in r.stderr, (args, r.stderr)
    r = subprocess.run([CLI, CORNELL, "-o", out, "--aperture", "0.1"], capture_output=True, text=True)  # Cornell's sensor is a pinhole: nothing says where the focus is
    assert r.returncode == 2 and "bad lens" in r.stderr, r.stderr
    r = subprocess.run([CLI, CORNELL, "-o", out, "--aperture", "-1", "--focus", "3"], capture_output=True, text=True)
    assert r.returncode == 2 and "bad lens" in r.stderr, r.stderr


def test_stratified_lens_needs_one_more_dimension(orc):
    """The lens sample is the pixel table's second 2-D dimension: under a lens n_sampled_dimensions must be 3 (max_depth + 1) + 2;
    one below is refused as too few dimensions are today (PTRS_ERR_UNSUPPORTED), without a lens that count is still enough."""
    cam, scene = ptrs.import_scene(CORNELL, (12, 12))
    t = twin.TwinScene(scene)
    depth = 2
    need = 3 * (depth + 1) + 1

    def params(nd, flags):
        return orc.make_params(12, 12, 4, depth, sampler=A.SAMPLER_STRATIFIED, n_sampled_dimensions=nd, flags=flags)
    lens = lens_abi(cam, 0.1, 6.0)
    rc, _, s_pin, _ = twin_render_raw(t, cam.to_abi(), params(need, 0))
    assert rc == 0
    assert twin_render_raw(t, lens, params(need, A.FLAG_THIN_LENS))[0] == ERR_UNSUPPORTED
    assert b"n_sampled_dimensions" in twin.lib().twin_last_error()
    rc, _, s_lens, st = twin_render_raw(t, lens, params(need + 1, A.FLAG_THIN_LENS))
    assert rc == 0 and st.error_flags == 0 and not np.array_equal(bits(s_lens), bits(s_pin))
    rc, _, s_zero, _ = twin_render_raw(t, lens_abi(cam, 0.0, 0.0), params(need, A.FLAG_THIN_LENS))  # radius 0: no lens dimension is drawn
    assert rc == 0 and np.array_equal(bits(s_zero), bits(s_pin))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def integrator(cam, spp, depth):
    return ptrs.PathIntegrator(ptrs.SamplerBuilder(spp, cam.film.get_sample_bounds()), depth)


_ulens = {}


def outside_ulens(W, H, spp):
    """u_lens of every (sample pixel, sample): Sobol' dimensions 2 and 3 in integers from the generator matrices (shade_cases.
    sobol_reference), at the index whose defining property outside_pfilm has checked and under the pixel's Cantor scramble."""
    if (W, H, spp) not in _ulens:
        yy, xx, ss = np.meshgrid(np.arange(-2, H + 2), np.arange(-2, W + 2), np.arange(spp), indexing="ij")
        px, py, sn = xx.ravel(), yy.ravel(), ss.ravel()
        p = A.PtrsRenderParams()
        p.width, p.height, p.spp, p.max_depth = W, H, spp, 1
        outside_pfilm(W, H, spp, "twin")  # (asserts what makes idx the sample's index)
        _, idx = twin.sobol_samples(p, px, py, sn, np.zeros(len(px), np.uint32))
        u = sc.sobol_reference(sc.sobol_matrices(), idx.astype(np.int64), sc.cantor_scramble(px, py), np.tile([2, 3], (len(px), 1)))
        u = u.reshape(H + 4, W + 4, spp, 2)
        u.setflags(write=False)
        _ulens[(W, H, spp)] = u
    return _ulens[(W, H, spp)]


@pytest.mark.gpu
@pytest.mark.parametrize("deal", [0, 1])
@pytest.mark.parametrize("W,H,spp", [(20, 12, 4), (37, 21, 1)])
def test_generated_lens_rays_are_the_samples_rays(W, H, spp, deal):
    """k_generate under a lens: the camera rays of one pass (dump_rays, round 0) are, as a multiset and bit for bit, pt::lens_ray of
    the outside (p_film, u_lens) of every (pixel, sample), with both ways of dealing paths to the queue segments."""
    cam, scene = ptrs.import_scene(CORNELL, (W, H))
    cam = cam.with_lens(0.15, 6.0)
    integ = integrator(cam, spp, 3)
    n = (W + 4) * (H + 4) * spp
    with ptrs.options(deal=deal):
        rays = ptrs.dump_rays(integ, cam, scene, 0, 2 * n)
    assert len(rays) == n
    pf, _ = outside_pfilm(W, H, spp, "twin")
    want = lens_twin.lens_rays(cam, 1.0 / math.sqrt(spp), pf.reshape(-1, 2), outside_ulens(W, H, spp).reshape(-1, 2))[:, :6]
    assert np.isinf(rays[:, 6]).all()
    assert np.array_equal(sorted_rows(rays[:, :6]), sorted_rows(want))
    pin = twin.camera_rays(cam.with_lens(0, 0), 1.0 / math.sqrt(spp), pf.reshape(-1, 2))[:, :6]
    assert not np.array_equal(sorted_rows(want), sorted_rows(pin))


@pytest.mark.gpu
@pytest.mark.parametrize("deal", [0, 1])
def test_generated_lens_rays_of_the_stratified_sampler(orc, deal):
    """The same with the stratified sampler: a 12 x 12 film's sample bounds are one 16 x 16 tile (seed 0), whose tables the oracle's
    restatement of the StratifiedSampler gives; p_film is the pixel's first 2-D dimension (held first against the pinhole's rays),
    u_lens its second."""
    W = H = 12
    dim, nd = 2, 8
    spp = dim * dim
    cam, scene = ptrs.import_scene(CORNELL, (W, H))
    t = orc.stratified_tile(0, 16, 16, dim, nd)  # pixels x-major; per pixel [nd * spp 1-D | nd * spp * 2 2-D]
    t2 = t[:, nd * spp:].reshape(16, 16, nd, spp, 2)  # [x][y][dimension][sample]
    px, py = np.meshgrid(np.arange(-2, 14), np.arange(-2, 14), indexing="ij")
    pf = (np.stack([px, py], -1).astype(F32)[:, :, None, :] + t2[:, :, 0]).astype(F32).reshape(-1, 2)
    ul = t2[:, :, 1].reshape(-1, 2)
    n = 16 * 16 * spp
    for lens, camera in ((False, cam), (True, cam.with_lens(0.15, 6.0))):
        integ = ptrs.PathIntegrator(ptrs.StratifiedSamplerBuilder(dim, nd), 1)
        with ptrs.options(deal=deal):
            rays = ptrs.dump_rays(integ, camera, scene, 0, 2 * n)
        assert len(rays) == n
        want = lens_twin.lens_rays(camera, 1.0 / math.sqrt(spp), pf, ul)[:, :6]
        assert np.array_equal(sorted_rows(rays[:, :6]), sorted_rows(want)), "lens" if lens else "pinhole"


# the coloured quads: six unit squares in a plane across the view axis, 0.1 apart, each emitting its own binary32-exact colour
QUAD_CENTRES = [(-1.1, -0.55), (0.0, -0.55), (1.1, -0.55), (-1.1, 0.55), (0.0, 0.55), (1.1, 0.55)]
QUAD_COLOURS = np.array([[1, 0.5, 0.25], [0.5, 1, 0.25], [0.25, 0.5, 1], [2, 0.125, 0.5], [0.125, 2, 1], [4, 4, 0.25]], np.float64)
QUAD_HALF, EDGE_DELTA = 0.5, 1e-4
QW, QH, QSPP = 24, 16, 8


def quads_scene(z):
    s = ptrs.RenderScene()
    black = s.add_material(A.MAT_MATTE, [s.const_rgb([0.0, 0.0, 0.0])])
    for (cx, cy), col in zip(QUAD_CENTRES, QUAD_COLOURS):
        sc._quad(s, [cx, cy, z], [QUAD_HALF, 0, 0], [0, QUAD_HALF, 0], black, uv=False, emission_rgb=col.astype(np.float32))
    cam = ptrs.look_at_camera([0, 0, 0], [0, 0, -1], [0, 1, 0], 40.0, (QW, QH))
    return cam, s


def quad_lookup(o, d, z):
    """Where float64 rays cross the plane at depth z: the point, the colour seen there (0 between the quads) and whether the point lies
    within EDGE_DELTA quad sides of a quad's edge."""
    t = (z - o[:, 2]) / d[:, 2]
    p = o + d * t[:, None]
    colour, near = np.zeros((len(p), 3)), np.zeros(len(p), bool)
    for (cx, cy), col in zip(QUAD_CENTRES, QUAD_COLOURS):
        m = np.maximum(np.abs(p[:, 0] - cx), np.abs(p[:, 1] - cy)) - QUAD_HALF  # < 0 inside
        colour[m < 0] = col
        near |= np.abs(m) < EDGE_DELTA * 2 * QUAD_HALF
    return p, colour, near


def lens_samples64(cam):
    pf, _ = outside_pfilm(QW, QH, QSPP, "twin")
    return lens_rays64(cam, pf.reshape(-1, 2), outside_ulens(QW, QH, QSPP).reshape(-1, 2))


@pytest.mark.gpu
def test_depth0_render_shows_what_the_float64_lens_ray_hits():
    """max_depth 0, the quads at depth 4, the focus at 2.5: the radiance of every sample is the colour of the quad its float64 lens ray
    (same Sobol' values, from the matrices) hits, or black -- bit for bit, the colours being exact.  Samples within 1e-4 quad sides of an
    edge are left out: 2 delta * 24 edge lengths over the 6.4 x 4.3 the sample bounds see at that depth, far below the 1 % asserted.
    The lens is wide enough that a pinhole render of the same samples differs in many of them."""
    cam, scene = quads_scene(-4.0)
    cam = cam.with_lens(0.25, 2.5)
    got = integrator(cam, QSPP, 0).render(cam, scene, want_samples=True).reshape(-1, 3)
    o, d = lens_samples64(cam)
    _, colour, near = quad_lookup(o, d, -4.0)
    assert near.mean() <= 0.01, near.mean()
    keep = ~near
    assert np.array_equal(got[keep].astype(np.float64), colour[keep]), "%d of %d samples differ" % ((got[keep] != colour[keep]).any(axis=1).sum(), keep.sum())
    assert len(np.unique(colour[keep], axis=0)) == 7  # every quad and the black between them is seen
    pin_cam = cam.with_lens(0, 0)
    pin = integrator(pin_cam, QSPP, 0).render(pin_cam, scene, want_samples=True).reshape(-1, 3)
    assert (pin != got).any(axis=1).mean() > 0.02


@pytest.mark.gpu
def test_focus_identity_and_first_hit_positions():
    """The quads IN the plane of focus (depth 3): lens and pinhole renders agree per sample outside the edge band, whatever the aperture;
    the first-hit position plane (sample_aov) is the float64 hit.  Allowance for a position: the ray's running bound carried to the plane,
    (e_o + t e_d) / cos; plus the triangle test's own: its barycentrics are quotients of edge functions x1 y2 - y1 x2 of the sheared,
    translated vertices (three roundings on products of at most 2 side^2, after two roundings of each coordinate: 20 * 2^-24 side^2
    against a determinant of side^2 cos), so each moves by at most 4 * 20 * 2^-24 / cos and the point by three times that times the
    diagonal: 340 * 2^-24 side / cos; plus the interpolation's gamma(7) sum |b_i p_i| <= 7 * 2^-24 * 3 max |p|.  Depth = |p - o| adds e_o."""
    z, f = -3.0, 3.0
    cam, scene = quads_scene(z)
    lens = cam.with_lens(0.3, f)
    got = integrator(lens, QSPP, 0).render(lens, scene, want_samples=True).reshape(-1, 3)
    pin = integrator(cam, QSPP, 0).render(cam, scene, want_samples=True).reshape(-1, 3)
    o, d = lens_samples64(lens)
    p64, colour, near = quad_lookup(o, d, z)
    assert near.mean() <= 0.01
    keep = ~near
    assert np.array_equal(bits(got[keep]), bits(pin[keep]))
    assert np.array_equal(got[keep].astype(np.float64), colour[keep])
    # positions and depths of the samples that hit a quad
    _, aov = integrator(lens, QSPP, 0).render_aov(lens, scene, want_samples=True)
    aov = aov.reshape(-1, A.PtrsAovSampleFloats).astype(np.float64)
    hit = keep & (colour.sum(axis=1) > 0)
    assert np.array_equal(aov[keep, 3] > 0, hit[keep])  # coverage: exactly the samples whose float64 ray hits a quad
    pf, _ = outside_pfilm(QW, QH, QSPP, "twin")
    ref = ref_lens_rays(lens, 1.0 / math.sqrt(QSPP), pf.reshape(-1, 2), outside_ulens(QW, QH, QSPP).reshape(-1, 2))
    e_o, e_d = np.linalg.norm(stack_e(ref["o"]), axis=1), np.linalg.norm(stack_e(ref["d"]), axis=1)
    cos = np.abs(d[:, 2])
    t = np.linalg.norm(p64 - o, axis=1)
    side = 2 * QUAD_HALF
    tol = (e_o + t * e_d) / cos + 340 * EPS * side / cos + 21 * EPS * np.abs(p64).max(axis=1)
    err = np.linalg.norm(aov[:, 8:11] - p64, axis=1)
    assert (err[hit] <= tol[hit]).all(), float((err[hit] / tol[hit]).max())
    assert (tol[hit] <= 1e-4).all()
    assert (np.abs(aov[hit, 7] - t[hit]) <= tol[hit] + e_o[hit] + 4 * EPS * t[hit]).all()
    print("positions: worst error / allowance = %.3f" % float((err[hit] / tol[hit]).max()))


PARITY = {
    "cornell_depth4": lambda: ptrs.import_scene(CORNELL, (24, 16)) + (4, 4, 0.15, 6.0),
    "image_textures": lambda: sc.cornell_plus(0, (24, 16), textured=True) + (4, 3, 0.2, 5.5),
    "environment": lambda: sc.env_spheres("256x256", (24, 16)) + (4, 3, 0.1, 4.0),
    "specular_chain": lambda: sc.glass_panes_box((24, 16)) + (4, 8, 0.1, 6.0),
    "nibbles13": lambda: ptrs.import_scene(CORNELL, (32772, 2)) + (2, 2, 0.15, 6.0),  # the smallest frame whose Sobol' index needs 33 bits (test_shade_forms)
}
_parity = {}


def parity_case(name):
    """camera with its lens, scene, integrator and the host twin's per-sample radiance and statistics (made once)."""
    if name not in _parity:
        cam, scene, spp, depth, radius, focal = PARITY[name]()
        cam = cam.with_lens(radius, focal)
        integ = integrator(cam, spp, depth)
        _, samples, st = twin.TwinScene(scene).render(cam, integ.params(cam), want_samples=True)
        samples.setflags(write=False)
        _parity[name] = (cam, scene, integ, samples, st)
    return _parity[name]


def assert_same_render(integ, cam, scene, want, wst, what):
    got = integ.render(cam, scene, want_samples=True)
    st = integ.last_stats
    assert np.array_equal(bits(got), bits(want)), "%s: %d samples differ from the twin's" % (what, (bits(got) != bits(want)).any(axis=-1).sum())
    assert (st.samples, st.rays_extension, st.rays_shadow, st.rays_mis) == (wst.samples, wst.rays_extension, wst.rays_shadow, wst.rays_mis), what
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PARITY))
def test_device_equals_twin_under_a_lens(name):
    """Per-sample radiance and ray counts of the device equal the host twin's with a lens: Cornell at depth 4, image textures (the
    first vertex's differentials), an environment map (k_env_presample's window), a chain of four specular surfaces, and the
    13-nibble form of the staged Sobol' window."""
    cam, scene, integ, want, wst = parity_case(name)
    assert integ.params(cam).flags & A.FLAG_THIN_LENS
    assert_same_render(integ, cam, scene, want, wst, name)
    if name == "cornell_depth4":  # and the lens is seen: the pinhole render of the same camera differs
        pin = cam.with_lens(0, 0)
        assert not np.array_equal(bits(integrator(pin, 4, 4).render(pin, scene, want_samples=True)), bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("name,opts", [("cornell_depth4", dict(shade_lds=0)), ("cornell_depth4", dict(shade_lds=1)), ("cornell_depth4", dict(tail=0)),
                                       ("cornell_depth4", dict(tail=1)), ("cornell_depth4", dict(lanes=1)), ("cornell_depth4", dict(lanes=4)),
                                       ("image_textures", dict(shade_lds=0)), ("image_textures", dict(tail=0)),
                                       ("environment", dict(env_presample=0)), ("environment", dict(env_presample=1)), ("environment", dict(shade_lds=0))])
def test_schedules_change_no_bit_under_a_lens(name, opts):
    cam, scene, integ, want, wst = parity_case(name)
    with ptrs.options(**opts):
        assert_same_render(integ, cam, scene, want, wst, "%s %s" % (name, opts))


@pytest.mark.gpu
def test_entry_points_agree_under_a_lens():
    """Chained render_range == render; render_tiles with every tile active == render_range; render_single_pixel == that pixel's
    samples of render_samples; the planes of render_aov carry the beauty film's weights.  Cornell 24 x 16, 4 spp, depth 4, with a lens."""
    cam, scene, integ, want, wst = parity_case("cornell_depth4")
    W, H, spp = cam.film.width, cam.film.height, 4
    cam.film.clear()
    integ.render(cam, scene)
    film = cam.film.pixels.copy()
    assert film["weight"].min() > 0
    cam.film.clear()
    samples = np.zeros((H + 4, W + 4, spp, 3), np.float32)
    for b, e in ((0, 1), (1, 3), (3, 4)):
        integ.render_range(cam, scene, b, e, samples=samples)
    assert np.array_equal(cam.film.pixels.view(np.uint32), film.view(np.uint32))
    assert np.array_equal(bits(samples), bits(want))
    cam.film.clear()
    tiles = np.ones(((H + 15) // 16, (W + 15) // 16), np.uint8)
    integ.render_tiles(cam, scene, 0, spp, tiles)
    assert np.array_equal(cam.film.pixels.view(np.uint32), film.view(np.uint32))
    cam.film.clear()
    for px, py in ((-2, -2), (5, 7), (W + 1, H + 1), (11, 3)):
        got = integ.render_single_pixel(cam, (px, py), scene)
        assert np.array_equal(bits(got), bits(want[py + 2, px + 2])), (px, py)
    planes = integ.render_aov(cam, scene)
    for name in A.PtrsAovNames:
        assert np.array_equal(bits(planes[name]["weight"]), bits(film["weight"])), name


@pytest.mark.gpu
def test_closed_form_radiance_does_not_see_the_lens():
    """test_estimator_kat's emissive cube (albedo 0.8, depth 2, default roulette) through a lens: L = Le (1 + rho + rho^2) from every
    point in every direction, so the camera ray does not matter; that file's tolerance, 4 sigma_ref + 2e-4 of the value with
    sigma_ref from the oracle's (pinhole) render of the case.  At depth 0 every sample is Le exactly."""
    import test_estimator_kat as ek
    cam, scene = ek.cube_scene("a08")
    cam = cam.with_lens(0.05, 1.2)
    rho = ek.ALBEDO["a08"]
    integ = ek._integrator(cam, 0, "default")
    s0 = integ.render(cam, scene, want_samples=True)
    assert np.array_equal(s0, np.broadcast_to(ek.LE.astype(np.float32), s0.shape))
    integ = ek._integrator(cam, 2, "default")
    _, tw, tst = twin.TwinScene(scene).render(cam, integ.params(cam), want_samples=True)
    got = integ.render(cam, scene, want_samples=True)
    assert np.array_equal(bits(got), bits(tw)) and integ.last_stats.rays_extension == tst.rays_extension
    want = ek.LE * (1 + rho + rho ** 2)
    ref = ek.interior(ek.render("oracle", "cube", ("a08",), 2, "default")[0])
    sigma = ref.std(axis=0) / math.sqrt(len(ref))
    mean = ek.interior(got).mean(axis=0)
    print("lens cube: mean %s want %s sigma_ref %s" % (mean, want, sigma))
    assert np.all(np.abs(mean - want) <= 4.0 * sigma + 2e-4 * want), (mean, want, sigma)


@pytest.mark.gpu
def test_autofocus_gives_the_depth_along_the_view_axis():
    """ptrs_camera_focus_distance on the quads' plane: the depth is the plane's, 4, for every raster point that shows a quad, however
    oblique its ray.  Allowance: t comes out of the triangle test as a quotient of a three-term sum of products by the determinant
    (16 roundings allowed), is off by e_d tan(angle) for the direction's bound, and is multiplied by -dir.z (its bound, one rounding).
    A ray between or beside the quads gives +inf."""
    cam, scene = quads_scene(-4.0)
    pts = np.array([[12.0, 5.0], [4.3, 3.1], [19.5, 12.7], [12.5, 11.2], [6.2, 12.9]], F32)
    ref = ref_camera_rays(cam, 1.0, pts)
    dirc = b_normalize(b_camera_point(cam, pts))
    o64 = np.zeros((len(pts), 3))
    d64 = stack_v(ref["d"])
    _, colour, near = quad_lookup(o64, d64, -4.0)
    assert (colour.sum(axis=1) > 0).all() and not near.any()
    e_d = np.linalg.norm(stack_e(ref["d"]), axis=1)
    for k, (x, y) in enumerate(pts):
        got = ptrs.focus_distance(cam, scene, (x, y))
        cosv = -dirc[2].v[k]
        tan = math.sqrt(1 - cosv * cosv) / cosv
        tol = 4.0 * (16 * EPS + e_d[k] * tan + dirc[2].e[k] / cosv + EPS)
        assert abs(got - 4.0) <= tol, (x, y, got, tol)
        assert tol <= 1e-5
    assert ptrs.focus_distance(cam.with_lens(0.3, 9.0), scene, (12.0, 5.0)) == ptrs.focus_distance(cam, scene, (12.0, 5.0))  # the lens plays no part
    miss = np.array([[12.0, 8.1], [0.5, 0.5], [23.9, 8.0], [15.0, 4.0]], F32)  # between two rows of quads, beside them, between two columns
    _, colour, near = quad_lookup(np.zeros((len(miss), 3)), stack_v(ref_camera_rays(cam, 1.0, miss)["d"]), -4.0)
    assert (colour.sum(axis=1) == 0).all() and not near.any()
    for x, y in miss:
        assert ptrs.focus_distance(cam, scene, (x, y)) == math.inf, (x, y)


@pytest.mark.gpu
def test_cli_renders_depth_of_field(tmp_path):
    """ptrs_headless end to end: a thinlens scene renders through its own lens (--aperture 0 closes it: another render.png);
    --aperture with --focus_at on Cornell focuses where focus_distance says, with --aov --denoise and --target_error --adaptive
    alongside, and writes every file; an autofocus ray that hits nothing is an error."""
    importlib.import_module("pathtracer-rs_amd.build").build_host()

    def run(name, scene, *args):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([CLI, scene, "-o", str(out), "-r", "48x32", "-s", "8", "-d", "3"] + list(args), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return out, r.stderr
    xml = str(tmp_path / "thinlens.xml")
    with open(xml, "w") as f:
        f.write(SENSOR % ("thinlens", LENS_FLOATS))
    own, _ = run("own", xml)  # (its emissive card stands well in front of the plane in focus)
    closed, _ = run("closed", xml, "--aperture", "0")
    png = lambda d: open(str(d / "render.png"), "rb").read()
    assert png(own) != png(closed)
    full, log = run("full", CORNELL, "--aperture", "0.2", "--focus_at", "24,16", "--aov", "--denoise", "--target_error", "0.05", "--min_samples", "4", "--adaptive")
    focus = float(log.split("INFO focus distance ")[1].split()[0])
    cam, scene = ptrs.import_scene(CORNELL, (48, 32))
    assert abs(focus - ptrs.focus_distance(cam, scene, (24.0, 16.0))) <= 1e-5 * focus  # (printed with six digits)
    for name in ("render.png", "albedo.png", "normal.png", "depth.png", "denoised.png", "samples.png"):
        assert (full / name).stat().st_size > 0, name
    r = subprocess.run([CLI, CORNELL, "-o", str(tmp_path), "-r", "48x32", "--aperture", "0.2", "--focus_at", "-40,-40"], capture_output=True, text=True)
    assert r.returncode == 1 and "hits nothing" in r.stderr, r.stderr
    # the Python host renders the imported lens too
    cl, sl = ptrs.import_scene(xml, (48, 32))
    cp = cl.with_lens(0, 0)
    a = integrator(cl, 4, 2).render(cl, sl, want_samples=True)
    b = integrator(cp, 4, 2).render(cp, sl, want_samples=True)
    assert np.isfinite(a).all() and not np.array_equal(bits(a), bits(b))


@pytest.mark.gpu
def test_shade_table_probe_has_no_lens():
    """ptrs_probe_shade_tables takes parameters and no camera: with the lens flag in them it reports the pinhole's staged window (top
    12 + 8 it), not whatever lies behind a camera it never got."""
    cam, scene = ptrs.import_scene(CORNELL, (24, 16))
    row = np.array([[0, 0, 0, 1, 2, 0, 0, 0, 0, 0, 0, 0]], np.uint32)
    for it in (0, 1, 4):
        heads = [ptrs.probe_shade_tables(scene, integrator(c, 4, 12).params(c), it, A.PROBE_SHADE_SOBOL, row)[0] for c in (cam, cam.with_lens(0.2, 5.0))]
        assert heads[0] == heads[1] and (heads[0]["sob_lo"], heads[0]["sob_n"]) == sc.window_expected(heads[0]["sob_nib"], it)


def textured_case():
    cam, scene = sc.cornell_plus(0, (24, 16), textured=True)
    return cam, scene, 4


def test_lens_aov_twin_without_a_lens_is_the_aov_twin():
    """The lens twin's AOV chain (aov_item handed the generated ray, as k_aov hands it) at radius 0 gives the rows of tests/aov_twin,
    which calls aov_item without a ray: the new argument changes nothing for a pinhole.  Image-textured Cornell, so the albedo reads the
    differentials."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "aov_twin"))
    import aov_twin
    cam, scene, spp = textured_case()
    pf, _ = outside_pfilm(24, 16, spp, "twin")
    pf = pf.reshape(-1, 2)
    ul = outside_ulens(24, 16, spp).reshape(-1, 2)
    ds = 1.0 / math.sqrt(spp)
    a = lens_twin.aov_rows(scene, cam, ds, pf, ul)
    b = aov_twin.aov_rows(scene, cam, ds, pf)
    assert np.array_equal(bits(a), bits(b))
    assert len(np.unique(bits(a[:, 0:3]), axis=0)) > 50  # the image texture is seen: many albedos
    c = lens_twin.aov_rows(scene, cam.with_lens(0.2, 5.5), ds, pf, ul)
    assert not np.array_equal(bits(c[:, 0:3]), bits(a[:, 0:3]))


@pytest.mark.gpu
def test_device_aov_samples_equal_the_lens_twin():
    """k_aov under a lens on the image-textured Cornell: every sample's 12 floats (albedo through the texture lookup with
    first_vertex_ray's differentials, coverage, normal, depth, position, triangle) equal the lens twin's chain at the outside
    (p_film, u_lens), bit for bit."""
    cam, scene, spp = textured_case()
    cam = cam.with_lens(0.2, 5.5)
    pf, _ = outside_pfilm(24, 16, spp, "twin")
    want = lens_twin.aov_rows(scene, cam, 1.0 / math.sqrt(spp), pf.reshape(-1, 2), outside_ulens(24, 16, spp).reshape(-1, 2))
    _, samples = integrator(cam, spp, 3).render_aov(cam, scene, want_samples=True)
    rows = samples.reshape(-1, 12)
    bad = (bits(rows) != bits(want)).any(axis=1)
    assert not bad.any(), "%d samples differ from the lens twin, first %r vs %r" % (bad.sum(), rows[bad][0], want[bad][0])
    assert (rows[:, 3] > 0).mean() > 0.4  # (the open box fills about six tenths of the inner sample rows)
