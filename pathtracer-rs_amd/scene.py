"""Host-side mirror of the reference's scene / camera construction for the render() hot path.

Mirrors (reference file:line, relative to /root/reference):
  * common/importer/mod.rs:6-25            import(path, resolution)           -> import_scene
  * common/importer/mitsuba.rs:20-151      gen_rectangle / gen_cube / gen_sphere (genmesh 0.6.2 Plane/Cube/SphereUv), load_obj
  * common/importer/mitsuba.rs:685-710     get_camera
  * common/mod.rs:33-62                    Camera::new
  * pathtracer/importer/mitsuba.rs:24-428  texture_from_mitsuba / material_from_bsdf / parse_shape / RenderScene::from_mitsuba
  * common/film.rs:132-185                 Film (resolution, sample bounds)
Every Mitsuba construct the reference's importer accepts is parsed: rectangle / cube / sphere / obj
shapes, twosided / diffuse / conductor / roughconductor / dielectric / plastic / roughplastic bsdfs
with rgb or texture (checkerboard, bitmap) parameters, area emitters on shapes, envmap / sunsky
emitters, the perspective sensor.  Everything here is host-side set-up that the
reference also does once, outside PathIntegrator::render; the results cross the C ABI as flat
arrays (include/ptrs.h).  All arithmetic is binary32 in the order nalgebra 0.32.2 performs it.
"""
import copy
import math
import os
import warnings
import xml.etree.ElementTree as ET

import numpy as np

from . import abi

F = np.float32


def _mat4(values):
    return np.array(values, dtype=np.float32).reshape(4, 4)


def transform_point(m, p):
    """nalgebra Transform * Point for a matrix whose last row is (0,0,0,1)."""
    x, y, z = F(p[0]), F(p[1]), F(p[2])
    return np.array([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], dtype=np.float32)


def transform_vector(m, v):
    x, y, z = F(v[0]), F(v[1]), F(v[2])
    return np.array([(m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z for r in range(3)], dtype=np.float32)


# ---- genmesh 0.6.2 generators (restated from memory: UNVERIFIED) -------------------
def gen_rectangle():
    """Plane::new(): 4 shared vertices (+-1,+-1,0), normal +z, one quad (0,1,3,2) triangulated as
    (0,1,3),(0,3,2)  (common/importer/mitsuba.rs:20-38)."""
    pos = np.array([[-1, -1, 0], [1, -1, 0], [-1, 1, 0], [1, 1, 0]], dtype=np.float32)
    normal = np.tile(np.array([0, 0, 1], dtype=np.float32), (4, 1))
    indices = np.array([[0, 1, 3], [0, 3, 2]], dtype=np.uint32)
    return pos, normal, indices


_CUBE_FACES = [
    ((1, 0, 0), (0b110, 0b111, 0b101, 0b100)),
    ((-1, 0, 0), (0b000, 0b001, 0b011, 0b010)),
    ((0, 1, 0), (0b011, 0b111, 0b110, 0b010)),
    ((0, -1, 0), (0b100, 0b101, 0b001, 0b000)),
    ((0, 0, 1), (0b101, 0b111, 0b011, 0b001)),
    ((0, 0, -1), (0b000, 0b010, 0b110, 0b100)),
]


def gen_cube():
    """Cube::new(): 6 faces x 4 vertices on +-1 with per-face normals, quads (4f,4f+1,4f+2,4f+3)
    triangulated as (x,y,z),(x,z,w)  (common/importer/mitsuba.rs:40-58)."""
    pos, normal, indices = [], [], []
    for f, (n, quad) in enumerate(_CUBE_FACES):
        for vid in quad:
            pos.append([1.0 if vid & 4 else -1.0, 1.0 if vid & 2 else -1.0, 1.0 if vid & 1 else -1.0])
            normal.append(n)
        b = 4 * f
        indices += [[b, b + 1, b + 2], [b, b + 2, b + 3]]
    return np.array(pos, dtype=np.float32), np.array(normal, dtype=np.float32), np.array(indices, dtype=np.uint32)


def gen_sphere(center, radius):
    """SphereUv::new(10, 10) under Similarity3(center, no rotation, radius)  (common/importer/mitsuba.rs:60-79):
    92 shared vertices (pole, 9 rings of 10, pole), unit vertex (cos a sin b, sin a sin b, cos b) with
    a = u/10 * pi * 2, b = v/10 * pi in binary32; 100 polygons (10 triangles, 80 quads, 10 triangles), quads
    triangulated as (x,y,z),(x,z,w).  The normal is the unit vertex: the similarity is not applied to it."""
    su = sv = 10
    pi = F(math.pi)

    def vert(u, v):
        a = (F(u) / F(su)) * pi * F(2.0)
        b = (F(v) / F(sv)) * pi
        ca, sa = F(math.cos(float(a))), F(math.sin(float(a)))
        cb, sb = F(math.cos(float(b))), F(math.sin(float(b)))
        return [ca * sb, sa * sb, cb]

    unit = [vert(0, 0)] + [vert(u, v) for v in range(1, sv) for u in range(su)] + [vert(0, sv)]

    def f(u, v):
        if v == 0:
            return 0
        if v == sv:
            return (sv - 1) * su + 1
        return (v - 1) * su + (u % su) + 1

    indices = []
    for v in range(sv):
        for u in range(su):
            if v == 0:
                indices.append([f(u, v), f(u, v + 1), f(u + 1, v + 1)])
            elif v == sv - 1:
                indices.append([f(u + 1, v + 1), f(u + 1, v), f(u, v)])
            else:
                x, y, z, w = f(u, v), f(u, v + 1), f(u + 1, v + 1), f(u + 1, v)
                indices += [[x, y, z], [x, z, w]]
    normal = np.array(unit, dtype=np.float32)
    c, r = np.array(center, dtype=np.float32), F(radius)
    pos = (normal * r + c).astype(np.float32)  # Similarity3 * Point: scale, (identity rotation), translate
    return pos, normal, np.array(indices, dtype=np.uint32)


def load_obj(path):
    """load_obj (common/importer/mitsuba.rs:81-151): the file's v / vn / vt lists in file order and its triangles.
    One object, one geometry, triangles only, normals required, and at every corner the position, normal and
    texture index are equal.  The values are parsed as binary64 and narrowed, as the reference does."""
    pos, normal, uv, indices = [], [], [], []
    n_obj = n_mtl = 0

    def fail(rule):
        raise ValueError("%s: %s" % (path, rule))

    try:
        text = open(path, "r").read()
    except OSError:
        raise ValueError("cannot open " + str(path))
    for line in text.splitlines():
        tok = line.split("#", 1)[0].split()
        if not tok:
            continue
        key, args = tok[0], tok[1:]
        try:
            if key == "v":
                if len(args) < 3:
                    fail("v needs three coordinates")
                pos.append([F(float(a)) for a in args[:3]])
            elif key == "vn":
                if len(args) < 3:
                    fail("vn needs three coordinates")
                normal.append([F(float(a)) for a in args[:3]])
            elif key == "vt":
                if len(args) < 2:
                    fail("vt needs two coordinates")
                uv.append([F(float(a)) for a in args[:2]])
            elif key == "f":
                if len(args) != 3:
                    fail("only triangle faces are supported")
                tri = []
                for a in args:
                    parts = a.split("/")
                    p = int(parts[0])
                    t = int(parts[1]) if len(parts) > 1 and parts[1] else None
                    n = int(parts[2]) if len(parts) > 2 and parts[2] else None
                    if n is None:
                        fail("faces need normals (v/vt/vn or v//vn)")
                    if p != n:
                        fail("position and normal index must be equal")
                    if t is not None and p != t:
                        fail("position and texture index must be equal")
                    tri.append(p if p > 0 else len(pos) + 1 + p)
                indices.append(tri)
            elif key == "o":
                n_obj += 1
                if n_obj > 1:
                    fail("only one object is supported")
            elif key == "usemtl":
                n_mtl += 1
                if n_mtl > 1:
                    fail("only one geometry (usemtl) per object is supported")
            elif key in ("g", "s", "mtllib"):
                pass
            else:
                fail("unsupported statement " + key)
        except ValueError as e:
            if str(e).startswith(str(path)):
                raise
            fail("malformed line: " + line.strip())
    if not indices:
        fail("no faces")
    if len(normal) != len(pos):
        fail("normal count must equal vertex count")
    if uv and len(uv) != len(pos):
        fail("texture coordinate count must equal vertex count")
    idx = np.array(indices, dtype=np.int64)
    if idx.min() < 1 or idx.max() > len(pos):
        fail("face index out of range")
    return (np.array(pos, dtype=np.float32), np.array(normal, dtype=np.float32),
            np.array(uv, dtype=np.float32) if uv else None, (idx - 1).astype(np.uint32))


# ---- camera ---------------------------------------------------------------------------------------
def _quat_from_rotation_matrix(r):
    """nalgebra UnitQuaternion::from_rotation_matrix; returns (i, j, k, w)."""
    tr = (r[0, 0] + r[1, 1]) + r[2, 2]
    q = F(0.25)
    if tr > 0:
        denom = np.sqrt(tr + F(1)) * F(2)
        w, i, j, k = q * denom, (r[2, 1] - r[1, 2]) / denom, (r[0, 2] - r[2, 0]) / denom, (r[1, 0] - r[0, 1]) / denom
    elif r[0, 0] > r[1, 1] and r[0, 0] > r[2, 2]:
        denom = np.sqrt(((F(1) + r[0, 0]) - r[1, 1]) - r[2, 2]) * F(2)
        w, i, j, k = (r[2, 1] - r[1, 2]) / denom, q * denom, (r[0, 1] + r[1, 0]) / denom, (r[0, 2] + r[2, 0]) / denom
    elif r[1, 1] > r[2, 2]:
        denom = np.sqrt(((F(1) + r[1, 1]) - r[0, 0]) - r[2, 2]) * F(2)
        w, i, j, k = (r[0, 2] - r[2, 0]) / denom, (r[0, 1] + r[1, 0]) / denom, q * denom, (r[1, 2] + r[2, 1]) / denom
    else:
        denom = np.sqrt(((F(1) + r[2, 2]) - r[0, 0]) - r[1, 1]) * F(2)
        w, i, j, k = (r[1, 0] - r[0, 1]) / denom, (r[0, 2] + r[2, 0]) / denom, (r[1, 2] + r[2, 1]) / denom, q * denom
    return np.array([i, j, k, w], dtype=np.float32)


def _rotation_axis_angle(axisangle):
    """nalgebra Rotation3::new(axisangle) = from_axis_angle(normalize(axisangle), |axisangle|)."""
    a = np.array(axisangle, dtype=np.float32)
    angle = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    if angle == 0:
        return np.eye(3, dtype=np.float32)
    ux, uy, uz = a / angle
    s, c = F(math.sin(float(angle))), F(math.cos(float(angle)))
    omc = F(1) - c
    sqx, sqy, sqz = ux * ux, uy * uy, uz * uz
    return np.array([
        [sqx + (F(1) - sqx) * c, ux * uy * omc - uz * s, ux * uz * omc + uy * s],
        [ux * uy * omc + uz * s, sqy + (F(1) - sqy) * c, uy * uz * omc - ux * s],
        [ux * uz * omc - uy * s, uy * uz * omc + ux * s, sqz + (F(1) - sqz) * c]], dtype=np.float32)


class Film:
    """common/film.rs:132-185 -- resolution, Gaussian(alpha=2, r=2) filter, accumulators."""

    FILTER_RADIUS = 2.0

    def __init__(self, width, height):
        self.width, self.height = int(width), int(height)
        self.pixels = np.zeros((self.height, self.width), dtype=abi.FILM_DTYPE)

    def clear(self):  # film.rs:164-172
        self.pixels[...] = 0

    def get_sample_bounds(self):  # film.rs:174-185 -> (min_x, min_y, max_x, max_y)
        r = self.FILTER_RADIUS
        return (math.floor(0.5 - r), math.floor(0.5 - r), math.ceil(self.width - 0.5 + r), math.ceil(self.height - 0.5 + r))

    def to_rgb(self):  # film.rs:253-271 (to_channel_updates): rgb / weight
        w = self.pixels["weight"][..., None]
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.pixels["rgb"] * (np.float32(1.0) / w)


class Camera:
    """common/mod.rs:20-62.  cam_to_world is an Isometry3 (unit quaternion i,j,k,w + translation)."""

    def __init__(self, rot_quat, trans, aspect, fovy, znear, zfar, resolution):
        w, h = F(resolution[0]), F(resolution[1])
        self.rot = np.array(rot_quat, dtype=np.float32)
        self.trans = np.array(trans, dtype=np.float32)
        # Perspective3::new(aspect, fovy, znear, zfar)
        aspect, fovy, znear, zfar = F(aspect), F(fovy), F(znear), F(zfar)
        self.m11 = F(1) / F(math.tan(float(fovy / F(2))))
        self.m00 = self.m11 / aspect
        self.m22 = (zfar + znear) / (znear - zfar)
        self.m23 = zfar * znear * F(2) / (znear - zfar)
        # screen_to_raster = S(W,H,1) * S(1/2,-1/2,1) * T(1,-1,0); raster_to_screen = inverse
        sx, sy = w * F(0.5), h * F(-0.5)
        self.screen_to_raster = _mat4([sx, 0, 0, sx * F(1), 0, sy, 0, sy * F(-1), 0, 0, 1, 0, 0, 0, 0, 1])
        ax, by = F(1) / sx, F(1) / sy
        self.raster_to_screen = _mat4([ax, 0, 0, F(-1), 0, by, 0, F(1), 0, 0, 1, 0, 0, 0, 0, 1])
        # raster_to_camera = cam_to_screen.to_projective().inverse() * raster_to_screen, applied to
        # raster (1,0,0), (0,1,0) and the origin with the homogeneous divide (common/mod.rs:44-48)
        n = self.m22 / self.m23
        inv00, inv11 = F(1) / self.m00, F(1) / self.m11
        p0 = np.array([(inv00 * F(-1)) / n, (inv11 * F(1)) / n, F(-1) / n], dtype=np.float32)
        px = np.array([(inv00 * ax + inv00 * F(-1)) / n, (inv11 * F(1)) / n, F(-1) / n], dtype=np.float32)
        py = np.array([(inv00 * F(-1)) / n, (inv11 * by + inv11 * F(1)) / n, F(-1) / n], dtype=np.float32)
        self.dx_camera = px - p0
        self.dy_camera = py - p0
        self.film = Film(int(resolution[0]), int(resolution[1]))
        # the thin lens (PtrsCameraLens; not in the reference): radius 0 is the pinhole
        self.lens_radius, self.focal_distance = 0.0, 0.0

    def with_lens(self, lens_radius, focal_distance):
        """This camera with a thin lens of `lens_radius` focused on the plane at depth `focal_distance` along the view axis
        (focus_distance() measures one), with a cleared film of its own.  Radius 0 gives the pinhole back."""
        lens_radius, focal_distance = float(lens_radius), float(focal_distance)
        if not (0.0 <= lens_radius < math.inf) or (lens_radius > 0.0 and not (0.0 < focal_distance < math.inf)):
            raise ValueError("thin lens: lens_radius must be finite and >= 0, focal_distance finite and > 0")
        c = copy.copy(self)
        c.film = Film(self.film.width, self.film.height)
        c.lens_radius, c.focal_distance = lens_radius, (focal_distance if lens_radius > 0.0 else 0.0)
        return c

    def to_abi(self):
        """The PtrsCamera; with a lens the PtrsCameraLens that PTRS_FLAG_THIN_LENS announces (PathIntegrator.params sets the flag)."""
        if self.lens_radius > 0.0:
            cl = abi.PtrsCameraLens()
            self._fill_abi(cl.camera)
            cl.lens_radius, cl.focal_distance = self.lens_radius, self.focal_distance
            return cl
        c = abi.PtrsCamera()
        self._fill_abi(c)
        return c

    def _fill_abi(self, c):
        c.rot[:] = [float(x) for x in self.rot]
        c.trans[:] = [float(x) for x in self.trans]
        c.m00, c.m11, c.m22, c.m23 = float(self.m00), float(self.m11), float(self.m22), float(self.m23)
        c.raster_to_screen[:] = [float(x) for x in self.raster_to_screen.reshape(16)]
        c.dx_camera[:] = [float(x) for x in self.dx_camera]
        c.dy_camera[:] = [float(x) for x in self.dy_camera]


def camera_from_matrix(cam_to_world4, fov_deg, film_w, film_h, resolution):
    """get_camera, common/importer/mitsuba.rs:685-710 (Q30)."""
    fov = F(fov_deg) * F(math.pi / 180.0)  # f32::to_radians
    rot_y = _rotation_axis_angle([0.0, -math.pi, 0.0])
    m = _mat4(cam_to_world4)
    r4 = np.eye(4, dtype=np.float32)
    r4[:3, :3] = rot_y
    mm = np.zeros((4, 4), dtype=np.float32)
    for i in range(4):
        for j in range(4):
            acc = F(0)
            for k in range(4):
                acc = acc + m[i, k] * r4[k, j]
            mm[i, j] = acc
    # try_convert::<Projective3, Similarity3>: normalise the columns, mean scale forced to 1
    rot = mm[:3, :3].copy()
    for col in range(3):
        c = rot[:, col]
        nrm = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        rot[:, col] = c / nrm
    q = _quat_from_rotation_matrix(rot)
    res = (F(resolution[0]), F(resolution[1]))
    return Camera(q, mm[:3, 3], res[0] / res[1], fov * (F(film_h) / F(film_w)), 0.01, 10000.0, resolution)


def look_at_camera(eye, target, up, fovy_deg, resolution, znear=0.01, zfar=10000.0):
    """Convenience for synthetic scenes (not a reference path): right-handed look-at, -z forward."""
    eye, target, up = (np.array(v, dtype=np.float64) for v in (eye, target, up))
    f = target - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    rot = np.stack([s, u, -f], axis=1).astype(np.float32)
    res = (F(resolution[0]), F(resolution[1]))
    return Camera(_quat_from_rotation_matrix(rot), eye.astype(np.float32), res[0] / res[1], F(fovy_deg) * F(math.pi / 180.0), znear, zfar, resolution)


# ---- RenderScene ----------------------------------------------------------------------------------
class RenderScene:
    """pathtracer/mod.rs:84-107: meshes, materials, textures, lights (+ derived flat description)."""

    def __init__(self):
        self.meshes, self.materials, self.textures, self.lights = [], [], [], []
        self._holder = None

    # builders -------------------------------------------------------------------------------------
    def add_texture(self, **kw):
        self.textures.append(kw)
        return len(self.textures) - 1

    def const_rgb(self, rgb):
        return self.add_texture(kind=abi.TEX_CONSTANT, channels=3, value=np.array(rgb, dtype=np.float32))

    def const_f(self, v):
        return self.add_texture(kind=abi.TEX_CONSTANT, channels=1, value=float(v))

    def add_material(self, kind, tex=(), flags=0, inner=-1):
        self.materials.append(dict(kind=kind, tex=list(tex), flags=flags, inner=inner))
        return len(self.materials) - 1

    def add_mesh(self, pos, indices, material, normal=None, uv=None, tangent=None, emission_rgb=None, alpha_mask_tex=-1):
        """One TriangleMesh; `emission_rgb` creates one DiffuseAreaLight per triangle in triangle
        order (pathtracer/importer/mitsuba.rs:306-331)."""
        self.meshes.append(dict(pos=pos, indices=indices, material=material, normal=normal, uv=uv, tangent=tangent, alpha_mask_tex=alpha_mask_tex))
        mi = len(self.meshes) - 1
        if emission_rgb is not None:
            ke = self.const_rgb(emission_rgb)
            for t in range(len(indices)):
                self.lights.append(dict(kind=abi.LIGHT_AREA, mesh=mi, tri=t, ke_tex=ke))
        return mi

    def add_point_light(self, p, intensity):
        self.lights.append(dict(kind=abi.LIGHT_POINT, v=p, c=intensity))

    def add_directional_light(self, w_light, radiance):
        w = np.array(w_light, dtype=np.float32)
        w = w / np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        self.lights.append(dict(kind=abi.LIGHT_DIRECTIONAL, v=w, c=radiance))

    def world_bound(self):
        """The bound of the meshes that have triangles (a mesh without one contributes nothing); None for a scene without geometry."""
        boxes = [np.asarray(m["pos"], dtype=np.float32).reshape(-1, 3) for m in self.meshes if len(m["indices"])]
        if not boxes:
            return None
        lo = np.min([b.min(axis=0) for b in boxes], axis=0)
        hi = np.max([b.max(axis=0) for b in boxes], axis=0)
        return lo, hi

    def preprocess_lights(self):
        """Light::preprocess (light.rs:209-211,480-482) with Bounds3::bounding_sphere (bounds.rs:126-134).  A scene without geometry has
        no bound to derive a sphere from: its lights keep the world_center / world_radius their records carry."""
        bound = self.world_bound()
        if bound is None:
            return
        lo, hi = bound
        center = (lo + hi) * F(0.5)
        d = center - hi
        radius = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        for l in self.lights:
            if l["kind"] in (abi.LIGHT_DIRECTIONAL, abi.LIGHT_INFINITE):
                l["world_center"], l["world_radius"] = center, float(radius)

    def num_triangles(self):
        return sum(len(m["indices"]) for m in self.meshes)

    def desc(self, bvh=None):
        self.preprocess_lights()
        self._holder = abi.SceneDescHolder(self.meshes, self.materials, self.textures, self.lights, bvh)
        return self._holder.desc


def _parse_matrix(el):
    return _mat4([float(v) for v in el.get("value").split()])


def _snake(name):
    """heck SnakeCase: a word starts at an upper-case letter after a lower-case one, and at the last letter of an
    upper-case run that a lower-case letter follows (intIOR -> int_ior, diffuseReflectance -> diffuse_reflectance)."""
    out, mode = [], 0  # mode: case of the last letter seen, 1 lower, 2 upper
    for i, ch in enumerate(name):
        if ch.isupper():
            nxt = name[i + 1] if i + 1 < len(name) else ""
            if out and out[-1] != "_" and (mode == 1 or (mode == 2 and nxt.islower())):
                out.append("_")
            out.append(ch.lower())
            mode = 2
        else:
            out.append(ch)
            if ch.islower():
                mode = 1
    return "".join(out)


def _rgb_value(el):
    v = [float(x) for x in el.get("value", "").replace(",", " ").split()]
    if len(v) < 3:
        raise ValueError("rgb parameter %s needs three values" % el.get("name"))
    return v[:3]


def _texture_from_mitsuba(scene, el, base):
    """texture_from_mitsuba, pathtracer/importer/mitsuba.rs:24-67."""
    kind = el.get("type")
    if kind == "checkerboard":
        rgbs = {_snake(c.get("name")): _rgb_value(c) for c in el.findall("rgb")}
        floats = {_snake(c.get("name")): float(c.get("value")) for c in el.findall("float")}
        for name, have in (("color0", rgbs), ("color1", rgbs), ("uscale", floats), ("vscale", floats), ("uoffset", floats), ("voffset", floats)):
            if name not in have:
                raise ValueError("checkerboard texture without " + name)
        return scene.add_texture(kind=abi.TEX_CHECKER, channels=3, value=np.array(rgbs["color0"], dtype=np.float32), value2=np.array(rgbs["color1"], dtype=np.float32),
                                 su=floats["uscale"], sv=floats["vscale"], du=floats["uoffset"], dv=floats["voffset"], wrap=abi.WRAP_REPEAT, levels=[])
    if kind == "bitmap":
        from PIL import Image
        from . import textures as tx
        fn = el.find("string[@name='filename']")
        if fn is None:
            raise ValueError("bitmap texture without filename")
        path = os.path.join(base, fn.get("value"))
        try:
            img = Image.open(path)
            img.load()
        except OSError:
            raise ValueError("cannot open " + path)
        if img.mode == "P" and "transparency" not in img.info:
            img = img.convert("RGB")
        if img.mode != "RGB":
            raise ValueError("unsupported image format for texture")
        # TODO in the reference: "verify that this -1 on the v is actually a feature of mitsuba"
        return tx.spectrum_texture(scene, np.array(img, dtype=np.uint8), wrap=abi.WRAP_REPEAT, uvmap=(1.0, -1.0, 0.0, 0.0), gamma=True)
    raise ValueError("unsupported texture type " + str(kind))


def _bsdf_to_material(scene, el, base="."):
    """material_from_bsdf, pathtracer/importer/mitsuba.rs:84-181."""
    kind = el.get("type")
    rgbs = {c.get("name"): _rgb_value(c) for c in el.findall("rgb")}
    floats = {_snake(c.get("name")): float(c.get("value")) for c in el.findall("float")}
    texture = el.find("texture")

    def with_defaults(rgb):  # texture_with_defaults: texture, else rgb, else 1
        if texture is not None:
            return _texture_from_mitsuba(scene, texture, base)
        return scene.const_rgb(rgb if rgb is not None else [1, 1, 1])

    if kind == "twosided":
        if el.find("bsdf") is None:
            raise ValueError("twosided without bsdf")
        return _bsdf_to_material(scene, el.find("bsdf"), base)
    if kind == "diffuse":
        return scene.add_material(abi.MAT_MATTE, [with_defaults(rgbs.get("reflectance"))])
    if kind in ("conductor", "roughconductor"):
        mat = el.find("string[@name='material']")
        if kind == "conductor" and mat is not None:
            if mat.get("value") == "none":
                return scene.add_material(abi.MAT_MIRROR)
            raise ValueError("other material values not supported yet!")
        if "eta" not in rgbs or "k" not in rgbs:
            raise ValueError("conductor without eta/k")
        if kind == "roughconductor" and "alpha" not in floats:
            raise ValueError("roughconductor without alpha")
        alpha = 0.001 if kind == "conductor" else floats["alpha"]
        eta, k = scene.const_rgb(rgbs["eta"]), scene.const_rgb(rgbs["k"])
        r = with_defaults(rgbs.get("specularReflectance", rgbs.get("specular_reflectance")))
        return scene.add_material(abi.MAT_METAL, [eta, k, r, scene.const_f(alpha), -1, -1], flags=0)
    if kind == "dielectric":
        if "int_ior" not in floats:
            raise ValueError("dielectric without intIOR")
        return scene.add_material(abi.MAT_GLASS, [scene.const_rgb([1, 1, 1]), scene.const_rgb([1, 1, 1]), scene.const_f(floats["int_ior"])])
    if kind in ("plastic", "roughplastic"):
        if "int_ior" not in floats or (kind == "roughplastic" and "alpha" not in floats):
            raise ValueError(kind + " without intIOR / alpha")
        e = F(floats["int_ior"])
        r0 = ((e - F(1)) * (e - F(1))) / ((e + F(1)) * (e + F(1)))
        a = 0.001 if kind == "plastic" else floats["alpha"]
        kd = with_defaults(rgbs.get("diffuseReflectance", rgbs.get("diffuse_reflectance")))
        return scene.add_material(abi.MAT_SUBSTRATE, [kd, scene.const_rgb([r0] * 3), scene.const_f(a), scene.const_f(a)], flags=0)
    raise ValueError("unsupported bsdf type " + str(kind))


def matmul4(a, b):
    """4x4 product in binary32, inner index ascending from the first product (the order both hosts use)."""
    r = np.zeros((4, 4), dtype=np.float32)
    for i in range(4):
        for j in range(4):
            acc = a[i, 0] * b[0, j]
            for k in range(1, 4):
                acc = acc + a[i, k] * b[k, j]
            r[i, j] = acc
    return r


def env_light_to_world():
    """Matrix4::from_euler_angles(-pi/2, -pi/2, 0).append_nonuniform_scaling((1, 1, -1))
    (pathtracer/importer/mitsuba.rs:365-372): Rz(yaw) Ry(pitch) Rx(roll) written out as nalgebra does, then the
    ROWS scaled.  For exact angles this is [[0,1,0],[0,0,1],[-1,0,0]]."""
    h = F(-math.pi / 2)  # -f32::consts::FRAC_PI_2
    sr, cr = F(math.sin(float(h))), F(math.cos(float(h)))
    sp, cp = sr, cr
    sy, cy = F(0.0), F(1.0)
    m = np.eye(4, dtype=np.float32)
    m[0, :3] = [cy * cp, (cy * sp) * sr - sy * cr, (cy * sp) * cr + sy * sr]
    m[1, :3] = [sy * cp, (sy * sp) * sr + cy * cr, (sy * sp) * cr - cy * sr]
    m[2, :3] = [-sp, cp * sr, cp * cr]
    for r, f in enumerate((F(1.0), F(1.0), F(-1.0))):
        m[r, :] = m[r, :] * f
    return m


DEFAULT_ENV_MAP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "abandoned_tank_farm_04_1k.hdr")


def _shape_matrix(sh):
    el = sh.find("transform/matrix")
    return _parse_matrix(el) if el is not None else np.eye(4, dtype=np.float32)


def import_scene(path, resolution, default_lights=False, env_map=None):
    """common/importer/mod.rs:6-25: dispatch on the extension; returns (Camera, RenderScene).
    .gltf / .glb -> gltf.import_gltf (default_lights = the CLI's --default_lights); .xml -> Mitsuba.  For a Mitsuba
    scene `env_map` names the Radiance file a sunsky emitter falls back to (default: the bundled data/ map)."""
    ext = os.path.splitext(str(path))[1].lower()
    if ext in (".gltf", ".glb"):
        from .gltf import import_gltf
        return import_gltf(path, resolution, default_lights=default_lights, env_map=env_map)
    if ext != ".xml":
        raise ValueError("unsupported format!")
    base = os.path.dirname(str(path)) or "."
    root = ET.parse(path).getroot()
    sensor = root.find("sensor")
    fov = float(sensor.find("float[@name='fov']").get("value"))
    film = sensor.find("film")
    fw = int(film.find("integer[@name='width']").get("value"))
    fh = int(film.find("integer[@name='height']").get("value"))
    cam = camera_from_matrix(_parse_matrix(sensor.find("transform/matrix")).reshape(16), fov, fw, fh, resolution)
    if sensor.get("type") == "thinlens":  # Mitsuba's thin-lens sensor: aperture_radius, focus_distance
        ap, fd = sensor.find("float[@name='aperture_radius']"), sensor.find("float[@name='focus_distance']")
        if ap is None or fd is None:
            raise ValueError("thinlens sensor: aperture_radius and focus_distance are required")
        cam = cam.with_lens(float(ap.get("value")), float(fd.get("value")))
    scene = RenderScene()
    named = {}
    for b in root.findall("bsdf"):
        named[b.get("id")] = _bsdf_to_material(scene, b, base)
    for sh in root.findall("shape"):
        kind = sh.get("type")
        uv = None
        m = _shape_matrix(sh)
        if kind == "rectangle":
            pos, normal, indices = gen_rectangle()
        elif kind == "cube":
            pos, normal, indices = gen_cube()
        elif kind == "sphere":
            pt, rad = sh.find("point"), sh.find("float")
            if pt is None or rad is None:
                raise ValueError("sphere needs a center point and a radius")
            pos, normal, indices = gen_sphere([float(pt.get(a, "0")) for a in "xyz"], float(rad.get("value")))
            m = np.eye(4, dtype=np.float32)  # Shape::Sphere has no transform: obj_to_world stays the identity
        elif kind == "obj":
            fn = sh.find("string")
            if fn is None:
                raise ValueError("obj shape without filename")
            pos, normal, uv, indices = load_obj(os.path.join(base, fn.get("value")))
            fnrm = sh.find("boolean")
            if fnrm is not None and fnrm.get("value") == "true":
                warnings.warn("face normals on for obj, vertex normals will be disregarded")
                normal = None
        else:
            raise ValueError("unsupported shape type " + str(kind))
        wpos = np.array([transform_point(m, p) for p in pos], dtype=np.float32)
        wnrm = np.array([transform_vector(m, n) for n in normal], dtype=np.float32) if normal is not None else None  # Q15: forward matrix, no renormalise
        ref = sh.find("ref")
        if ref is not None:
            if ref.get("id") not in named:
                raise ValueError("unknown bsdf id " + str(ref.get("id")))
            mat = named[ref.get("id")]
        elif sh.find("bsdf") is not None:
            mat = _bsdf_to_material(scene, sh.find("bsdf"), base)
        else:
            raise ValueError("either ref exists or embedded bsdf exists")
        em = sh.find("emitter")
        emission = None
        if em is not None and em.get("type") == "area":
            emission = _rgb_value(em.find("rgb")) if em.find("rgb") is not None else [1.0, 1.0, 1.0]
        scene.add_mesh(wpos, indices, mat, normal=wnrm, uv=uv, emission_rgb=emission)
    # scene-level emitters join the list after every shape's area lights, in document order (mitsuba.rs:374-420)
    for em in root.findall("emitter"):
        kind = em.get("type")
        if kind == "area":
            warnings.warn("area lights should not be standalone!")
        elif kind == "point":
            pass
        elif kind == "envmap":
            from . import textures as tx
            fn, mt = em.find("string"), em.find("transform/matrix")
            if fn is None or mt is None:
                raise ValueError("envmap emitter needs a toWorld matrix and a filename")
            hdr = os.path.join(base, fn.get("value"))
            if not os.path.exists(hdr):
                raise ValueError("cannot open " + hdr)
            tx.add_infinite_light(scene, tx.read_rgbe(hdr), light_to_world=matmul4(_parse_matrix(mt), env_light_to_world()))
        elif kind == "sunsky":
            from . import textures as tx
            warnings.warn("sunsky emitter not supported, putting default env map instead")
            hdr = env_map if env_map is not None else DEFAULT_ENV_MAP
            img = tx.read_rgbe(hdr) if isinstance(hdr, (str, os.PathLike)) else np.asarray(hdr, dtype=np.float32)
            tx.add_infinite_light(scene, img, light_to_world=env_light_to_world())
        else:
            raise ValueError("unsupported emitter type " + str(kind))
    return cam, scene
