"""Scenes at the legal edges of a description (include/ptrs.h above ptrs_scene_create), shared by tests/test_scene_desc.py and
tests/test_scene_edges.py: the base of tests/cpp/scene_desc_cases.cpp rebuilt in Python, and the cases that are rendered -- a scene
without geometry, meshes without triangles, one triangle behind a pre-built tree whose root is a leaf, the base scaled by 2^60."""
import importlib

import numpy as np

ptrs = importlib.import_module("pathtracer-rs_amd")
A = importlib.import_module("pathtracer-rs_amd.abi")
tx = importlib.import_module("pathtracer-rs_amd.textures")
RenderScene = importlib.import_module("pathtracer-rs_amd.scene").RenderScene

F32 = np.float32
FILM = (24, 16)
SPP, DEPTH = 4, 3
BVH_DTYPE = np.dtype([("p_min", "<f4", 3), ("p_max", "<f4", 3), ("offset", "<u4"), ("num_prims", "<u2"), ("axis", "u1"), ("pad", "u1")])


def quad(x, y, z, w):
    pos = np.array([[x, y, z], [x + w, y, z], [x + w, y + w, z], [x, y + w, z]], F32)
    return pos, np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


def camera(scale=1.0):
    s = float(scale)
    return ptrs.look_at_camera([0.25 * s, 0.2 * s, 1.0 * s], [0.25 * s, 0.25 * s, 0.0], [0, 1, 0], 30.0, FILM)


def env_map(cols, rows, bright=(3, 2)):
    """A dim map with ONE bright texel (row, column; the camera looks down -z, at the map's last row) -- values small enough that a binary32
    error of the lookup position, a few 1e-7 of the map, times the map's steepest slope stays well inside the image-texture bound of
    tests/test_surface_kat.py."""
    img = np.full((rows, cols, 3), 0.25, F32) * np.array([1.0, 0.75, 0.5], F32)
    img[bright] = np.array([2.0, 1.75, 1.5], F32)
    return img


def base_scene(scale=1.0, zero_mesh_first=False):
    """Two meshes (4 + 2 triangles, every coordinate a multiple of 1/8 in [0, 1/2]), the six material kinds and a NORMAL wrapper, a constant,
    a checker and an image texture, an area light, a point light and a 4 x 2 environment light.  scale: every position times it."""
    s = RenderScene()
    rgb, f = s.const_rgb([0.75, 0.5, 0.25]), s.const_f(0.5)
    check = s.add_texture(kind=A.TEX_CHECKER, channels=3, value=[0.75, 0.375, 0.1875], value2=0.125, su=2.0, sv=2.0)
    img = s.add_texture(kind=A.TEX_IMAGE, channels=3, wrap=A.WRAP_REPEAT, su=2.0, sv=2.0,
                        levels=[(np.arange(24, dtype=F32) % 7 * F32(0.125)).reshape(2, 4, 3), np.full((1, 2, 3), 0.25, F32)])
    s.add_material(A.MAT_MATTE, [rgb])
    s.add_material(A.MAT_METAL, [rgb, rgb, rgb, f])
    s.add_material(A.MAT_MIRROR)
    s.add_material(A.MAT_GLASS, [rgb, rgb, f])
    disney = s.add_material(A.MAT_DISNEY, [check, f, f, f])
    s.add_material(A.MAT_SUBSTRATE, [rgb, rgb, f, f])
    normal = s.add_material(A.MAT_NORMAL, [img], inner=0)
    k = F32(scale)
    if zero_mesh_first:
        s.add_mesh(np.zeros((0, 3), F32), np.zeros((0, 3), np.uint32), 0)
    pa, ia = quad(0.0, 0.0, 0.0, 0.25)
    pb, ib = quad(0.25, 0.25, 0.5, 0.25)
    s.add_mesh(np.concatenate([pa, pb]) * k, np.concatenate([ia, ib + 4]), normal)
    pc, ic = quad(0.0, 0.375, 0.25, 0.125)
    m1 = s.add_mesh(pc * k, ic, disney)
    s.lights.append(dict(kind=A.LIGHT_AREA, mesh=m1, tri=0, ke_tex=rgb))
    s.add_point_light(np.array([0.25, 0.25, 0.375], F32) * k, [1.0, 1.0, 1.0])
    tx.add_infinite_light(s, env_map(4, 2, (0, 1)))
    return camera(scale), s


def env_only():
    """(a) no mesh, one 8 x 4 environment light with one bright texel; the light's record names the world sphere itself."""
    s = RenderScene()
    tx.add_infinite_light(s, env_map(8, 4))
    s.lights[-1].update(world_center=[0.0, 0.0, 0.0], world_radius=1.0)
    return camera(), s


def nothing():
    """(b) no mesh and no light."""
    return camera(), RenderScene()


def zero_meshes_point_light():
    """(c) only meshes without triangles -- one without vertices, one with vertices nothing refers to -- and a point light."""
    s = RenderScene()
    m = s.add_material(A.MAT_MATTE, [s.const_rgb([0.5, 0.5, 0.5])])
    s.add_mesh(np.zeros((0, 3), F32), np.zeros((0, 3), np.uint32), m)
    s.add_mesh(quad(0.0, 0.0, 0.0, 0.25)[0], np.zeros((0, 3), np.uint32), m)
    s.add_point_light([0.25, 0.25, 0.5], [1.0, 1.0, 1.0])
    return camera(), s


def one_triangle():
    """(e) one triangle and a point light; one_triangle_tree() is its pre-built tree: a root that is a leaf."""
    s = RenderScene()
    m = s.add_material(A.MAT_MATTE, [s.const_rgb([0.75, 0.5, 0.25])])
    s.add_mesh(np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.125]], F32), np.array([[0, 1, 2]], np.uint32), m)
    s.add_point_light([0.25, 0.25, 0.5], [1.0, 1.0, 1.0])
    return camera(), s


def one_triangle_tree():
    nodes = np.zeros(1, BVH_DTYPE)
    nodes[0]["p_max"] = [0.5, 0.5, 0.125]
    nodes[0]["num_prims"] = 1
    return nodes, np.zeros(1, np.uint32)


# name -> (builder, pre-built tree or None, the scene has no triangle)
CASES = {
    "a_env_only": (env_only, None, True),
    "b_nothing": (nothing, None, True),
    "c_zero_triangle_meshes": (zero_meshes_point_light, None, True),
    "d_zero_triangle_mesh_first": (lambda: base_scene(zero_mesh_first=True), None, False),
    "e_one_triangle_root_leaf": (one_triangle, one_triangle_tree, False),
    "f_scaled_2^60": (lambda: base_scene(scale=2.0 ** 60), None, False),
}
EMPTY = [n for n, c in CASES.items() if c[2]]


def fixed_rays(scale=1.0):
    """64 fixed rays: axis-parallel ones (infinite reciprocals, a negative zero), rays with a finite t_max, and rays aimed at the base's three quads from
    origins around them."""
    rng = np.random.default_rng(11)
    o = rng.uniform(-1.0, 1.0, (64, 3)).astype(F32)
    d = rng.normal(size=(64, 3)).astype(F32)
    for k in range(6):
        d[k] = 0.0
        d[k, k % 3] = 1.0 if k < 3 else -1.0
    d[6] = [0.0, -0.0, -1.0]
    d[7] = [0.0, 0.0, -1.0]
    o[:8] = [0.125, 0.125, 1.0]
    for k, (x, y, z, w) in enumerate(((0.0, 0.0, 0.0, 0.25), (0.25, 0.25, 0.5, 0.25), (0.0, 0.375, 0.25, 0.125))):  # 16 rays at each of the base's quads
        target = np.array([x, y, z], F32) + rng.uniform(0.0, w, (16, 3)).astype(F32) * np.array([1, 1, 0], F32)
        d[16 + 16 * k:32 + 16 * k] = target - o[16 + 16 * k:32 + 16 * k]
    t = np.full((64, 1), np.inf, F32)
    t[8:24] = 0.5
    return np.concatenate([o * F32(scale), d, t * F32(scale)], axis=1).astype(F32)
