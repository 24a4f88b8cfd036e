"""Scenes and references of tests/test_shade_tables.py and tests/test_shade_forms.py: one scene on each side of every capacity edge
of the shade stage's staged tables (triangle records, light records, the environment light's marginal tables, the Sobol' window),
the material zoo under each of the shade kernels' four feature sets, and the Sobol' value from the generator matrices."""
import importlib
import math
import os

import numpy as np

from conftest import CORNELL, ROOT

ptrs = importlib.import_module("pathtracer-rs_amd")
scenes = importlib.import_module("pathtracer-rs_amd.scenes")
tx = importlib.import_module("pathtracer-rs_amd.textures")
A = ptrs.abi

# what ptrs_hip.hip stages per workgroup (the tests sit on both sides of each)
SH_LIGHTS, SH_TRIS, SH_MARG_N, SH_SOB_WORDS = 16, 39, 1024, 3200
ONE_MINUS_EPS = np.float32(1.0) - np.float32(2.0 ** -24)


# ---- Sobol' values from the generator matrices -----------------------------------------------------------------------------------
def sobol_matrices():
    raw = open(os.path.join(ROOT, "data", "sobol_tables.bin"), "rb").read()
    assert raw[:8] == b"PTRSSOB1"
    return np.frombuffer(raw, dtype="<u4", count=1024 * 52, offset=32).reshape(1024, 52).astype(np.int64)


def sobol_reference(mats, index, scramble, dims):
    """min(1 - eps, float32(v) * 2^-32), v = scramble ^ XOR of the matrix columns of dimension `dim` at the set bits of `index`, in
    integers from the matrices alone.  index: (n,) below 2^52, scramble: (n,), dims: (n, k) -> (n, k) binary32."""
    index = np.asarray(index, np.int64)
    dims = np.asarray(dims, np.int64)
    v = np.broadcast_to(np.asarray(scramble, np.int64)[:, None], dims.shape).copy()
    for c in range(52):
        bit = ((index >> c) & 1).astype(bool)
        if bit.any():
            v ^= np.where(bit[:, None], mats[dims, c], 0)
    assert (v >= 0).all() and (v < (1 << 32)).all()
    f = v.astype(np.float32)  # int64 -> binary32 rounds to nearest even, exactly like the uint32 conversion
    return np.minimum(f * np.float32(2.0 ** -32), ONE_MINUS_EPS).astype(np.float32)


def cantor_scramble(px, py):
    """The pixel's scramble word (sobol.rs:84-90): the low 32 bits of the Cantor pairing of the offset pixel."""
    a, b = np.asarray(px, np.int64) + 1073741823, np.asarray(py, np.int64) + 1073741823
    return ((a + b) * (a + b + 1) // 2 + b) & 0xFFFFFFFF


def sobol_route(h, index, dims, n):
    """The route ShadeCtxLds::sobol must take for each row, from the configuration the probe returned."""
    index, dims = np.asarray(index, np.uint64), np.asarray(dims, np.int64)
    used = np.arange(dims.shape[1])[None, :] < np.asarray(n)[:, None]
    staged = np.full(len(index), h["sob_nib"] >= 13) | (((index >> np.uint64(32)) == 0) & (h["sob_nib"] >= 8))
    inside = ((dims >= h["sob_lo"]) & (dims < h["sob_lo"] + h["sob_n"])) | ~used
    consecutive = ((dims == dims[:, :1] + np.arange(dims.shape[1])[None, :]) | ~used).all(axis=1)
    r = np.where(staged & inside.all(axis=1), np.where(consecutive & (h["sob_nib"] == 8), A.SOB_ROUTE_RUN, A.SOB_ROUTE_LOOP), A.SOB_ROUTE_GLOBAL)
    return r.astype(np.uint32)


def window_expected(nib, it):
    """The window of round `it` by the issue's arithmetic: the top `cap` dimensions below min(1024, 12 + 8 it)."""
    cap = SH_SOB_WORDS // (16 * nib + 4)
    top = min(1024, 12 + 8 * it)
    lo = max(0, top - cap)
    return lo, top - lo


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def _drop_meshes(scene, drop):
    keep = [i for i in range(len(scene.meshes)) if i not in drop]
    new_index = {old: new for new, old in enumerate(keep)}
    scene.meshes = [scene.meshes[i] for i in keep]
    for l in scene.lights:
        if l["kind"] == A.LIGHT_AREA:
            l["mesh"] = new_index[l["mesh"]]


def _image_texture(scene, seed, shape=(12, 20), uvmap=(2.0, 2.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    return tx.spectrum_texture(scene, rng.uniform(40, 230, shape + (3,)).astype(np.uint8), uvmap=uvmap)


def _quad(scene, center, ex, ey, material, uv=True, **kw):
    c, ex, ey = (np.array(v, np.float32) for v in (center, ex, ey))
    pos = np.array([c - ex - ey, c + ex - ey, c - ex + ey, c + ex + ey], np.float32)
    n = np.cross(ex, ey)
    n = (n / np.linalg.norm(n)).astype(np.float32)
    return scene.add_mesh(pos, np.array([[0, 1, 2], [2, 1, 3]], np.uint32), material, normal=np.tile(n, (4, 1)),
                          uv=np.array([[0, 0], [1, 0], [0, 1], [1, 1]], np.float32) if uv else None, **kw)


def _env_l2w():
    cr, sr = math.cos(-math.pi / 2), math.sin(-math.pi / 2)
    rxm = np.array([[1, 0, 0, 0], [0, cr, -sr, 0], [0, sr, cr, 0], [0, 0, 0, 1]], np.float64)
    rym = np.array([[cr, 0, sr, 0], [0, 1, 0, 0], [-sr, 0, cr, 0], [0, 0, 0, 1]], np.float64)
    return (rym @ rxm @ np.diag([1.0, 1.0, -1.0, 1.0])).astype(np.float32)


ZOO_FEATS = ("simple", "img", "img_env", "full")
FEAT_OF = {"simple": A.FEAT_SIMPLE, "img": A.FEAT_IMG, "img_env": A.FEAT_IMG_ENV, "full": A.FEAT_FULL}


def open_zoo(feat, resolution=(120, 80), second_env=False):
    """scenes.material_zoo without its ceiling and back wall (environment samples connect), plus what raises the shade kernels'
    feature set: "img" one image texture on a matte card, "img_env" also the synthetic environment map, "full" also an alpha-masked
    card and a normal-mapped card.  second_env: a second, dimmer environment light with another map.  Returns cam, scene and the
    indices of the environment lights."""
    cam, s = scenes.material_zoo(resolution)
    _drop_meshes(s, (1, 2))
    env = []
    if feat != "simple":
        card = s.add_material(A.MAT_MATTE, [_image_texture(s, 31)])
        _quad(s, [2.3, 1.6, -1.0], [0.5, 0, 0.2], [0, 0.5, 0], card)
    if feat in ("img_env", "full"):
        env.append(tx.add_infinite_light(s, scenes.synthetic_env_map(), light_to_world=_env_l2w()))
        if second_env:
            env.append(tx.add_infinite_light(s, scenes.synthetic_env_map(16, 32, seed=9), light_to_world=None, scale=(0.5, 0.4, 0.3)))
    if feat == "full":
        mask = s.add_texture(kind=A.TEX_CHECKER, channels=1, value=0.0, value2=1.0, su=5.0, sv=3.0, du=0.05, dv=0.1)
        green = s.add_material(A.MAT_MATTE, [s.const_rgb([0.2, 0.7, 0.3])])
        _quad(s, [-2.3, 1.5, -0.6], [0.5, 0, -0.2], [0, 0.5, 0], green, alpha_mask_tex=mask)
        rng = np.random.default_rng(33)
        nm = np.zeros((16, 16, 3), np.uint8)
        ang, tilt = rng.uniform(0, 2 * math.pi, (16, 16)), rng.uniform(0.0, 0.5, (16, 16))
        nm[..., 0] = np.clip(127.5 * (1 + tilt * np.cos(ang)), 0, 255)
        nm[..., 1] = np.clip(127.5 * (1 + tilt * np.sin(ang)), 0, 255)
        nm[..., 2] = np.clip(127.5 * (1 + np.sqrt(1 - tilt ** 2)), 0, 255)
        inner = s.add_material(A.MAT_MATTE, [s.const_rgb([0.7, 0.7, 0.75])])
        bumpy = s.add_material(A.MAT_NORMAL, [tx.normal_map_texture(s, nm, uvmap=(3.0, 2.0, 0.0, 0.0))], inner=inner)
        _quad(s, [0.0, 2.0, -2.2], [0.8, 0, 0], [0, 0.45, 0], bumpy)
    return cam, s, env


def first_hit_kinds(cam, scene):
    """The material kinds (NormalMaterial wrappers resolved) the camera rays through the pixel centres hit first: a CPU trace."""
    import twin
    w, h = cam.film.width, cam.film.height
    x, y = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    rays = twin.camera_rays(cam, 1.0, np.stack([x.ravel(), y.ravel()], 1).astype(np.float32))
    r7 = np.concatenate([rays[:, 0:6], np.full((len(rays), 1), np.inf, np.float32)], 1)
    hits, _ = twin.TwinScene(scene).trace_rays(r7)
    mat_of_prim = np.concatenate([np.full(len(m["indices"]), m["material"]) for m in scene.meshes])
    kinds = set()
    for m in np.unique(mat_of_prim[hits["prim"][hits["prim"] >= 0]]):
        while scene.materials[m]["kind"] == A.MAT_NORMAL:
            m = scene.materials[m]["inner"]
        kinds.add(scene.materials[m]["kind"])
    return kinds


def cornell_plus(extra, resolution, textured=False):
    """Cornell (36 triangles) with `extra` small triangles floating under the ceiling, away from every surface; textured: an image
    texture on the first wall mesh (which then needs uv), so the staged records' dpdu / dpdv fields are read."""
    cam, scene = ptrs.import_scene(CORNELL, resolution)
    mat = scene.meshes[0]["material"]
    for k in range(extra):
        x = -0.55 + 0.3 * k
        pos = np.array([[x, 1.60, 0.35], [x + 0.2, 1.60, 0.35], [x + 0.2, 1.60, 0.55]], np.float32)
        scene.add_mesh(pos, np.array([[0, 1, 2]], np.uint32), mat)
    if textured:
        m = scene.meshes[0]
        n_v = len(np.asarray(m["pos"]).reshape(-1, 3))
        if m.get("uv") is None:
            p = np.asarray(m["pos"], np.float32).reshape(-1, 3)
            lo, ext = p.min(axis=0), np.maximum(p.max(axis=0) - p.min(axis=0), 1e-6)
            ax = np.argsort(ext)[1:]  # the two wide axes of the wall
            m["uv"] = ((p[:, ax] - lo[ax]) / ext[ax]).astype(np.float32)
        assert len(m["uv"]) == n_v
        m["material"] = scene.add_material(A.MAT_MATTE, [_image_texture(scene, 41, uvmap=(1.0, 1.0, 0.0, 0.0))])
    return cam, scene


def lights_floor(extra, resolution=(96, 64)):
    """A matte floor under 16 small emissive triangles (lights 0 .. 15), then `extra` as light 16: None, "area", "point" or "env"."""
    s = ptrs.RenderScene()
    grey = s.add_material(A.MAT_MATTE, [s.const_rgb([0.6, 0.6, 0.6])])
    _quad(s, [0, 0, 0], [3, 0, 0], [0, 0, -3], grey, uv=False)

    def lamp(k, rgb):
        x, z = -2.1 + 1.4 * (k % 4), -2.1 + 1.4 * (k // 4 % 4) + (0.5 if k >= 16 else 0.0)
        pos = np.array([[x, 1.2, z], [x + 0.3, 1.2, z], [x, 1.2, z + 0.3]], np.float32)  # facing down
        s.add_mesh(pos, np.array([[0, 1, 2]], np.uint32), grey, emission_rgb=rgb)
    for k in range(SH_LIGHTS):
        lamp(k, [6.0 + k, 14.0 - 0.5 * k, 5.0 + (k % 3)])
    if extra == "area":
        lamp(16, [30.0, 8.0, 4.0])
    elif extra == "point":
        s.add_point_light([0.3, 1.8, 0.4], [5.0, 4.0, 9.0])
    elif extra == "env":
        tx.add_infinite_light(s, scenes.synthetic_env_map(), light_to_world=_env_l2w())
    cam = ptrs.look_at_camera([0.0, 2.6, 5.0], [0.0, 0.3, 0.0], [0, 1, 0], 45.0, resolution)
    return cam, s


# rows x cols: nv = 2 rows = 2, 512, 1024 (the last size that is staged: maps are powers of two), 2048
ENV_SIZES = {"1x1": (1, 1), "256x256": (256, 256), "512x256": (512, 256), "1024x512": (1024, 512)}


def env_map_of(rows, cols, seed=13):
    """A seeded sky of any size (procedural: nothing is read): a vertical gradient, a cosine ripple and one bright block."""
    rng = np.random.default_rng(seed)
    v = (np.arange(rows, dtype=np.float32) + 0.5) / rows
    u = (np.arange(cols, dtype=np.float32) + 0.5) / cols
    img = (0.4 + 0.6 * (1 - v))[:, None, None] * np.array([0.6, 0.8, 1.0], np.float32)[None, None, :] * (1.0 + 0.3 * np.cos(6 * np.pi * u))[None, :, None]
    img = img * (1.0 + 0.1 * rng.uniform(-1, 1, (rows, cols, 1)))
    r0, c0 = int(0.3 * rows), int(0.6 * cols)
    img[r0:r0 + max(1, rows // 64), c0:c0 + max(1, cols // 64)] = [300.0, 260.0, 200.0]
    return img.astype(np.float32)


def env_spheres(size, resolution=(48, 32)):
    """The floor and the three spheres of scenes.textured_env (image-textured matte, Disney with a roughness texture, normal-mapped,
    glass) under an environment map of ENV_SIZES[size]; the alpha-masked cards are left out."""
    rows, cols = ENV_SIZES[size]
    cam, s = scenes.textured_env(resolution, env=env_map_of(rows, cols))
    area = sorted({l["mesh"] for l in s.lights if l["kind"] == A.LIGHT_AREA})
    s.lights = [l for l in s.lights if l["kind"] != A.LIGHT_AREA]
    _drop_meshes(s, set(range(4, len(s.meshes))) | set(area))
    for m in s.meshes:
        m["alpha_mask_tex"] = -1
    return cam, s


def glass_panes_box(resolution):
    """A matte box open towards the camera with an area light under its ceiling, seen through two parallel glass panes: every camera
    path crosses four specular surfaces before its first matte vertex."""
    s = ptrs.RenderScene()
    white = s.add_material(A.MAT_MATTE, [s.const_rgb([0.7, 0.7, 0.7])])
    red = s.add_material(A.MAT_MATTE, [s.const_rgb([0.7, 0.2, 0.2])])
    glass = s.add_material(A.MAT_GLASS, [s.const_rgb([1, 1, 1]), s.const_rgb([1, 1, 1]), s.const_f(1.5)])
    _quad(s, [0, -1, -2], [2, 0, 0], [0, 0, -2], white, uv=False)     # floor
    _quad(s, [0, 1, -2], [2, 0, 0], [0, 0, 2], white, uv=False)       # ceiling
    _quad(s, [0, 0, -4], [2, 0, 0], [0, 1, 0], white, uv=False)       # back
    _quad(s, [-2, 0, -2], [0, 0, 2], [0, 1, 0], red, uv=False)        # left
    _quad(s, [2, 0, -2], [0, 0, -2], [0, 1, 0], white, uv=False)      # right
    _quad(s, [0, 0.98, -2], [0.5, 0, 0], [0, 0, 0.5], white, uv=False, emission_rgb=[14.0, 13.0, 11.0])
    for z0 in (1.0, 0.4):  # two slabs, 0.1 thick, wider than the view
        _quad(s, [0, 0, z0], [6, 0, 0], [0, 6, 0], glass, uv=False)
        _quad(s, [0, 0, z0 - 0.1], [6, 0, 0], [0, -6, 0], glass, uv=False)
    cam = ptrs.look_at_camera([0.0, 0.0, 3.0], [0.0, 0.0, -2.0], [0, 1, 0], 40.0, resolution)
    return cam, s
