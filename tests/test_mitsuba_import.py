"""The Mitsuba importer beyond Cornell: sphere and obj shapes, checkerboard / bitmap reflectances, envmap and sunsky emitters, in the
Python host (scene.py) and the C++ host (host/ptrs_host.cpp, through ptrs_headless).

Fixtures: tests/golden/mitsuba/ (written by tests/golden/make_mitsuba_fixtures.py; all this project's own).  Tests 1-4 hold the
import against answers that do not come from the oracle: topology, float64 restatements, known texels.  Every tolerance is a rounding
bound with its derivation next to it (u = 2^-24, the unit roundoff of binary32); none is measured."""
import importlib
import math
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import twin
from conftest import ROOT
from test_host_cpp import CLI, _bits, _compare_full, _read_full_dump

FIX = os.path.join(ROOT, "tests", "golden", "mitsuba")
ALL = os.path.join(FIX, "all_features.xml")
SUNSKY = os.path.join(FIX, "sunsky.xml")
U = 2.0 ** -24
F = np.float32

# all_features.xml, in document order
MESH_FLOOR, MESH_CUBE, MESH_SPHERE, MESH_LAMP, MESH_OBJ, MESH_OBJ_FACE, MESH_WALL = range(7)
OBJ_TO_WORLD = np.array([[0.25, -0.12, 0.05, -0.15], [0.1, 0.28, 0.07, 0.95], [-0.08, 0.04, 0.29, -0.5], [0, 0, 0, 1]], np.float32)
ENV_TO_WORLD = np.array([[0.866025, 0, 0.5, 0], [0.1, 0.98, -0.173205, 0], [-0.49, 0.2, 0.848705, 0], [0, 0, 0, 1]], np.float32)

HEAD = """<?xml version="1.0" encoding="utf-8"?>
<scene version="0.5.0" >
	<sensor type="perspective" >
		<float name="fov" value="24" />
		<transform name="toWorld" ><matrix value="-1 0 0 0 0 1 0 1 0 0 -1 6.8 0 0 0 1"/></transform>
		<film type="ldrfilm" ><integer name="width" value="96" /><integer name="height" value="64" /></film>
	</sensor>
"""
GROUND = """	<shape type="rectangle" >
		<transform name="toWorld" ><matrix value="2 0 0 0 0 0 2 0 0 -2 0 0 0 0 0 1"/></transform>
		<bsdf type="diffuse" ><rgb name="reflectance" value="0.5, 0.5, 0.5"/></bsdf>
	</shape>
"""
CHECKER = """<texture type="checkerboard" name="t" >
			<rgb name="color0" value="0.75, 0.5, 0.25"/><rgb name="color1" value="0.125, 0.25, 0.5"/>
			<float name="uscale" value="1" /><float name="vscale" value="1" /><float name="uoffset" value="0" /><float name="voffset" value="0" />
		</texture>"""


@pytest.fixture(scope="module")
def cli():
    importlib.import_module("pathtracer-rs_amd.build").build_host()
    return CLI


@pytest.fixture()
def work(tmp_path):
    """A scratch copy of the fixture directory: scene files written next to it find the images, the mesh and the map."""
    d = tmp_path / "m"
    shutil.copytree(FIX, str(d))
    return d


def _write(work, name, body):
    p = str(work / name)
    with open(p, "w") as f:
        f.write(HEAD + body + "</scene>\n")
    return p


def _import(ptrs, path, res=(48, 32)):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ptrs.import_scene(path, res)


def _cli_error(cli, path, tmp):
    r = subprocess.run([cli, path, "--dump-scene-full", str(tmp / "x.dump")], capture_output=True, text=True)
    assert r.returncode == 1, "ptrs_headless must refuse %s with exit status 1, got %d: %s" % (path, r.returncode, r.stderr)
    return r.stderr


# ---- 1. sphere -------------------------------------------------------------------------------------------------------------------
def _sphere_uv(index):
    """(u, v) of shared vertex `index` of SphereUv(10, 10): pole, nine rings of ten, pole."""
    if index == 0:
        return 0, 0
    if index == 91:
        return 0, 10
    return (index - 1) % 10, (index - 1) // 10 + 1


def _unit64(u, v):
    """The unit vertex in float64.  The mesh is DEFINED with its two angles evaluated in binary32 (a = u/10 * pi * 2, b = v/10 * pi, the
    generator's own arithmetic), so the float64 answer takes those two binary32 angles as its inputs."""
    a = float((F(u) / F(10)) * F(math.pi) * F(2.0))
    b = float((F(v) / F(10)) * F(math.pi))
    return np.array([math.cos(a) * math.sin(b), math.sin(a) * math.sin(b), math.cos(b)])


@pytest.mark.parametrize("mesh,center,radius", [(MESH_SPHERE, (0.55, 0.4, 0.3), 0.4), (MESH_LAMP, (-0.1, 1.75, 0.2), 0.125)])
def test_sphere_mesh(ptrs, mesh, center, radius):
    """92 vertices, 180 triangles, a closed 2-manifold with one winding, every vertex on the sphere.
    Position bound, per coordinate: |p - (c + r u^)| <= 8 u (r + max|c|): two correctly rounded trig values, their product, the scale
    and the add are five roundings of relative size u on a value of at most r + |c| (the centre and radius enter as the binary32 values the importer parsed).
    Normal bound: 3 u (two trig values, one product; |u^| <= 1)."""
    _, scene = _import(ptrs, ALL)
    m = scene.meshes[mesh]
    pos, nrm, idx = np.asarray(m["pos"], np.float64), np.asarray(m["normal"], np.float64), np.asarray(m["indices"], np.int64)
    assert pos.shape == (92, 3) and nrm.shape == (92, 3) and idx.shape == (180, 3) and m["uv"] is None
    edges = {}
    for t in idx:
        assert len(set(t)) == 3
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            edges[(a, b)] = edges.get((a, b), 0) + 1
    assert all(n == 1 for n in edges.values()), "a directed edge is used twice"
    assert all((b, a) in edges for (a, b) in edges), "an edge has no opposite: the surface is open"
    assert 92 - len(edges) // 2 + 180 == 2
    c, r = np.array(center, np.float64), float(radius)
    tri = pos[idx]
    n_geom = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    side = ((tri.mean(axis=1) - c) * n_geom).sum(axis=1)
    assert (side > 0).all() or (side < 0).all(), "mixed winding"
    assert (side > 0).all(), "the triangles face inwards"
    c32, r32 = np.array(center, np.float32).astype(np.float64), float(F(radius))
    for i in range(92):
        uh = _unit64(*_sphere_uv(i))
        assert np.abs(pos[i] - (c32 + r32 * uh)).max() <= 8 * U * (r32 + np.abs(c32).max()), i
        assert np.abs(nrm[i] - uh).max() <= 3 * U, i
    assert scene.meshes[mesh]["material"] == (2 if mesh == MESH_SPHERE else 3)


def test_sphere_ignores_a_transform_child(ptrs, cli, work):
    shape = """	<bsdf type="diffuse" id="M" ><rgb name="reflectance" value="0.5, 0.5, 0.5"/></bsdf>
	<shape type="sphere" >
		<point name="center" x="0.3" y="0.7" z="-0.2" />
		<float name="radius" value="0.6" />%s
		<ref id="M" />
	</shape>
"""
    plain = _write(work, "plain.xml", shape % "")
    moved = _write(work, "moved.xml", shape % '\n\t\t<transform name="toWorld" ><matrix value="2 0 0 5 0 3 0 6 0 0 4 7 0 0 0 1"/></transform>')
    (_, a), (_, b) = _import(ptrs, plain), _import(ptrs, moved)
    for k in ("pos", "normal", "indices"):
        assert np.asarray(a.meshes[0][k]).tobytes() == np.asarray(b.meshes[0][k]).tobytes(), k
    dumps = []
    for p in (plain, moved):
        subprocess.check_call([cli, p, "--dump-scene-full", p + ".dump", "-r", "48x32"])
        dumps.append(open(p + ".dump", "rb").read())
    assert dumps[0] == dumps[1]


# ---- 2. obj ----------------------------------------------------------------------------------------------------------------------
def _read_obj_lists(path):
    v, vn, vt = [], [], []
    for line in open(path):
        t = line.split()
        if t and t[0] in ("v", "vn", "vt"):
            {"v": v, "vn": vn, "vt": vt}[t[0]].append([float(x) for x in t[1:]])
    return np.array(v), np.array(vn), np.array(vt)


def test_obj_mesh(ptrs):
    """File order is kept; positions are toWorld * (x, 1), normals the upper 3x3 * n without renormalising (Q15), uvs the file's own.
    Bound per coordinate: 4 u sum_j |m_ij| |x_j| -- three products and three adds of the binary32 evaluation, each at most u of a partial
    sum that the sum of magnitudes bounds (the first product's rounding is shared by the adds after it: 4 covers it)."""
    _, scene = _import(ptrs, ALL)
    v, vn, vt = _read_obj_lists(os.path.join(FIX, "mesh.obj"))
    m = scene.meshes[MESH_OBJ]
    M = OBJ_TO_WORLD.astype(np.float64)
    v32, vn32 = v.astype(np.float32).astype(np.float64), vn.astype(np.float32).astype(np.float64)
    pos, nrm = np.asarray(m["pos"], np.float64), np.asarray(m["normal"], np.float64)
    assert pos.shape == v.shape and nrm.shape == vn.shape
    want_p = v32 @ M[:3, :3].T + M[:3, 3]
    bound_p = 4 * U * (np.abs(v32) @ np.abs(M[:3, :3]).T + np.abs(M[:3, 3]))
    assert (np.abs(pos - want_p) <= bound_p).all()
    want_n = vn32 @ M[:3, :3].T
    assert (np.abs(nrm - want_n) <= 4 * U * (np.abs(vn32) @ np.abs(M[:3, :3]).T)).all()
    assert np.array_equal(_bits(m["uv"]), _bits(vt.astype(np.float32)))
    faces = [[int(c.split("/")[0]) - 1 for c in line.split()[1:]] for line in open(os.path.join(FIX, "mesh.obj")) if line.startswith("f ")]
    assert np.array_equal(np.asarray(m["indices"]), np.array(faces, np.uint32))
    face = scene.meshes[MESH_OBJ_FACE]
    assert face["normal"] is None and face["uv"] is not None and np.array_equal(np.asarray(face["indices"]), np.asarray(m["indices"]))


OBJ_OK = ["o one", "v 0 0 0", "v 1 0 0", "v 0 1 0", "v 1 1 0", "vn 0 0 1", "vn 0 0 1", "vn 0 0 1", "vn 0 0 1", "usemtl a", "f 1//1 2//2 3//3", "f 2//2 4//4 3//3"]


def _edit(lines, drop=(), replace=None, insert=None):
    out = [l for l in lines if not l.startswith(tuple(drop))] if drop else list(lines)
    if replace:
        out = [replace[1] if l == replace[0] else l for l in out]
    if insert:
        out.insert(insert[0], insert[1])
    return out


@pytest.mark.parametrize("name,lines,rule", [
    ("two_objects", _edit(OBJ_OK, insert=(9, "o two")), "only one object"),
    ("quad", _edit(OBJ_OK, replace=("f 2//2 4//4 3//3", "f 1//1 2//2 4//4 3//3")), "only triangle faces"),
    ("no_normals", _edit(OBJ_OK, drop=("vn", "f"), insert=(6, "f 1 2 3")), "faces need normals"),
    ("index_mismatch", _edit(OBJ_OK, replace=("f 2//2 4//4 3//3", "f 2//2 4//3 3//3")), "position and normal index must be equal"),
    ("two_usemtl", _edit(OBJ_OK, insert=(11, "usemtl b")), "only one geometry"),
])
def test_obj_refusals(ptrs, cli, work, name, lines, rule):
    """Each rule of load_obj is a clean error that names the file and the rule, in both hosts."""
    with open(str(work / (name + ".obj")), "w") as f:
        f.write("\n".join(lines) + "\n")
    body = """	<shape type="obj" >
		<string name="filename" value="%s.obj" />
		<transform name="toWorld" ><matrix value="1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1"/></transform>
		<bsdf type="diffuse" ><rgb name="reflectance" value="0.5, 0.5, 0.5"/></bsdf>
	</shape>
"""
    path = _write(work, name + ".xml", body % name)
    with pytest.raises(ValueError) as e:
        _import(ptrs, path)
    assert rule in str(e.value) and name + ".obj" in str(e.value)
    err = _cli_error(cli, path, work)
    assert rule in err and name + ".obj" in err
    with open(str(work / "fine.obj"), "w") as f:  # the unedited file is accepted: the edits above are what is refused
        f.write("\n".join(OBJ_OK) + "\n")
    _, scene = _import(ptrs, _write(work, "fine.xml", body % "fine"))
    assert np.asarray(scene.meshes[0]["indices"]).tolist() == [[0, 1, 2], [1, 3, 2]]


# ---- 3. textures -----------------------------------------------------------------------------------------------------------------
def test_checkerboard_record_and_lookup(ptrs, work):
    _, scene = _import(ptrs, ALL)
    mat = scene.materials[scene.meshes[MESH_CUBE]["material"]]
    assert mat["kind"] == ptrs.abi.MAT_SUBSTRATE
    t = scene.textures[mat["tex"][0]]
    assert t["kind"] == ptrs.abi.TEX_CHECKER and t["channels"] == 3
    assert np.array_equal(_bits(t["value"]), _bits([0.8, 0.1, 0.1])) and np.array_equal(_bits(t["value2"]), _bits([0.1, 0.2, 0.8]))
    assert (F(t["su"]), F(t["sv"]), F(t["du"]), F(t["dv"])) == (F(4), F(3), F(0.125), F(0.25))
    # texture.rs:81-87 at uscale = vscale = 1, no offset: the cell of uv (0.25, 0.25) is color1, the cell of (0.25, 0.75) color0
    path = _write(work, "checker.xml", '\t<bsdf type="diffuse" id="C" >\n\t\t' + CHECKER + "\n\t</bsdf>\n" + GROUND.replace("<bsdf type=\"diffuse\" ><rgb name=\"reflectance\" value=\"0.5, 0.5, 0.5\"/></bsdf>", '<ref id="C" />'))
    _, sc = _import(ptrs, path)
    tid = sc.materials[0]["tex"][0]
    out = twin.texture_probe(twin.TwinScene(sc), tid, np.array([[0.25, 0.25, 0, 0, 0, 0], [0.25, 0.75, 0, 0, 0, 0]], np.float32))
    assert np.array_equal(_bits(out[0, :3]), _bits([0.125, 0.25, 0.5])), "uv (0.25, 0.25) must give color1"
    assert np.array_equal(_bits(out[1, :3]), _bits([0.75, 0.5, 0.25])), "uv (0.25, 0.75) must give color0"


def test_bitmap_texture(ptrs, work):
    """ImageTexture::<Spectrum>::new(image, 1, Repeat, UVMap(1, -1, 0, 0), gamma): the pyramid is bitwise spectrum_texture's on the same
    pixels; the lookup at uv = (0.125, 0.125) with a zero footprint is texel (row 3, column 0) of the 4 x 4 image: st = (0.125, -0.125),
    s = 0.125 * 4 - 0.5 = 0, t = -0.125 * 4 - 0.5 = -1 -> Repeat -> row 3, both weights of the bilinear lookup exactly 1 and 0.
    Against float64: v = p/255, ((v + 0.055)/1.055)^2.4 within 9 u relative: three roundings before the power (the quotient, the sum, the
    division) that the exponent multiplies by 2.4, one rounding of the result."""
    from PIL import Image
    tx, abi = ptrs.textures, ptrs.abi
    _, scene = _import(ptrs, ALL)
    t = scene.textures[scene.materials[scene.meshes[MESH_FLOOR]["material"]]["tex"][0]]
    assert t["kind"] == abi.TEX_IMAGE and t["wrap"] == abi.WRAP_REPEAT and (t["su"], t["sv"], t["du"], t["dv"]) == (1.0, -1.0, 0.0, 0.0)
    px = np.array(Image.open(os.path.join(FIX, "tex_rgb.png")))
    assert px.shape == (20, 12, 3)
    ref = ptrs.RenderScene()
    want = ref.textures[tx.spectrum_texture(ref, px, wrap=abi.WRAP_REPEAT, uvmap=(1, -1, 0, 0), gamma=True)]["levels"]
    assert len(t["levels"]) == len(want) == 6 and t["levels"][0].shape == (32, 16, 3)  # resampled to powers of two
    for a, b in zip(t["levels"], want):
        assert np.array_equal(_bits(a), _bits(b))
    t4 = scene.materials[scene.meshes[MESH_OBJ]["material"]]["tex"][0]
    p4 = np.array(Image.open(os.path.join(FIX, "tex_4x4.png")))
    assert len({tuple(p) for p in p4.reshape(-1, 3)}) == 16
    out = twin.texture_probe(twin.TwinScene(scene), t4, np.array([[0.125, 0.125, 0, 0, 0, 0]], np.float32))
    want = tx.inverse_gamma_correct(p4[3, 0].astype(np.float32) / F(255.0))
    assert np.array_equal(_bits(out[0, :3]), _bits(want))
    v = p4[3, 0].astype(np.float64) / 255.0
    exact = np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
    assert (np.abs(out[0, :3] - exact) <= 9 * U * exact).all()


BSDFS = {
    "diffuse": ('<bsdf type="diffuse" id="B" ><rgb name="reflectance" value="0.2, 0.2, 0.2"/>%s</bsdf>', 0),
    "conductor": ('<bsdf type="conductor" id="B" ><rgb name="eta" value="0.2, 0.9, 1.1"/><rgb name="k" value="3.9, 2.4, 2.1"/><rgb name="specularReflectance" value="0.2, 0.2, 0.2"/>%s</bsdf>', 2),
    "roughconductor": ('<bsdf type="roughconductor" id="B" ><float name="alpha" value="0.2" /><rgb name="eta" value="0.2, 0.9, 1.1"/><rgb name="k" value="3.9, 2.4, 2.1"/><rgb name="specularReflectance" value="0.2, 0.2, 0.2"/>%s</bsdf>', 2),
    "plastic": ('<bsdf type="plastic" id="B" ><float name="intIOR" value="1.5" /><rgb name="diffuseReflectance" value="0.2, 0.2, 0.2"/>%s</bsdf>', 0),
    "roughplastic": ('<bsdf type="roughplastic" id="B" ><float name="intIOR" value="1.5" /><float name="alpha" value="0.2" /><rgb name="diffuseReflectance" value="0.2, 0.2, 0.2"/>%s</bsdf>', 0),
}


@pytest.mark.parametrize("kind", sorted(BSDFS))
@pytest.mark.parametrize("form", ["named", "twosided", "embedded"])
def test_texture_beats_rgb(ptrs, work, kind, form):
    """texture_with_defaults: a texture child wins over the rgb parameter (which wins over 1) -- named, through twosided, embedded."""
    abi = ptrs.abi
    xml, slot = BSDFS[kind]
    shape = GROUND.replace("<bsdf type=\"diffuse\" ><rgb name=\"reflectance\" value=\"0.5, 0.5, 0.5\"/></bsdf>", "%s")
    for tex, want_kind in ((CHECKER, abi.TEX_CHECKER), ("", abi.TEX_CONSTANT)):
        b = xml % tex
        if form == "named":
            body = "\t" + b + "\n" + shape % '<ref id="B" />'
        elif form == "twosided":
            body = '\t<bsdf type="twosided" id="B" >' + b.replace(' id="B"', "") + "</bsdf>\n" + shape % '<ref id="B" />'
        else:
            body = shape % b.replace(' id="B"', "")
        _, scene = _import(ptrs, _write(work, "b.xml", body))
        t = scene.textures[scene.materials[scene.meshes[0]["material"]]["tex"][slot]]
        assert t["kind"] == want_kind
        if want_kind == abi.TEX_CONSTANT:
            assert np.array_equal(_bits(t["value"]), _bits([0.2, 0.2, 0.2]))
        else:
            assert np.array_equal(_bits(t["value"]), _bits([0.75, 0.5, 0.25]))


def test_texture_refusals(ptrs, cli, work):
    shape = GROUND.replace("<bsdf type=\"diffuse\" ><rgb name=\"reflectance\" value=\"0.5, 0.5, 0.5\"/></bsdf>", "%s")
    rgba = _write(work, "rgba.xml", shape % '<bsdf type="diffuse" ><texture type="bitmap" name="reflectance" ><string name="filename" value="tex_rgba.png" /></texture></bsdf>')
    with pytest.raises(ValueError, match="unsupported image format for texture"):
        _import(ptrs, rgba)
    assert "unsupported image format for texture" in _cli_error(cli, rgba, work)
    for missing in ("color0", "color1", "uscale", "vscale", "uoffset", "voffset"):
        kept = "".join(l for l in CHECKER.replace("/><", "/>\n<").splitlines(True) if 'name="%s"' % missing not in l)
        assert kept != CHECKER.replace("/><", "/>\n<")
        p = _write(work, "missing.xml", shape % ('<bsdf type="diffuse" >' + kept + "</bsdf>"))
        with pytest.raises(ValueError, match=missing):
            _import(ptrs, p)
        assert missing in _cli_error(cli, p, work)


# ---- 4. emitters -----------------------------------------------------------------------------------------------------------------
def _env_64():
    """E = diag(1, 1, -1) Ry(-pi/2) Rx(-pi/2) in float64 at the binary32 angle the reference passes (-FRAC_PI_2 as f32)."""
    h = float(F(-math.pi / 2))
    c, s = math.cos(h), math.sin(h)
    rx = np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1]])
    ry = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]])
    return np.diag([1.0, 1.0, -1.0, 1.0]) @ ry @ rx


def test_light_order_and_env_matrix(ptrs, work):
    """Area lights of the shapes in document / triangle order, then the scene-level emitters.
    light_to_world = toWorld * E.  With toWorld = I it is within 4 u of the signed permutation [[0,1,0],[0,0,1],[-1,0,0]] (its value for
    exact angles; the binary32 cos(pi/2) is 4.4e-8 = 0.73 u and the products with 0 and 1 are exact).  With the fixture's toWorld it is
    within 8 u sum_k |a_ik| |b_kj| of the float64 product: an entry of E carries at most three roundings (a trig value, two products;
    its sums add exact zeros), the 4-term product one per product and one per add -- seven.  world_to_light is the float64 inverse
    rounded once, so its float64 product with light_to_world is the identity within the same bound (one rounding per factor)."""
    abi = ptrs.abi
    _, scene = _import(ptrs, ALL)
    assert len(scene.lights) == 181
    for t, l in enumerate(scene.lights[:180]):
        assert (l["kind"], l["mesh"], l["tri"]) == (abi.LIGHT_AREA, MESH_LAMP, t)
    ke = scene.textures[scene.lights[0]["ke_tex"]]
    assert np.array_equal(_bits(ke["value"]), _bits([9, 8, 6])) and all(l["ke_tex"] == scene.lights[0]["ke_tex"] for l in scene.lights[:180])
    env = scene.lights[180]
    assert env["kind"] == abi.LIGHT_INFINITE and (env["dist"]["nu"], env["dist"]["nv"]) == (32, 16)
    assert np.array_equal(_bits(scene.textures[env["lmap_tex"]]["levels"][0]), _bits(ptrs.textures.read_rgbe(os.path.join(FIX, "env_16x8.hdr"))))
    A, E = ENV_TO_WORLD.astype(np.float64), _env_64()
    l2w, w2l = np.asarray(env["light_to_world"], np.float64), np.asarray(env["world_to_light"], np.float64)
    assert (np.abs(l2w - A @ E) <= 8 * U * (np.abs(A) @ np.abs(E))).all()
    assert (np.abs(w2l @ l2w - np.eye(4)) <= 8 * U * (np.abs(w2l) @ np.abs(l2w))).all()
    ident = _write(work, "ident.xml", GROUND + '\t<emitter type="envmap" >\n\t\t<transform name="toWorld" ><matrix value="1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1"/></transform>\n\t\t<string name="filename" value="env_16x8.hdr" />\n\t</emitter>\n')
    _, sc = _import(ptrs, ident)
    assert len(sc.lights) == 1
    m = np.asarray(sc.lights[0]["light_to_world"], np.float64)
    perm = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [-1, 0, 0, 0], [0, 0, 0, 1]], np.float64)
    assert (np.abs(m - perm) <= 4 * U).all()


def test_sunsky_falls_back_to_the_bundled_map(ptrs):
    """sunsky: a warning, then data/abandoned_tank_farm_04_1k.hdr under E alone.  The map is 1024 x 512 and is the light's level-0 image;
    InfiniteAreaLight::new samples its distribution at twice that resolution (light.rs:348-398): 2048 x 1024."""
    with pytest.warns(UserWarning, match="sunsky"):
        _, scene = ptrs.import_scene(SUNSKY, (48, 32))
    assert [l["kind"] for l in scene.lights] == [ptrs.abi.LIGHT_INFINITE]
    env = scene.lights[0]
    hdr = ptrs.textures.read_rgbe(os.path.join(ROOT, "data", "abandoned_tank_farm_04_1k.hdr"))
    assert hdr.shape == (512, 1024, 3)
    assert np.array_equal(_bits(scene.textures[env["lmap_tex"]]["levels"][0]), _bits(hdr))
    assert (env["dist"]["nu"], env["dist"]["nv"]) == (2048, 1024) and np.asarray(env["dist"]["func"]).shape == (1024, 2048)
    assert (np.abs(np.asarray(env["light_to_world"], np.float64) - _env_64()) <= 4 * U).all()


def test_standalone_point_and_area_emitters_add_nothing(ptrs, cli, work):
    body = GROUND + '\t<emitter type="point" />\n\t<emitter type="area" ><rgb name="radiance" value="1, 1, 1"/></emitter>\n'
    path = _write(work, "loose.xml", body)
    with pytest.warns(UserWarning, match="area lights should not be standalone"):
        _, scene = ptrs.import_scene(path, (48, 32))
    assert scene.lights == [] and len(scene.meshes) == 1
    dump = str(work / "loose.dump")
    r = subprocess.run([cli, path, "--dump-scene-full", dump], capture_output=True, text=True)
    assert r.returncode == 0 and "area lights should not be standalone" in r.stderr
    assert _read_full_dump(dump, ptrs.abi)[4] == []


# ---- 5. Python host = C++ host ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,res", [(ALL, (96, 64)), (ALL, (37, 23)), (SUNSKY, (48, 32))])
def test_cpp_import_matches_python_import(cli, ptrs, tmp_path, path, res):
    """Camera, meshes, materials, textures with every MIP level, lights with their distributions (the helpers of test_host_cpp.py), and
    what those helpers leave out: the checker's second colour and every texture's UV mapping."""
    dump = str(tmp_path / "full.dump")
    subprocess.check_call([cli, path, "--dump-scene-full", dump, "-r", "%dx%d" % res])
    cam_p, scene = _import(ptrs, path, res)
    full = _read_full_dump(dump, ptrs.abi)
    _compare_full(ptrs.abi, full, cam_p, scene)
    for c, t in zip(full[3], scene.textures):
        assert np.array_equal(_bits(c["uvmap"]), _bits([t.get("su", 1.0), t.get("sv", 1.0), t.get("du", 0.0), t.get("dv", 0.0)]))
        if t["kind"] == ptrs.abi.TEX_CHECKER:
            assert np.array_equal(_bits(c["value"]), _bits(t["value"])) and np.array_equal(_bits(c["value2"]), _bits(t["value2"]))
    for c, m in zip(full[1], scene.meshes):
        assert (c["normal"] is None) == (m["normal"] is None) and (c["uv"] is None) == (m["uv"] is None)


def test_cpp_env_map_flag_overrides_the_sunsky_map(cli, ptrs, work):
    dump = str(work / "full.dump")
    hdr = str(work / "env_16x8.hdr")
    subprocess.check_call([cli, SUNSKY, "--dump-scene-full", dump, "-r", "48x32", "--env_map", hdr])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cam_p, scene = ptrs.import_scene(SUNSKY, (48, 32), env_map=hdr)
    assert scene.lights[0]["dist"]["nu"] == 32
    _compare_full(ptrs.abi, _read_full_dump(dump, ptrs.abi), cam_p, scene)


# ---- 6. the imported scene renders identically on the host twin and the oracle -------------------------------------------------------
def test_imported_scene_twin_matches_oracle(ptrs, orc):
    cam, scene = _import(ptrs, ALL, (48, 32))
    p = orc.make_params(48, 32, 4, 5)
    _, so, sto = orc.OracleScene(scene).render(cam, p, n_threads=4, want_samples=True)
    _, stw, stt = twin.TwinScene(scene).render(cam, p, want_samples=True)
    assert (stt.rays_extension, stt.rays_shadow, stt.rays_mis) == (sto.rays_extension, sto.rays_shadow, sto.rays_mis)
    assert stt.samples == sto.samples
    bad = (so.view(np.uint32) != stw.view(np.uint32)).any(axis=-1)
    assert bad.sum() == 0, "%d of %d samples differ" % (bad.sum(), bad.size)
    assert np.isfinite(stw).all() and stw.mean() > 0.01
