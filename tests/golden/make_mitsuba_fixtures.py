"""Writes the Mitsuba importer's fixtures under tests/golden/mitsuba/ (tests/test_mitsuba_import.py,
tests/test_gpu_mitsuba.py).  All of them are this project's own: hand-written scene files and a mesh, seeded images.

    python tests/golden/make_mitsuba_fixtures.py

  all_features.xml  floor rectangle with a bitmap reflectance, cube with a checkerboard roughplastic, matte sphere, emissive
                    sphere, obj with vt and a bitmap, obj with faceNormals, a shape with an embedded bsdf, envmap with a toWorld
  sunsky.xml        one rectangle under a sunsky emitter (falls back to data/abandoned_tank_farm_04_1k.hdr)
  mesh.obj          octahedron, 8 triangles, vn and vt at every vertex
  tex_rgb.png       12 x 20 RGB8 (not a power of two: the Lanczos resample runs)
  tex_4x4.png       4 x 4 RGB8, 16 distinct texels
  tex_rgba.png      4 x 4 RGBA8 (refused as a bitmap texture)
  env_16x8.hdr      16 x 8 Radiance map, flat scanlines
"""
import os

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mitsuba")

SENSOR = """	<sensor type="perspective" >
		<float name="fov" value="24" />
		<transform name="toWorld" >
			<matrix value="-1 0 0 0 0 1 0 1 0 0 -1 6.8 0 0 0 1"/>
		</transform>
		<film type="ldrfilm" >
			<integer name="width" value="96" />
			<integer name="height" value="64" />
		</film>
	</sensor>
"""

ALL_FEATURES = """<?xml version="1.0" encoding="utf-8"?>
<!-- every construct of the Mitsuba importer in one small open scene -->
<scene version="0.5.0" >
""" + SENSOR + """	<bsdf type="twosided" id="Floor" >
		<bsdf type="diffuse" >
			<rgb name="reflectance" value="0.2, 0.2, 0.2"/>
			<texture type="bitmap" name="reflectance" >
				<string name="filename" value="tex_rgb.png" />
			</texture>
		</bsdf>
	</bsdf>
	<bsdf type="roughplastic" id="Checker" >
		<float name="intIOR" value="1.5" />
		<float name="alpha" value="0.25" />
		<texture type="checkerboard" name="diffuseReflectance" >
			<rgb name="color0" value="0.8, 0.1, 0.1"/>
			<rgb name="color1" value="0.1, 0.2, 0.8"/>
			<float name="uscale" value="4" />
			<float name="vscale" value="3" />
			<float name="uoffset" value="0.125" />
			<float name="voffset" value="0.25" />
		</texture>
	</bsdf>
	<bsdf type="diffuse" id="Matte" >
		<rgb name="reflectance" value="0.7, 0.6, 0.4"/>
	</bsdf>
	<bsdf type="diffuse" id="Lamp" >
		<rgb name="reflectance" value="0, 0, 0"/>
	</bsdf>
	<bsdf type="twosided" id="Painted" >
		<bsdf type="diffuse" >
			<texture type="bitmap" name="reflectance" >
				<string name="filename" value="tex_4x4.png" />
			</texture>
		</bsdf>
	</bsdf>
	<bsdf type="roughconductor" id="Copper" >
		<float name="alpha" value="0.125" />
		<rgb name="eta" value="0.2, 0.92, 1.1"/>
		<rgb name="k" value="3.9, 2.45, 2.14"/>
		<rgb name="specularReflectance" value="0.9, 0.9, 0.9"/>
	</bsdf>
	<shape type="rectangle" >
		<transform name="toWorld" >
			<matrix value="2 0 0 0 0 0 2 0 0 -2 0 0 0 0 0 1"/>
		</transform>
		<ref id="Floor" />
	</shape>
	<shape type="cube" >
		<transform name="toWorld" >
			<matrix value="0.303109 0 0.175 -0.75 0 0.35 0 0.35 -0.175 0 0.303109 -0.1 0 0 0 1"/>
		</transform>
		<ref id="Checker" />
	</shape>
	<shape type="sphere" >
		<point name="center" x="0.55" y="0.4" z="0.3" />
		<float name="radius" value="0.4" />
		<ref id="Matte" />
	</shape>
	<shape type="sphere" >
		<point name="center" x="-0.1" y="1.75" z="0.2" />
		<float name="radius" value="0.125" />
		<ref id="Lamp" />
		<emitter type="area" >
			<rgb name="radiance" value="9, 8, 6"/>
		</emitter>
	</shape>
	<shape type="obj" >
		<string name="filename" value="mesh.obj" />
		<transform name="toWorld" >
			<matrix value="0.25 -0.12 0.05 -0.15 0.1 0.28 0.07 0.95 -0.08 0.04 0.29 -0.5 0 0 0 1"/>
		</transform>
		<ref id="Painted" />
	</shape>
	<shape type="obj" >
		<string name="filename" value="mesh.obj" />
		<boolean name="faceNormals" value="true" />
		<transform name="toWorld" >
			<matrix value="0.3 0 0 0.9 0 0.45 0 1.1 0 0 0.3 -0.6 0 0 0 1"/>
		</transform>
		<ref id="Copper" />
	</shape>
	<shape type="rectangle" >
		<transform name="toWorld" >
			<matrix value="1.5 0 0 0 0 1 0 1 0 0 1 -1.5 0 0 0 1"/>
		</transform>
		<bsdf type="plastic" >
			<float name="intIOR" value="1.49" />
			<rgb name="diffuseReflectance" value="0.3, 0.5, 0.35"/>
		</bsdf>
	</shape>
	<emitter type="point" />
	<emitter type="envmap" >
		<transform name="toWorld" >
			<matrix value="0.866025 0 0.5 0 0.1 0.98 -0.173205 0 -0.49 0.2 0.848705 0 0 0 0 1"/>
		</transform>
		<string name="filename" value="env_16x8.hdr" />
	</emitter>
</scene>
"""

SUNSKY = """<?xml version="1.0" encoding="utf-8"?>
<scene version="0.5.0" >
""" + SENSOR + """	<bsdf type="diffuse" id="Ground" >
		<rgb name="reflectance" value="0.5, 0.5, 0.5"/>
	</bsdf>
	<shape type="rectangle" >
		<transform name="toWorld" >
			<matrix value="2 0 0 0 0 0 2 0 0 -2 0 0 0 0 0 1"/>
		</transform>
		<ref id="Ground" />
	</shape>
	<shape type="sphere" >
		<point name="center" x="0" y="0.5" z="0" />
		<float name="radius" value="0.5" />
		<ref id="Ground" />
	</shape>
	<emitter type="sunsky" />
</scene>
"""


def octahedron_obj():
    """6 vertices, 8 outward-wound triangles; vn = the unit vertex, vt = a seeded point of the unit square per vertex."""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    vt = [(0.1, 0.2), (0.9, 0.3), (0.5, 0.95), (0.45, 0.05), (0.3, 0.6), (0.75, 0.7)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    lines = ["# octahedron: position, normal and texture index are equal at every corner", "mtllib none.mtl", "o octahedron"]
    lines += ["v %g %g %g" % p for p in v] + ["vn %g %g %g" % p for p in v] + ["vt %g %g" % t for t in vt]
    lines += ["g faces", "usemtl none", "s 1"] + ["f " + " ".join("%d/%d/%d" % (i + 1, i + 1, i + 1) for i in t) for t in f]
    return "\n".join(lines) + "\n"


def write_rgbe_flat(path, img):
    img = np.asarray(img, dtype=np.float32)
    m = img.max(axis=-1)
    e = np.where(m > 1e-32, np.floor(np.log2(np.maximum(m, 1e-38))) + 1, 0).astype(np.int32)
    scale = np.where(m > 1e-32, np.exp2((8 - e).astype(np.float32)), 0).astype(np.float32)
    rgbe = np.zeros(img.shape[:2] + (4,), np.uint8)
    rgbe[..., :3] = np.clip(img * scale[..., None], 0, 255).astype(np.uint8)
    rgbe[..., 3] = np.where(m > 1e-32, e + 128, 0).astype(np.uint8)
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % img.shape[:2])
        f.write(rgbe.tobytes())


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(11)
    for name, text in (("all_features.xml", ALL_FEATURES), ("sunsky.xml", SUNSKY), ("mesh.obj", octahedron_obj())):
        with open(os.path.join(OUT, name), "w") as f:
            f.write(text)
    Image.fromarray(rng.integers(30, 240, (20, 12, 3)).astype(np.uint8), "RGB").save(os.path.join(OUT, "tex_rgb.png"))
    t4 = np.zeros((4, 4, 3), np.uint8)
    for r in range(4):
        for c in range(4):
            t4[r, c] = (20 + 60 * c, 30 + 55 * r, 250 - 13 * (4 * r + c))
    Image.fromarray(t4, "RGB").save(os.path.join(OUT, "tex_4x4.png"))
    Image.fromarray(np.dstack([t4, np.full((4, 4), 200, np.uint8)]), "RGBA").save(os.path.join(OUT, "tex_rgba.png"))
    # sky gradient over a dim ground, one bright texel: enough structure for the light's 2-D distribution
    v = (np.arange(8, dtype=np.float32) + 0.5) / 8
    env = np.where((v < 0.5)[:, None, None], np.stack([0.4 + 0.5 * (1 - v), 0.6 + 0.3 * (1 - v), 1.0 + 0 * v], -1)[:, None, :], np.array([0.2, 0.16, 0.12], np.float32))
    env = (env * (1.0 + 0.2 * rng.uniform(-1, 1, (8, 16, 1)))).astype(np.float32)
    env[2, 5] = (60.0, 50.0, 40.0)
    write_rgbe_flat(os.path.join(OUT, "env_16x8.hdr"), env)


if __name__ == "__main__":
    main()
