"""ptrs_scene_create's contract (include/ptrs.h): the descriptions it must refuse, with the rule named, and the legal edges it must accept.
CPU only: tests/cpp/scene_desc_cases.cpp runs the table through build_host_scene (csrc/pt_host_scene.h) stand-alone; a dozen refused rows,
rebuilt here, go through the real library, which refuses them before its first device call.  No refused row is ever rendered or traced."""
import ctypes as C
import os
import subprocess

import numpy as np

import scene_desc_cases as cases
from conftest import ROOT

A = cases.A
INVALID, UNSUPPORTED, DEVICE = -1, -2, -3

NULL_ROWS = {
    "textures_null": "textures is NULL", "materials_null": "materials is NULL", "lights_null": "lights is NULL", "meshes_null": "meshes is NULL",
    "level_data_null": "image texture: level_data is NULL", "level_cols_null": "image texture: level_cols is NULL",
    "level_rows_null": "image texture: level_rows is NULL", "level_data_1_null": "image texture: a level's data is NULL",
    "bvh_prims_null": "bvh_nodes without bvh_prims",
}
TEXTURE_ROWS = {
    "texture_kind_-1": "texture kind out of range", "texture_kind_3": "texture kind out of range",
    "texture_channels_0": "texture channels must be 1 or 3", "texture_channels_2": "texture channels must be 1 or 3", "texture_channels_4": "texture channels must be 1 or 3",
    "image_n_levels_0": "image texture without levels", "image_n_levels_-1": "image texture without levels",
    "level_cols_0": "empty texture level", "level_cols_-3": "empty texture level", "level_rows_0": "empty texture level", "level_rows_-3": "empty texture level",
    "image_wrap_-1": "image texture wrap out of range", "image_wrap_3": "image texture wrap out of range",
}
NEED3, NEED1 = "material needs a 3-channel texture in a slot that has none", "material needs a 1-channel texture in a slot that has none"
# the slots every kind requires (include/ptrs.h PTRS_MAT_*), by material index of the base = kind: 3 or 1 channels
REQUIRED = {0: [3], 1: [3, 3, 3], 3: [3, 3, 1], 4: [3, 1, 1, 1], 5: [3, 3, 1, 1], 6: [3]}
MATERIAL_ROWS = {"material_%d_slot_%d_channels" % (m, k): (NEED3 if ch == 3 else NEED1) for m, need in REQUIRED.items() for k, ch in enumerate(need)}
MATERIAL_ROWS.update({
    "material_1_slot_3_channels": "metal: roughness textures have 1 channel",
    "material_slot_-2": "material texture id out of range", "material_slot_n_textures": "material texture id out of range",
    "metal_u_rough_alone": "metal: u_rough and v_rough come both or not at all", "metal_v_rough_alone": "metal: u_rough and v_rough come both or not at all",
    "metal_no_roughness": "metal without a roughness texture",
    "normal_inner_-1": "normal material: inner out of range", "normal_inner_n_materials": "normal material: inner out of range",
    "normal_inner_itself": "normal material wraps itself", "normal_pair_names_each_other": "normal materials wrap each other",
    "normal_chain_of_five": "normal materials nested too deeply",
})
MESH_ROWS = {
    "mesh_material_-1": "mesh material out of range", "mesh_material_n_materials": "mesh material out of range",
    "vertex_index_n_verts": "vertex index out of range", "no_vertices_with_a_triangle": "mesh with triangles but no vertices",
    "alpha_mask_3_channels": "alpha mask must be a 1-channel texture", "pos_null": "mesh with triangles but pos is NULL",
    "indices_null": "mesh with triangles but indices is NULL", "position_nan": "mesh 1 vertex 2: position is not finite",
    "position_+inf": "mesh 1 vertex 2: position is not finite", "position_-inf": "mesh 0 vertex 5: position is not finite",
}
LIGHT_ROWS = {
    "area_mesh_n_meshes": "area light: mesh out of range", "area_tri_n_tris": "area light: triangle out of range",
    "area_ke_tex_-1": "area light: ke_tex must be a 3-channel texture", "area_ke_tex_1_channel": "area light: ke_tex must be a 3-channel texture",
    "infinite_lmap_constant": "infinite light: lmap_tex must be a 3-channel image texture",
    "infinite_dist_nu_0": "infinite light: distribution without rows or columns", "infinite_dist_nu_-1": "infinite light: distribution without rows or columns",
    "infinite_dist_nv_0": "infinite light: distribution without rows or columns", "infinite_dist_nv_-1": "infinite light: distribution without rows or columns",
    "infinite_dist_func_null": "infinite light: dist_func is NULL", "infinite_dist_cdf_null": "infinite light: dist_cdf is NULL",
    "infinite_dist_func_int_null": "infinite light: dist_func_int is NULL", "infinite_marg_cdf_null": "infinite light: marg_cdf is NULL",
}
TWICE = "bvh node reached twice"
TREE_ROWS = {
    "tree_leaf_range_wraps": "bvh leaf range out of bounds", "tree_leaf_range_past_end": "bvh leaf range out of bounds",
    "tree_child_n_nodes": "bvh child index out of range", "tree_interior_in_last_slot": "bvh interior node in the last record has no first child",
    "tree_axis_3": "bvh axis out of range", "tree_prim_n_tris": "bvh prim out of range",
    "tree_child_is_itself": TWICE, "tree_child_is_parent": TWICE, "tree_child_is_next": TWICE, "tree_chain_of_64": TWICE, "tree_two_parents_share_a_child": TWICE,
    "tree_node_never_reached": "bvh node never reached",
}
REFUSED = {n: (INVALID, m) for rows in (NULL_ROWS, TEXTURE_ROWS, MATERIAL_ROWS, MESH_ROWS, LIGHT_ROWS, TREE_ROWS) for n, m in rows.items()}
REFUSED.update({n: (UNSUPPORTED, "unknown material kind") for n in ("material_kind_7", "material_kind_-1")})
REFUSED.update({n: (UNSUPPORTED, "unknown light kind") for n in ("light_kind_4", "light_kind_-1")})

# accepted rows: the facts that must hold (the other facts of a row that keeps the base's tree must equal the base row's)
LIKE_BASE = dict(n_tris=6, quad=0, tree_is_base=1, planes_ok=1)
NO_TRIANGLE = dict(n_tris=0, nodes=0, nodes2=1, nodes4=0, quad=0, reported=1, depth=1, planes_ok=1)      # one pair record no ray can enter
NO_TRIANGLE_QUAD = dict(n_tris=0, nodes=0, nodes2=0, nodes4=1, quad=1, reported=1, depth=1, planes_ok=1)  # node_form = 2: one quad record of empty slots
ACCEPTED = {
    "base": LIKE_BASE, "base_own_builder": LIKE_BASE, "unused_records_appended": LIKE_BASE, "normal_chain_of_four": LIKE_BASE,
    "zero_triangle_mesh_first": LIKE_BASE, "zero_triangle_mesh_wild_pointers": LIKE_BASE, "scaled_2^-60": LIKE_BASE, "scaled_2^60": LIKE_BASE,
    "no_mesh": NO_TRIANGLE, "no_mesh_no_light": NO_TRIANGLE, "only_zero_triangle_meshes": NO_TRIANGLE,
    "no_mesh_quad_form": NO_TRIANGLE_QUAD, "only_zero_triangle_meshes_quad_form": NO_TRIANGLE_QUAD,
    "one_triangle_root_leaf_tree": dict(n_tris=1, nodes=1, nodes2=1, nodes4=0, quad=0, reported=1, planes_ok=1),
    "one_triangle": dict(n_tris=1, nodes=1, nodes2=1, nodes4=0, quad=0, reported=1, planes_ok=1),
    "one_triangle_quad_form": dict(n_tris=1, nodes=1, nodes2=0, nodes4=1, quad=1, reported=1, planes_ok=1),
}


def test_scene_description_table(orc, tmp_path):
    """tests/cpp/scene_desc_cases.cpp: every row's return code and message (refused) or layout facts (accepted; the oracle accepts the same
    description).  The child's time limit is a hang guard only: every row is linear in the description's size, the chain of 64 nodes whose
    paths number 2^64 included.  A row that crashes the program, or a row the table does not know, fails here."""
    exe = str(tmp_path / "scene_desc_cases")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "scene_desc_cases.cpp"), "-ldl"])
    out = subprocess.run([exe, os.path.join(ROOT, "oracle", "liboracle.so")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[-1] == "rows\t%d" % (len(REFUSED) + len(ACCEPTED)), lines[-1]
    seen = {}
    for line in lines[:-1]:
        name, code, text = line.split("\t")
        assert name not in seen, name
        seen[name] = (int(code), text)
    assert set(seen) == set(REFUSED) | set(ACCEPTED)
    for name, want in REFUSED.items():
        assert seen[name] == want, (name, seen[name])
    facts = {}
    for name, want in ACCEPTED.items():
        code, text = seen[name]
        assert code == 0, (name, text)
        facts[name] = dict((k, int(v)) for k, v in (f.split("=") for f in text.split()))
        assert facts[name].pop("oracle") == 0, name
        for k, v in want.items():
            assert facts[name][k] == v, (name, k, facts[name])
    for name, want in ACCEPTED.items():
        if want is LIKE_BASE:
            assert facts[name] == facts["base"], name


def _create(desc):
    lib = cases.ptrs.load_library()
    h = C.c_void_p()
    rc = lib.ptrs_scene_create(C.byref(desc), 0, C.byref(h))
    msg = lib.ptrs_last_error().decode()
    assert (rc == 0) == bool(h), "a handle comes back with PTRS_OK and only then"
    return rc, msg, h


def _base_tree(orc):
    nodes, prims = orc.OracleScene(cases.base_scene()[1]).get_bvh()
    return nodes, prims


def _chain(nodes, prims):
    c = np.zeros(64, nodes.dtype)
    c["p_min"], c["p_max"] = nodes[0]["p_min"], nodes[0]["p_max"]
    c["offset"] = np.arange(1, 65)
    c[63]["offset"], c[63]["num_prims"] = 0, 1
    return c, prims


def _leaf_wraps(nodes, prims):
    i = int(np.flatnonzero(nodes["num_prims"])[0])
    nodes[i]["offset"], nodes[i]["num_prims"] = 0xffffffff, 1
    return nodes, prims


def _child_is_itself(nodes, prims):
    i = int(np.flatnonzero(nodes["num_prims"] == 0)[-1])
    nodes[i]["offset"] = i
    return nodes, prims


def _set(path, value):
    """A row that overwrites one field of the ctypes records behind the description: path = (array, index, field[, index])."""
    def f(d):
        rec = getattr(d, path[0])[path[1]]
        if len(path) == 4:
            getattr(rec, path[2])[path[3]] = value
        else:
            setattr(rec, path[2], value)
    return f


def _null_level(d):
    d.textures[3].level_data[1] = A.f32p()


def _nan_position(d):
    d.meshes[1].pos[3 * 2 + 1] = float("nan")


def _normal_pair(d):  # the Mirror becomes a second wrapper: 2 -> 6 -> 2
    d.materials[2].kind, d.materials[2].inner = A.MAT_NORMAL, 6
    d.materials[2].tex[0] = 3
    d.materials[6].inner = 2


# name -> (change of the description's records | None, change of the pre-built tree | None, code, message)
LIBRARY_ROWS = {
    "textures_null": (lambda d: setattr(d, "textures", C.POINTER(A.PtrsTexture)()), None, INVALID, "textures is NULL"),
    "level_data_1_null": (_null_level, None, INVALID, "image texture: a level's data is NULL"),
    "image_wrap_3": (_set(("textures", 3, "wrap"), 3), None, INVALID, "image texture wrap out of range"),
    "material_slot_-2": (_set(("materials", 2, "tex", 5), -2), None, INVALID, "material texture id out of range"),
    "metal_u_rough_alone": (_set(("materials", 1, "tex", 4), 1), None, INVALID, "metal: u_rough and v_rough come both or not at all"),
    "normal_pair_names_each_other": (_normal_pair, None, INVALID, "normal materials wrap each other"),
    "mesh_material_n_materials": (_set(("meshes", 1, "material"), 7), None, INVALID, "mesh material out of range"),
    "position_nan": (_nan_position, None, INVALID, "mesh 1 vertex 2: position is not finite"),
    "indices_null": (_set(("meshes", 0, "indices"), A.u32p()), None, INVALID, "mesh with triangles but indices is NULL"),
    "area_tri_n_tris": (_set(("lights", 0, "tri"), 2), None, INVALID, "area light: triangle out of range"),
    "infinite_dist_cdf_null": (_set(("lights", 2, "dist_cdf"), A.f32p()), None, INVALID, "infinite light: dist_cdf is NULL"),
    "light_kind_4": (_set(("lights", 1, "kind"), 4), None, UNSUPPORTED, "unknown light kind"),
    "tree_leaf_range_wraps": (None, _leaf_wraps, INVALID, "bvh leaf range out of bounds"),
    "tree_child_is_itself": (None, _child_is_itself, INVALID, TWICE),
    "tree_chain_of_64": (None, _chain, INVALID, TWICE),
}


def test_library_refuses_before_the_first_device_call(orc):
    """The same rows through ptrs_scene_create of the real library, built with abi.SceneDescHolder and changed in its ctypes records: code
    and message are build_host_scene's, on a machine without a GPU too -- the description is checked before a device is selected.  A valid
    description gets PTRS_ERR_DEVICE there (no fall-back, tests/test_abi.py), so the order of the two checks is what is seen."""
    import torch
    tree = _base_tree(orc)
    for name, (change, change_tree, code, message) in LIBRARY_ROWS.items():
        assert REFUSED[name] == (code, message), name  # the row is the table's
        _, scene = cases.base_scene()
        bvh = change_tree(tree[0].copy(), tree[1].copy()) if change_tree else None
        desc = scene.desc(bvh)
        if change:
            change(desc)
        rc, msg, h = _create(desc)
        assert (rc, msg) == (code, message), name
    if not torch.cuda.is_available():  # (with a GPU a valid description creates a scene: the gpu tests' business)
        for bvh in (None, tree):
            _, scene = cases.base_scene()  # (the scene owns the description's buffers)
            rc, msg, _ = _create(scene.desc(bvh))
            assert rc == DEVICE and "no HIP device" in msg, (rc, msg)
