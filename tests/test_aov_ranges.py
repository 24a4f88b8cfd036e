"""Feature planes for sample ranges and tiles, and the planes of an adaptive film (ptrs_render_aov_range, ptrs_render_aov_tiles,
ptrs_render_aov_adaptive).  Every claim is a bit comparison unless it says otherwise.

On the CPU the aov plan twin (tests/aov_plan_twin: render_aov_impl itself on the host twin's back end plus the AOV hooks) is held
against itself (chained ranges against the dense call, tiles against the range call), against the aov twin's per-sample rows, against
the converge twin's beauty weights and against the adaptive twin's film.  The argument checks call the library and need no device; the
motivating known answer runs through the denoise twin.  Under -m gpu the device is held against the twin on five shapes and every
mask, under the schedule knobs, over stale slots, end to end through render_adaptive, render_denoised and the CLI.
"""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded: one HIP runtime per process)

from conftest import CORNELL, ROOT

for _d in ("aov_plan_twin", "aov_twin", "denoise_twin", "converge_twin", "adaptive_twin"):
    sys.path.insert(0, os.path.join(ROOT, "tests", _d))
import adaptive_twin  # noqa: E402
import aov_plan_twin  # noqa: E402
import aov_twin  # noqa: E402
import converge_twin  # noqa: E402
import denoise_twin  # noqa: E402
from test_adaptive import CASES, MASKS, SENTINEL, active_sample_pixels, midpoint_target, tile_mask, tile_pixels  # noqa: E402
from test_camera_film_kat import outside_pfilm  # noqa: E402

ptrs = importlib.import_module("pathtracer-rs_amd")
scenes_mod = importlib.import_module("pathtracer-rs_amd.scenes")
A = ptrs.abi
F32 = np.float32
CLI = os.path.join(ROOT, "pathtracer-rs_amd", "ptrs_headless")
INVALID, DEVICE = -1, -3
NAMES = ("albedo", "normal", "depth")

# shape -> (resolution, spp, depth of the beauty renders, the sample range of the range and mask tests)
SHAPES = {k: (v[0], v[1], v[2], v[3]) for k, v in CASES.items()}  # cornell 40 x 36 / 16, material_zoo 48 x 32 / 4, stratified 24 x 20 / 9
SHAPES["gltf"] = ((48, 32), 4, 3, (1, 3))          # image textures through the differentials, a normal map, an alpha card; 900 paths per pass: band mode
SHAPES["textured_env"] = ((48, 32), 2, 3, (1, 2))  # misses
BAND_PPP = 900


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def stack_values(films):
    """(3, H, W) FILM_DTYPE -> (3, H, W, 4) float32: rgb, weight."""
    return np.concatenate([films["rgb"], films["weight"][..., None]], axis=-1)


def same(a, b, sel=None):
    va, vb = bits(stack_values(a)), bits(stack_values(b))
    return np.array_equal(va, vb) if sel is None else np.array_equal(va[:, sel], vb[:, sel])


def start_planes(W, H, seed):
    """Three planes as a few earlier samples leave them: non-zero everywhere, different from each other."""
    rng = np.random.default_rng(seed)
    f = np.zeros((3, H, W), A.FILM_DTYPE)
    f["weight"] = rng.uniform(0.5, 1.5, (3, H, W)).astype(F32)
    f["rgb"] = rng.uniform(0.05, 0.9, (3, H, W, 3)).astype(F32) * f["weight"][..., None]
    return f


_scenes = {}


def make_scene(name, tmp_path_factory):
    if name not in _scenes:
        (W, H), spp, depth, _r = SHAPES[name]
        if name == "zoo":
            _scenes[name] = scenes_mod.material_zoo((W, H))
        elif name == "textured_env":
            _scenes[name] = scenes_mod.textured_env((W, H))
        elif name == "gltf":
            import gltf_fixture as gf
            _scenes[name] = ptrs.import_scene(gf.write_gltf(str(tmp_path_factory.mktemp("aov_ranges_gltf")), glb=True), (W, H))
        else:
            _scenes[name] = ptrs.import_scene(CORNELL, (W, H))
    return _scenes[name]


def twin_params(orc, name, **kw):
    (W, H), spp, depth, _r = SHAPES[name]
    if name == "stratified":
        return orc.make_params(W, H, spp, depth, sampler=A.SAMPLER_STRATIFIED, n_sampled_dimensions=19, **kw)
    return orc.make_params(W, H, spp, depth, **kw)


_twin_cases = {}


def twin_case(orc, name, tmp_path_factory):
    """Made once per shape on the twin: start planes, the dense call on them (planes and samples), the range call on them."""
    if name not in _twin_cases:
        (W, H), spp, depth, (b, e) = SHAPES[name]
        cam, scene = make_scene(name, tmp_path_factory)
        ts = aov_plan_twin.AovScene(scene)
        p = twin_params(orc, name)
        start = start_planes(W, H, 5)
        dense, dense_s = start.copy(), np.zeros((H + 4, W + 4, spp, 12), F32)
        dense_st = ts.render(cam, p, dense, samples=dense_s)
        rng_f, rng_s = start.copy(), np.full((H + 4, W + 4, spp, 12), SENTINEL, F32)
        rng_st = ts.render(cam, p, rng_f, sample_range=(b, e), samples=rng_s)
        for a in (start, dense, dense_s, rng_f, rng_s):
            a.setflags(write=False)
        _twin_cases[name] = dict(cam=cam, scene=scene, ts=ts, p=p, start=start, dense=dense, dense_s=dense_s, dense_st=dense_st, rng=rng_f, rng_s=rng_s, rng_st=rng_st)
    return _twin_cases[name]


def check_aov_tiles(what, m, W, H, b, e, got, start, ref, samples, ref_samples, stats, ref_stats):
    """test_adaptive's check_tiles_result on three planes: active tiles hold the range call's bits, inactive tiles the start's; the
    sample export holds the reference's values on the active sample pixels inside the range and the sentinel elsewhere; the sample
    count is the numpy dilation count; the rays are at most the range call's, and equal with every tile active."""
    px, act = tile_pixels(m, W, H), active_sample_pixels(m, W, H)
    assert same(got, ref, px), what + ": an active tile's pixels differ from the range call's"
    assert same(got, start, ~px), what + ": an inactive tile's pixels changed"
    if samples is not None:
        inside = np.zeros(samples.shape[:3], bool)
        inside[:, :, b:e] = act[..., None]
        assert np.array_equal(bits(samples)[inside], bits(ref_samples)[inside]), what + ": exported samples of active sample pixels differ"
        assert (samples[~inside] == SENTINEL).all(), what + ": an entry outside the active sample pixels / the range was written"
    n = int(act.sum()) * (e - b)
    assert stats.samples == n, (what, stats.samples, n)
    assert stats.rays_extension <= ref_stats.rays_extension and (stats.rays_shadow, stats.rays_mis) == (0, 0), what
    if (m != 0).all():
        assert stats.rays_extension == ref_stats.rays_extension and stats.samples == ref_stats.samples, what
    if not (m != 0).any():
        assert stats.rays_extension == 0 and stats.passes == 0 and stats.kernel_launches == 0, what


# ---- CPU: the range form on the twin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_twin_chained_ranges_equal_the_dense_call(orc, name, tmp_path_factory):
    """Ranges [0, a), [a, b), [b, spp) from seeded non-zero planes give the dense call's planes and samples, under the default plan and
    at 900 paths per pass (gltf and cornell: row blocks, band mode); the dense samples are the aov twin's rows."""
    c = twin_case(orc, name, tmp_path_factory)
    (W, H), spp, depth, (a, b) = SHAPES[name]
    cam, ts = c["cam"], c["ts"]
    cuts = sorted(set([0, a, b, spp]))
    assert c["dense_st"].samples == (W + 4) * (H + 4) * spp and c["rng_st"].samples == (W + 4) * (H + 4) * (b - a)
    for ppp in (0, BAND_PPP):
        p = twin_params(orc, name, paths_per_pass=ppp)
        if ppp:
            d2 = c["start"].copy()
            st = ts.render(cam, p, d2)
            assert same(d2, c["dense"]), "%s: the dense call depends on the pass plan" % name
            if (W + 4) * (H + 4) > ppp:  # band mode: row blocks x sample indices
                assert st.passes == -(-(H + 4) // (ppp // (W + 4))) * spp, (name, st.passes)
        f, s = c["start"].copy(), np.full(c["dense_s"].shape, SENTINEL, F32)
        n = 0
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            n += ts.render(cam, p, f, sample_range=(lo, hi), samples=s).samples
        assert same(f, c["dense"]), "%s, paths_per_pass %d: chained ranges differ from the dense call" % (name, ppp)
        assert np.array_equal(bits(s), bits(c["dense_s"])) and n == c["dense_st"].samples
    # the range call's export: its entries are the dense call's, everything else is untouched
    inside = np.zeros(c["rng_s"].shape[:3], bool)
    inside[:, :, a:b] = True
    assert np.array_equal(bits(c["rng_s"])[inside], bits(c["dense_s"])[inside]) and (c["rng_s"][~inside] == SENTINEL).all()
    if name != "stratified":
        pf, _ = outside_pfilm(W, H, spp, "twin")
        rows = aov_twin.aov_rows(c["scene"], cam, float(F32(1.0) / np.sqrt(F32(spp))), pf.reshape(-1, 2))
        assert np.array_equal(bits(rows), bits(c["dense_s"].reshape(-1, 12))), name
    if name == "textured_env":
        assert (c["dense_s"][..., 3] == 0).any() and (c["dense_s"][..., 3] == 1).any()  # misses and hits


# ---- CPU: the tile form on the twin -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_twin_tiles_equal_the_range_call(orc, name, mask, tmp_path_factory):
    c = twin_case(orc, name, tmp_path_factory)
    (W, H), spp, depth, (b, e) = SHAPES[name]
    m = tile_mask(mask, W, H)
    f, s = c["start"].copy(), np.full(c["dense_s"].shape, SENTINEL, F32)
    st = c["ts"].render(c["cam"], c["p"], f, sample_range=(b, e), tiles=m, samples=s)
    check_aov_tiles("%s %s" % (name, mask), m, W, H, b, e, f, c["start"], c["rng"], s, c["dense_s"], st, c["rng_st"])


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("name", ["cornell", "gltf"])
def test_twin_tiles_in_band_mode(orc, name, mask, tmp_path_factory):
    """900 paths per pass: row blocks, one gather per sample index over the band on the tile list; blocks without an active sample
    pixel are not run.  The same bits as under the default plan."""
    c = twin_case(orc, name, tmp_path_factory)
    (W, H), spp, depth, (b, e) = SHAPES[name]
    m = tile_mask(mask, W, H)
    p = twin_params(orc, name, paths_per_pass=BAND_PPP)
    f, s = c["start"].copy(), np.full(c["dense_s"].shape, SENTINEL, F32)
    st = c["ts"].render(c["cam"], p, f, sample_range=(b, e), tiles=m, samples=s)
    check_aov_tiles("%s %s band mode" % (name, mask), m, W, H, b, e, f, c["start"], c["rng"], s, c["dense_s"], st, c["rng_st"])
    n_blocks = -(-(H + 4) // (BAND_PPP // (W + 4)))
    rows = -(-(H + 4) // n_blocks)
    act_rows = active_sample_pixels(m, W, H).any(axis=1)
    assert st.passes == sum(bool(act_rows[r:r + rows].any()) for r in range(0, H + 4, rows)) * (e - b), (name, mask, st.passes)


# ---- CPU: the planes' weights are the beauty film's ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "stratified"])
def test_twin_range_weights_are_the_beauty_films(orc, name, tmp_path_factory):
    """From zero films render_aov_range(0, n)'s weight channel equals the converge twin's render_range(0, n) film weight."""
    c = twin_case(orc, name, tmp_path_factory)
    (W, H), spp, depth, (_a, n) = SHAPES[name]
    rs = converge_twin.RangeScene(c["scene"])
    film = np.zeros((H, W), A.FILM_DTYPE)
    rs.render_range(c["cam"], c["p"], 0, n, film=film)
    planes = np.zeros((3, H, W), A.FILM_DTYPE)
    c["ts"].render(c["cam"], c["p"], planes, sample_range=(0, n))
    assert (film["weight"] > 0).all()
    for k in range(3):
        assert np.array_equal(bits(planes[k]["weight"]), bits(film["weight"])), (name, NAMES[k])


# ---- CPU: the adaptive loop ---------------------------------------------------------------------------------------------------------
def test_twin_planes_of_an_adaptive_film(orc, tmp_path_factory):
    """The adaptive twin's render_adaptive (Cornell 40 x 36, ceiling 16, min 2, the midpoint target of test_twin_adaptive_loop) leaves
    tiles at different sample counts; render_aov_adaptive(tile_spp) gives per tile the bits of render_aov_range(0, tile_spp[t]), and
    weights equal to the adaptive film's on every pixel."""
    c = twin_case(orc, "cornell", tmp_path_factory)
    (W, H), spp, depth, _r = SHAPES["cornell"]
    mn = CASES["cornell"][4]
    cam, p, ts = c["cam"], c["p"], c["ts"]
    at = adaptive_twin.TileScene(c["scene"])
    uni = at.render_adaptive(cam, p, 0.0, mn)
    target = midpoint_target(uni["tile_errors"]["error"][1])
    r = at.render_adaptive(cam, p, target, mn)
    tile_spp = r["tile_spp"]
    counts = sorted(set(tile_spp.reshape(-1).tolist()))
    print("target %.6g, tile_spp %s" % (target, tile_spp.tolist()))
    assert len(counts) >= 2, "precondition: the midpoint target must leave tiles at two different sample counts"
    planes = np.zeros((3, H, W), A.FILM_DTYPE)
    n = ts.render_adaptive(cam, p, mn, tile_spp, planes)
    assert n == r["samples"]  # the same sample pixels, block by block, as the beauty's tile passes
    for cnt in counts:
        ref = np.zeros((3, H, W), A.FILM_DTYPE)
        ts.render(cam, p, ref, sample_range=(0, cnt))
        px = tile_pixels((tile_spp == cnt).astype(np.uint8), W, H)
        assert same(planes, ref, px), "the tiles at %d samples are not render_aov_range(0, %d)'s" % (cnt, cnt)
    for k in range(3):
        assert np.array_equal(bits(planes[k]["weight"]), bits(r["film"]["weight"])), NAMES[k]
    # a tile with 0 keeps its bits
    some = tile_spp.copy()
    some[0, 0] = 0
    seeded = c["start"].copy()
    ts.render_adaptive(cam, p, mn, some, seeded)
    one = np.zeros(tile_spp.shape, np.uint8)
    one[0, 0] = 1
    assert same(seeded, c["start"], tile_pixels(one, W, H)) and not same(seeded, c["start"], ~tile_pixels(one, W, H))


# ---- CPU: argument checks through the library, no device ---------------------------------------------------------------------------
def test_entry_points_check_their_arguments():
    """Every refusal of the six entry points is PTRS_ERR_INVALID with its message, made before the first device call (without a GPU a
    well-formed call ends at "no HIP device")."""
    L = ptrs.load_library()
    assert L.ptrs_abi_version() == 4
    cam, scene = ptrs.import_scene(CORNELL, (8, 8))
    integ = ptrs.PathIntegrator(ptrs.SamplerBuilder(8, cam.film.get_sample_bounds()), 2)
    p, cabi = integ.params(cam), cam.to_abi()
    pp, cp = C.addressof(p), C.addressof(cabi)
    fake = C.addressof((C.c_char * 64)())
    planes = np.zeros((3, 8, 8), A.FILM_DTYPE)
    ptr3 = (C.c_void_p * 3)(*[planes[k].ctypes.data for k in range(3)])
    ptr2 = (C.c_void_p * 3)(planes[0].ctypes.data, None, planes[2].ctypes.data)
    st = A.PtrsStats()
    sp = C.addressof(st)
    one = np.ones(1, np.uint8)
    tp = one.ctypes.data
    pb = integ.params(cam)
    pb.row_begin, pb.row_end = 2, 6
    err = L.ptrs_last_error
    no_gpu = not torch.cuda.is_available()
    forms = [
        (lambda s, c, q, b, e, mk, pl: L.ptrs_render_aov_range(s, c, q, b, e, mk, pl, None, sp), False),
        (lambda s, c, q, b, e, mk, pl: L.ptrs_render_aov_range_device(s, c, q, b, e, mk, pl, None, None, sp), False),
        (lambda s, c, q, b, e, mk, pl: L.ptrs_render_aov_tiles(s, c, q, b, e, tp, mk, pl, None, sp), True),
        (lambda s, c, q, b, e, mk, pl: L.ptrs_render_aov_tiles_device(s, c, q, b, e, tp, mk, pl, None, None, sp), True),
    ]
    for call, tiled in forms:
        assert call(None, cp, pp, 0, 8, 7, ptr3) == INVALID and b"null" in err()
        assert call(fake, None, pp, 0, 8, 7, ptr3) == INVALID and b"null" in err()
        assert call(fake, cp, None, 0, 8, 7, ptr3) == INVALID and b"null" in err()
        for mask in (0, 8, 0xffffffff):
            assert call(fake, cp, pp, 0, 8, mask, ptr3) == INVALID and b"PTRS_AOV_" in err(), mask
        assert call(fake, cp, pp, 0, 8, 7, ptr2) == INVALID and b"null plane pointer" in err()
        assert call(fake, cp, pp, 0, 8, 7, None) == INVALID and b"null plane pointer" in err()
        for (b, e) in ((0, 0), (3, 3), (5, 4), (0, 9), (8, 9), (8, 8), (0xffffffff, 1)):
            assert call(fake, cp, pp, b, e, 7, ptr3) == INVALID and b"sample range: need sample_begin < sample_end <= spp (8" in err(), (b, e)
        if tiled:
            assert call(fake, cp, C.addressof(pb), 0, 8, 7, ptr3) == INVALID and b"whole film" in err()
        if no_gpu:
            assert call(fake, cp, pp, 0, 8, 5, ptr2) == DEVICE and b"no HIP device" in err()
            assert call(fake, cp, pp, 7, 8, 7, ptr3) == DEVICE and b"no HIP device" in err()
    assert L.ptrs_render_aov_tiles(fake, cp, pp, 0, 8, None, 7, ptr3, None, sp) == INVALID and b"null" in err()
    assert L.ptrs_render_aov_tiles_device(fake, cp, pp, 0, 8, None, 7, ptr3, None, None, sp) == INVALID and b"null" in err()
    ts = np.full(1, 8, np.uint32)
    for fn, tail in ((L.ptrs_render_aov_adaptive, (sp,)), (L.ptrs_render_aov_adaptive_device, (None, sp))):
        adp = lambda s, c, q, mn, t, mk, pl: fn(s, c, q, mn, t, mk, pl, *tail)
        assert adp(None, cp, pp, 2, ts.ctypes.data, 7, ptr3) == INVALID and b"null" in err()
        assert adp(fake, None, pp, 2, ts.ctypes.data, 7, ptr3) == INVALID and b"null" in err()
        assert adp(fake, cp, None, 2, ts.ctypes.data, 7, ptr3) == INVALID and b"null" in err()
        assert adp(fake, cp, pp, 2, None, 7, ptr3) == INVALID and b"null" in err()
        assert adp(fake, cp, pp, 2, ts.ctypes.data, 0, ptr3) == INVALID and b"PTRS_AOV_" in err()
        assert adp(fake, cp, pp, 2, ts.ctypes.data, 7, ptr2) == INVALID and b"null plane pointer" in err()
        assert adp(fake, cp, C.addressof(pb), 2, ts.ctypes.data, 7, ptr3) == INVALID and b"whole film" in err()
        for mn in (0, 1, 3, 16):
            assert adp(fake, cp, pp, mn, ts.ctypes.data, 7, ptr3) == INVALID and b"min_spp" in err(), mn
        for bad in (3, 16, 1, 6):  # neither 0 nor the end of a block of (2, 4, 8); 16 = the ceiling x 2
            t = np.full(1, bad, np.uint32)
            assert adp(fake, cp, pp, 2, t.ctypes.data, 7, ptr3) == INVALID and b"tile_spp[0] = %d" % bad in err(), bad
        if no_gpu:
            for ok in (0, 2, 4, 8):
                t = np.full(1, ok, np.uint32)
                assert adp(fake, cp, pp, 2, t.ctypes.data, 7, ptr3) == DEVICE and b"no HIP device" in err(), ok
    # a larger film: the message names the tile
    cam2, _ = ptrs.import_scene(CORNELL, (40, 36))
    p2, c2 = integ.params(cam2), cam2.to_abi()
    big = np.zeros((3, 36, 40), A.FILM_DTYPE)
    ptr_big = (C.c_void_p * 3)(*[big[k].ctypes.data for k in range(3)])
    t9 = np.full(9, 8, np.uint32)
    t9[5] = 3
    assert L.ptrs_render_aov_adaptive(fake, C.addressof(c2), C.addressof(p2), 2, t9.ctypes.data, 7, ptr_big, sp) == INVALID and b"tile_spp[5] = 3" in err()
    t9[5], t9[7] = 8, 16
    assert L.ptrs_render_aov_adaptive(fake, C.addressof(c2), C.addressof(p2), 2, t9.ctypes.data, 7, ptr_big, sp) == INVALID and b"tile_spp[7] = 16" in err()
    with pytest.raises(ptrs.PtrsError, match="tiles_y x tiles_x"):
        integ.render_aov_tiles(cam, scene, 0, 8, np.ones((2, 2), np.uint8))
    with pytest.raises(ptrs.PtrsError, match="tiles_y x tiles_x"):
        integ.render_aov_adaptive(cam, scene, np.ones((2, 2), np.uint32))


# ---- CPU: the motivating known answer ----------------------------------------------------------------------------------------------
def two_weight_film(w_left, w_right, plane_weights):
    """A 64 x 32 film of constant albedo 0.8, normal, depth and coverage, radiance noise of standard deviation 0.0578 (uniform, width
    0.2) around 0.5 x albedo, beauty weight w_left on the left half and w_right on the right; the planes carry plane_weights (H, W)."""
    H, W = 32, 64
    rng = np.random.default_rng(3)
    w = np.where(np.arange(W)[None, :] < W // 2, F32(w_left), F32(w_right)) * np.ones((H, 1), F32)
    colour = (0.4 + rng.uniform(-0.1, 0.1, (H, W, 3))).astype(F32)
    beauty = np.zeros((H, W), A.FILM_DTYPE)
    beauty["weight"], beauty["rgb"] = w, colour * w[..., None]
    pw = np.asarray(plane_weights, F32) * np.ones((H, W), F32)
    planes = {k: np.zeros((H, W), A.FILM_DTYPE) for k in NAMES}
    for k in NAMES:
        planes[k]["weight"] = pw
    planes["albedo"]["rgb"] = F32(0.8) * pw[..., None]
    planes["normal"]["rgb"] = np.array([0, 0, 1], F32) * pw[..., None]
    planes["depth"]["rgb"] = np.array([2.0, 1.0, 0.0], F32) * pw[..., None]
    return beauty, planes, colour


def test_mismatched_plane_weights_defeat_the_denoiser():
    """The two-weight film through the denoise twin (5 iterations, default sigmas).  With planes that carry the film's own weights the
    left half's standard deviation falls below a quarter of the input's (measured 0.0033 of 0.0578); with planes of weight 64
    everywhere -- render_aov at spp_done under tiles frozen at 8 -- it stays above half of it (measured 0.0576)."""
    beauty, matched, colour = two_weight_film(8, 64, np.where(np.arange(64)[None, :] < 32, 8.0, 64.0))
    _b, uniform, _c = two_weight_film(8, 64, 64.0)
    left = np.zeros((32, 64), bool)
    left[:, :32] = True
    sd_in = float(colour[left].astype(np.float64).std())
    out_m = denoise_twin.denoise(beauty, matched)["rgb"].astype(np.float64)
    out_u = denoise_twin.denoise(beauty, uniform)["rgb"].astype(np.float64)
    sd = {k: (float(o[left].std()), float(o[~left].std())) for k, o in (("matched", out_m), ("weight 64", out_u))}
    print("input standard deviation %.4f; left / right half after the filter: matched planes %.4f / %.4f, planes of weight 64 %.4f / %.4f" % (
        sd_in, sd["matched"][0], sd["matched"][1], sd["weight 64"][0], sd["weight 64"][1]))
    assert abs(sd_in - 0.0578) < 0.002
    assert sd["matched"][0] < 0.25 * sd_in
    assert sd["weight 64"][0] > 0.5 * sd_in


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def integrator(cam, name, **kw):
    (W, H), spp, depth, _r = SHAPES[name]
    if name == "stratified":
        return ptrs.PathIntegrator(ptrs.StratifiedSamplerBuilder(3, 19), depth, **kw)
    return ptrs.PathIntegrator(ptrs.SamplerBuilder(spp, cam.film.get_sample_bounds()), depth, **kw)


def as_dict(films):
    return {k: films[i] for i, k in enumerate(NAMES)}


def gpu_range(integ, cam, scene, b, e, start, samples=None):
    f = start.copy()
    integ.render_aov_range(cam, scene, b, e, samples=samples, into=as_dict(f))
    return f, integ.last_stats


def gpu_tiles(integ, cam, scene, b, e, m, start, samples=None):
    f = start.copy()
    integ.render_aov_tiles(cam, scene, b, e, m, samples=samples, into=as_dict(f))
    return f, integ.last_stats


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", list(SHAPES))
def test_device_equals_twin(orc, name, fused, tmp_path_factory):
    """k_generate_tiles -> k_aov -> k_film_aov_tiles / k_export_aov_tiles (fused 0: k_film_tiles per plane) against the twin: the range
    form and every mask of the tile form, planes, samples and statistics."""
    c = twin_case(orc, name, tmp_path_factory)
    (W, H), spp, depth, (b, e) = SHAPES[name]
    cam, scene = c["cam"], c["scene"]
    integ = integrator(cam, name)
    with ptrs.options(aov_fused_film=fused):
        s = np.full(c["dense_s"].shape, SENTINEL, F32)
        f, st = gpu_range(integ, cam, scene, b, e, c["start"], s)
        assert same(f, c["rng"]), "%s: the range form's planes differ from the twin's" % name
        assert np.array_equal(bits(s), bits(c["rng_s"])), "%s: the range form's samples differ from the twin's" % name
        assert (st.samples, st.rays_extension, st.rays_shadow, st.rays_mis) == (c["rng_st"].samples, c["rng_st"].rays_extension, 0, 0)
        for mask in MASKS:
            m = tile_mask(mask, W, H)
            s = np.full(c["dense_s"].shape, SENTINEL, F32)
            f, st = gpu_tiles(integ, cam, scene, b, e, m, c["start"], s)
            check_aov_tiles("%s %s fused %d" % (name, mask, fused), m, W, H, b, e, f, c["start"], c["rng"], s, c["dense_s"], st, c["rng_st"])
            if (m != 0).any():
                want = c["ts"].render(cam, c["p"], c["start"].copy(), sample_range=(b, e), tiles=m)
                assert (st.samples, st.rays_extension) == (want.samples, want.rays_extension), (name, mask)
                assert st.shade_launches == 0 and st.connect_launches == 0 and st.tail_launches == 0


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["lanes_1", "deal_1", "node_form_2", "paths_per_pass_900", "device_entry"])
def test_schedules_do_not_change_a_bit(orc, schedule, tmp_path_factory, tmp_path):
    """On the glTF fixture a range call and a checker-mask tile call are bit-identical under one lane, region dealing, quad nodes
    (a fresh import), 900 paths per pass (three row blocks: band mode) and through the _device entry points on a caller's stream."""
    import gltf_fixture as gf
    c = twin_case(orc, "gltf", tmp_path_factory)
    (W, H), spp, depth, (b, e) = SHAPES["gltf"]
    cam, scene = c["cam"], c["scene"]
    m = tile_mask("checker", W, H)
    px = tile_pixels(m, W, H)
    want_t = c["start"].copy()
    vt, vr = stack_values(want_t), stack_values(c["rng"])
    vt[:, px] = vr[:, px]  # the tile call's contract: the range call's bits on the active tiles, the start's elsewhere
    want_t["rgb"], want_t["weight"] = vt[..., :3], vt[..., 3]

    def both(integ, cam_, scene_):
        f, _ = gpu_range(integ, cam_, scene_, b, e, c["start"])
        t, st = gpu_tiles(integ, cam_, scene_, b, e, m, c["start"])
        return f, t, st

    opts = dict(lanes_1=dict(lanes=1), deal_1=dict(deal=1))
    if schedule in opts:
        with ptrs.options(**opts[schedule]):
            f, t, _ = both(integrator(cam, "gltf"), cam, scene)
    elif schedule == "node_form_2":
        with ptrs.options(node_form=2):
            cam2, scene2 = ptrs.import_scene(gf.write_gltf(str(tmp_path), glb=True), (W, H))
            f, t, _ = both(integrator(cam2, "gltf"), cam2, scene2)
    elif schedule == "paths_per_pass_900":
        f, t, st = both(integrator(cam, "gltf", paths_per_pass=BAND_PPP), cam, scene)
        act_rows = active_sample_pixels(m, W, H).any(axis=1)
        assert st.passes == sum(bool(act_rows[r:r + 12].any()) for r in range(0, H + 4, 12)) * (e - b)
    else:
        integ = integrator(cam, "gltf")
        stream = torch.cuda.Stream()
        out = []
        for tiles in (None, m):
            dev = {k: torch.from_numpy(stack_values(c["start"])[i].copy()).cuda() for i, k in enumerate(NAMES)}
            sdev = torch.full(((H + 4) * (W + 4) * spp * 12,), float(SENTINEL), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ptrs_ = {k: v.data_ptr() for k, v in dev.items()}
            if tiles is None:
                integ.render_aov_range_device(cam, scene, b, e, ptrs_, stream=stream.cuda_stream, samples_device_ptr=sdev.data_ptr())
            else:
                integ.render_aov_tiles_device(cam, scene, b, e, tiles, ptrs_, stream=stream.cuda_stream, samples_device_ptr=sdev.data_ptr())
            g = np.zeros((3, H, W), A.FILM_DTYPE)
            for i, k in enumerate(NAMES):
                v = dev[k].cpu().numpy()
                g[i]["rgb"], g[i]["weight"] = v[..., :3], v[..., 3]
            out.append(g)
            s = sdev.cpu().numpy().reshape(c["dense_s"].shape)
            inside = np.zeros(s.shape[:3], bool)
            inside[:, :, b:e] = True if tiles is None else active_sample_pixels(m, W, H)[..., None]
            assert np.array_equal(bits(s)[inside], bits(c["dense_s"])[inside]) and (s[~inside] == SENTINEL).all()
        f, t = out
    assert same(f, c["rng"]), schedule + ": the range call"
    assert same(t, want_t), schedule + ": the checker-mask tile call"


@pytest.mark.gpu
@pytest.mark.parametrize("ppp", [0, BAND_PPP])
def test_stale_slots_are_never_gathered(orc, ppp, tmp_path_factory):
    """A dense render_aov at other parameters first (another sample count, planes nobody keeps), so that every slot of the value arrays
    -- and at 900 paths per pass every slot of the band's arrays -- holds other values; then a centre-mask tile call: active tiles hold
    the range call's bits, inactive tiles the start's."""
    c = twin_case(orc, "cornell", tmp_path_factory)
    (W, H), spp, depth, (b, e) = SHAPES["cornell"]
    cam, scene = c["cam"], c["scene"]
    other = ptrs.PathIntegrator(ptrs.SamplerBuilder(2, cam.film.get_sample_bounds()), depth, paths_per_pass=ppp)
    other.render_aov(cam, scene)
    m = tile_mask("centre", W, H)
    integ = integrator(cam, "cornell", paths_per_pass=ppp)
    s = np.full(c["dense_s"].shape, SENTINEL, F32)
    f, st = gpu_tiles(integ, cam, scene, b, e, m, c["start"], s)
    check_aov_tiles("stale slots, paths_per_pass %d" % ppp, m, W, H, b, e, f, c["start"], c["rng"], s, c["dense_s"], st, c["rng_st"])


def mixed_target(integ, cam, scene, spp, mn):
    """The midpoint target of the uniform run's second check (test_adaptive's choice), from existing calls only."""
    blocks = ptrs.converge_schedule(spp, mn)
    half = np.zeros_like(cam.film.pixels)
    cam.film.clear()
    for k, (b, mid, e) in enumerate(blocks[:2]):
        integ.render_range(cam, scene, b, mid, half=half)
        integ.render_range(cam, scene, mid, e)
    tiles, _s = ptrs.film_error(cam.film.pixels, half)
    cam.film.clear()
    return midpoint_target(tiles["error"])


@pytest.mark.gpu
def test_adaptive_planes_end_to_end(orc, tmp_path_factory):
    """render_adaptive from a cleared film (Cornell 40 x 36, ceiling 16, min 2, the mixed target), then render_aov_adaptive(tile_spp):
    the weight bits of all three planes equal the film's, per tile the planes equal render_aov_range(0, tile_spp[t]) and the twin's;
    render_denoised(target_error, adaptive=True) equals the denoise twin fed those films; the next plain render keeps its bits and its
    hand-over round."""
    c = twin_case(orc, "cornell", tmp_path_factory)
    (W, H), spp, depth, _r = SHAPES["cornell"]
    mn = CASES["cornell"][4]
    cam, scene = c["cam"], c["scene"]
    integ = integrator(cam, "cornell")
    cam.film.clear()
    integ.render(cam, scene)  # (the scene's first render learns the survival profile)
    cam.film.clear()
    integ.render(cam, scene)
    full, tail_before = cam.film.pixels.copy(), integ.last_stats.tail_round
    target = mixed_target(integ, cam, scene, spp, mn)
    r = integ.render_adaptive(cam, scene, target, min_spp=mn)
    film = cam.film.pixels.copy()
    tile_spp = r["tile_spp"]
    counts = sorted(set(tile_spp.reshape(-1).tolist()))
    print("target %.6g, tile_spp %s" % (target, tile_spp.tolist()))
    assert len(counts) >= 2, "precondition: the target must leave tiles at two different sample counts"
    planes = integ.render_aov_adaptive(cam, scene, tile_spp, min_spp=mn)
    st = integ.last_stats
    got = np.stack([planes[k] for k in NAMES])
    for k in NAMES:
        assert np.array_equal(bits(planes[k]["weight"]), bits(film["weight"])), k
    for cnt in counts:
        ref, _ = gpu_range(integ, cam, scene, 0, cnt, np.zeros((3, H, W), A.FILM_DTYPE))
        assert same(got, ref, tile_pixels((tile_spp == cnt).astype(np.uint8), W, H)), "the tiles at %d samples are not render_aov_range(0, %d)'s" % (cnt, cnt)
    tw = np.zeros((3, H, W), A.FILM_DTYPE)
    n = c["ts"].render_adaptive(cam, c["p"], mn, tile_spp, tw)
    assert same(got, tw) and st.samples == n
    # a tile with 0 keeps its bits
    some = tile_spp.copy()
    some[-1, -1] = 0
    seeded = c["start"].copy()
    integ.render_aov_adaptive(cam, scene, some, min_spp=mn, into=as_dict(seeded))
    one = np.zeros(tile_spp.shape, np.uint8)
    one[-1, -1] = 1
    assert same(seeded, c["start"], tile_pixels(one, W, H)) and not same(seeded, c["start"], ~tile_pixels(one, W, H))
    # render_denoised on the adaptive film and its planes
    cam.film.clear()
    out = integ.render_denoised(cam, scene, target_error=target, min_spp=mn, adaptive=True)
    assert np.array_equal(bits(cam.film.pixels["rgb"]), bits(film["rgb"])) and np.array_equal(integ.last_converge["tile_spp"], tile_spp)
    want = denoise_twin.denoise(film, planes)
    assert np.array_equal(bits(out["rgb"]), bits(want["rgb"])) and (out["weight"] == 1).all()
    cam.film.clear()
    integ.render(cam, scene)
    assert np.array_equal(bits(cam.film.pixels["rgb"]), bits(full["rgb"])) and np.array_equal(bits(cam.film.pixels["weight"]), bits(full["weight"]))
    assert integ.last_stats.tail_round == tail_before
    cam.film.clear()


@pytest.mark.gpu
def test_matched_planes_help_the_denoiser():
    """Cornell 64 x 64, depth 5, ceiling 64, min 4, the mixed target; reference: 1024 spp on the device.  Over the pixels of the tiles
    frozen below the ceiling whose reference luminance is <= 1, the mean squared error of the denoised image with matched planes
    (render_aov_adaptive) is below that with the planes of render_aov at spp_done (the CLI's path before this call existed).  An
    ordering, no margin.  Measured on MI355X (tile_spp from 4 to 64, 3819 pixels): 5.362e-05 with matched planes, 5.389e-05 with the
    planes at spp_done = 64; the noisy film itself has 5.073e-05 there."""
    cam, scene = ptrs.import_scene(CORNELL, (64, 64))
    W = H = 64
    ref_integ = ptrs.PathIntegrator(ptrs.SamplerBuilder(1024, cam.film.get_sample_bounds()), 5)
    cam.film.clear()
    ref_integ.render(cam, scene)
    ref = (cam.film.pixels["rgb"] / cam.film.pixels["weight"][..., None]).astype(np.float64)
    integ = ptrs.PathIntegrator(ptrs.SamplerBuilder(64, cam.film.get_sample_bounds()), 5)
    target = mixed_target(integ, cam, scene, 64, 4)
    r = integ.render_adaptive(cam, scene, target, min_spp=4)
    film = cam.film.pixels.copy()
    cam.film.clear()
    frozen = tile_pixels((r["tile_spp"] < r["spp_done"]).astype(np.uint8), W, H)
    assert frozen.any() and not frozen.all(), "precondition: some tiles frozen below the ceiling, some not"
    matched = integ.render_aov_adaptive(cam, scene, r["tile_spp"], min_spp=4)
    at_done = ptrs.PathIntegrator(ptrs.SamplerBuilder(r["spp_done"], cam.film.get_sample_bounds()), 5).render_aov(cam, scene)
    dn = ptrs.Denoiser(W, H)
    try:
        out_m = dn.denoise(film, matched)["rgb"].astype(np.float64)
        out_u = dn.denoise(film, at_done)["rgb"].astype(np.float64)
    finally:
        dn.close()
    sel = frozen & (ref @ np.array([0.212671, 0.715160, 0.072169]) <= 1.0)
    mse = lambda img: float(((img - ref) ** 2)[sel].mean())
    noisy = (film["rgb"] / film["weight"][..., None]).astype(np.float64)
    print("tile_spp %s; MSE over %d frozen pixels: noisy %.6g, denoised with matched planes %.6g, with planes at spp_done = %d %.6g" % (
        r["tile_spp"].tolist(), int(sel.sum()), mse(noisy), mse(out_m), r["spp_done"], mse(out_u)))
    assert mse(out_m) < mse(out_u)


@pytest.mark.gpu
def test_headless_cli_adaptive_planes(tmp_path):
    """ptrs_headless --adaptive --denoise --aov takes its planes from render_aov_adaptive.  With a huge target every tile stops at
    --min_samples: the four images equal the plain -s 4 run's byte for byte (constant textures: the differential scale of the
    ceiling changes nothing).  With the mixed target denoised.png is within one code value of render_denoised(adaptive=True)."""
    from PIL import Image
    importlib.import_module("pathtracer-rs_amd.build").build_host()
    dirs = {k: tmp_path / k for k in ("plain4", "huge", "mixed")}
    for d in dirs.values():
        d.mkdir()
    base = [CLI, CORNELL, "-r", "32x32", "-d", "3", "--headless", "--denoise", "--aov"]
    subprocess.check_call(base + ["-s", "4", "-o", str(dirs["plain4"])])
    subprocess.check_call(base + ["-s", "16", "-o", str(dirs["huge"]), "--adaptive", "--target_error", "1e30", "--min_samples", "4"])
    for f in ("denoised.png", "albedo.png", "normal.png", "depth.png", "render.png"):
        assert (dirs["huge"] / f).read_bytes() == (dirs["plain4"] / f).read_bytes(), f
    cam, scene = ptrs.import_scene(CORNELL, (32, 32))
    integ = ptrs.PathIntegrator(ptrs.SamplerBuilder(16, cam.film.get_sample_bounds()), 3)
    target = mixed_target(integ, cam, scene, 16, 4)
    subprocess.check_call(base + ["-s", "16", "-o", str(dirs["mixed"]), "--adaptive", "--target_error", repr(float(target)), "--min_samples", "4"])
    out = integ.render_denoised(cam, scene, target_error=float(F32(target)), min_spp=4, adaptive=True)
    assert len(set(integ.last_converge["tile_spp"].reshape(-1).tolist())) >= 2, "precondition: tiles at two different sample counts"
    v = out["rgb"].astype(np.float64)
    srgb = np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(np.maximum(v, 0.0), 1.0 / 2.4) - 0.055)
    want = np.clip(np.floor(srgb * 255.0 + 0.5), 0, 255).astype(int)
    png = np.asarray(Image.open(str(dirs["mixed"] / "denoised.png"))).astype(int)
    assert png.shape == (32, 32, 4) and np.abs(png[..., :3] - want).max() <= 1
