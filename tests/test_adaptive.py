"""Adaptive sampling (ptrs_render_tiles, ptrs_render_adaptive): every claim is a bit comparison against code that renders
whole frames -- the range form (ptrs_render_range / the converge twin's render_range), the plain render, the oracle's samples.

On the CPU the adaptive twin (tests/adaptive_twin: the tile form of render_impl and the adaptive loop on the host twin's back end plus
the tile hooks) is held against the converge twin's range renders, the oracle's samples, and numpy restatements written here of the
dilation rule (which sample pixels a set of tiles needs) and the freeze rule.  The argument checks of the entry points call the library
and need no device.  Under -m gpu the same mask matrix runs through ptrs_render_tiles and its _device form under every schedule knob,
and ptrs_render_adaptive is held against expectations built from ptrs_render_range and ptrs_film_error alone.
"""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded: one HIP runtime per process)

from conftest import CORNELL, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "converge_twin"))
sys.path.insert(0, os.path.join(ROOT, "tests", "adaptive_twin"))
import adaptive_twin  # noqa: E402
import converge_twin  # noqa: E402

ptrs = importlib.import_module("pathtracer-rs_amd")
scenes_mod = importlib.import_module("pathtracer-rs_amd.scenes")
A = ptrs.abi
F32 = np.float32
CLI = os.path.join(ROOT, "pathtracer-rs_amd", "ptrs_headless")
INVALID, DEVICE = -1, -3
SENTINEL = F32(7.0)

# scene -> (resolution, spp, depth, the sample range of the mask tests, min_spp of the adaptive tests)
CASES = {
    "cornell": ((40, 36), 16, 5, (3, 10), 2),  # 3 x 3 tiles, clipped columns 8 wide and clipped rows 4 high; NX = 44: 64-slot chunks straddle rows
    "zoo": ((48, 32), 4, 8, (1, 4), 2),        # glass: passes that stay open for null-BSDF skips
    "stratified": ((24, 20), 9, 5, (2, 9), 0),  # 3 x 3 strata per pixel; 2 x 2 tiles, clipped
}
MASKS = ["all", "none", "centre", "corners", "checker", "row", "lastcol"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def values(f):
    return np.concatenate([f["rgb"], f["weight"][..., None]], axis=-1)


def same_px(a, b, sel):
    return np.array_equal(bits(a["rgb"])[sel], bits(b["rgb"])[sel]) and np.array_equal(bits(a["weight"])[sel], bits(b["weight"])[sel])


def same_film(a, b):
    return same_px(a, b, np.ones(a.shape, bool))


def tile_mask(name, W, H):
    ty, tx = (H + 15) // 16, (W + 15) // 16
    m = np.zeros((ty, tx), np.uint8)
    if name == "all":
        m[:] = 1
    elif name == "centre":
        m[ty // 2, tx // 2] = 1
    elif name == "corners":
        m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = 1
    elif name == "checker":
        m[(np.add.outer(np.arange(ty), np.arange(tx)) % 2) == 0] = 3  # (any non-zero byte is active)
    elif name == "row":
        m[ty // 2, :] = 1
    elif name == "lastcol":
        m[:, -1] = 1
    return m


def tile_pixels(m, W, H):
    """The pixels of the active tiles, (H, W) bool."""
    return np.repeat(np.repeat(m != 0, 16, axis=0), 16, axis=1)[:H, :W]


def active_sample_pixels(m, W, H):
    """The dilation rule restated: sample pixel (sx, sy) of the (H + 4, W + 4) grid has raster pixel (sx - 2, sy - 2) and is active iff a
    pixel of the 5 x 5 window around it lies in an active tile.  The pixel map padded by 4: the window of (sx, sy) is [sy, sy + 5) x [sx, sx + 5)."""
    pad = np.pad(tile_pixels(m, W, H), 4)
    out = np.zeros((H + 4, W + 4), bool)
    for dy in range(5):
        for dx in range(5):
            out |= pad[dy:dy + H + 4, dx:dx + W + 4]
    return out


def start_films(W, H, seed):
    """A film and a half film as a few earlier samples leave them: non-zero everywhere, different from each other."""
    rng = np.random.default_rng(seed)
    out = []
    for scale in (3.0, 1.5):
        f = np.zeros((H, W), A.FILM_DTYPE)
        f["weight"] = rng.uniform(0.5, 1.5, (H, W)).astype(F32) * F32(scale)
        f["rgb"] = rng.uniform(0.05, 0.9, (H, W, 3)).astype(F32) * f["weight"][..., None]
        out.append(f)
    return out


def make_scene(name):
    (W, H), spp, depth, _rng, _mn = CASES[name]
    if name == "zoo":
        cam, scene = scenes_mod.material_zoo((W, H))
    else:
        cam, scene = ptrs.import_scene(CORNELL, (W, H))
    return cam, scene


def twin_params(orc, name, **kw):
    (W, H), spp, depth, _rng, _mn = CASES[name]
    if name == "stratified":
        return orc.make_params(W, H, spp, depth, sampler=A.SAMPLER_STRATIFIED, n_sampled_dimensions=19, **kw)
    return orc.make_params(W, H, spp, depth, **kw)


def check_tiles_result(what, m, W, H, b, e, got_f, got_h, start_f, start_h, ref_f, ref_h, samples, ref_samples, n_samples, ref_stats, stats):
    """The contract of ptrs_render_tiles on one mask: active tiles hold the range render's bits, inactive tiles the start's, in both
    films; the sample export holds the reference's values on the active sample pixels inside the range and the sentinel elsewhere; the
    sample count is the numpy count; the rays are at most the full range's (equal with every tile active)."""
    px = tile_pixels(m, W, H)
    act = active_sample_pixels(m, W, H)
    assert same_px(got_f, ref_f, px), what + ": an active tile's film pixels differ from the range render's"
    assert same_px(got_f, start_f, ~px), what + ": an inactive tile's film pixels changed"
    if got_h is not None:
        assert same_px(got_h, ref_h, px), what + ": an active tile's half-film pixels differ from the range render's"
        assert same_px(got_h, start_h, ~px), what + ": an inactive tile's half-film pixels changed"
    if samples is not None:
        inside = np.zeros(samples.shape[:3], bool)
        inside[:, :, b:e] = act[..., None]
        assert np.array_equal(bits(samples)[inside], bits(ref_samples)[inside]), what + ": exported samples of active sample pixels differ"
        assert (samples[~inside] == SENTINEL).all(), what + ": an entry outside the active sample pixels / the range was written"
    assert n_samples == int(act.sum()) * (e - b), (what, n_samples, int(act.sum()) * (e - b))
    rays, ref_rays = (stats.rays_extension, stats.rays_shadow, stats.rays_mis), (ref_stats.rays_extension, ref_stats.rays_shadow, ref_stats.rays_mis)
    assert all(r <= q for r, q in zip(rays, ref_rays)), (what, rays, ref_rays)
    if (m != 0).all():
        assert rays == ref_rays and n_samples == ref_stats.samples, what
    if not (m != 0).any():
        assert rays == (0, 0, 0) and stats.passes == 0 and stats.kernel_launches == 0, what


# ---- CPU: the numpy restatement itself, on shapes whose answer is known ---------------------------------------------------------------
def test_dilation_restatement_known_answers():
    assert active_sample_pixels(tile_mask("all", 40, 36), 40, 36).all()
    assert not active_sample_pixels(tile_mask("none", 40, 36), 40, 36).any()
    c = active_sample_pixels(tile_mask("centre", 40, 36), 40, 36)  # tile (1, 1): pixels 16..31 both ways -> raster 14..33 -> grid 16..35
    assert c.sum() == 20 * 20 and c[16:36, 16:36].all()
    lc = active_sample_pixels(tile_mask("lastcol", 40, 36), 40, 36)  # pixels x 32..39, every row: raster x 30..41 -> grid 32..43, all 40 rows
    assert lc.sum() == 12 * 40 and lc[:, 32:].all()
    k = active_sample_pixels(tile_mask("corners", 40, 36), 40, 36)  # adjacent aprons overlap nowhere here: 20 x 20, 12 x 20, 20 x 8, 12 x 8
    assert k.sum() == 20 * 20 + 12 * 20 + 20 * 8 + 12 * 8


# ---- CPU: the freeze rule -----------------------------------------------------------------------------------------------------------------
def freeze_np(tiles, target, active):
    nxt = ((active != 0) & ~(tiles["error"] < F32(target))).astype(np.uint8)
    return nxt, int(nxt.sum())


def test_freeze_rule_against_numpy():
    L = ptrs.load_library()
    rng = np.random.default_rng(5)
    for n in (1, 9, 257):
        t = np.zeros(n, A.TILE_DTYPE)
        t["error"] = rng.uniform(0.0, 0.2, n).astype(F32)
        t["valid"] = rng.integers(1, 257, n)
        target = float(np.median(t["error"]))  # (with n odd: one tile's error EQUALS the target, and is not frozen)
        t["error"][::7] = F32(target)
        t["error"][3::11] = np.inf
        t[5::13] = (0.0, 0)  # tiles without a valid pixel: error 0
        for active in (np.ones(n, np.uint8), (rng.random(n) < 0.6).astype(np.uint8) * 200):
            for tg in (target, 0.0, 1e30):
                want, n_want = freeze_np(t, tg, active)
                got, n_got = adaptive_twin.freeze(t, tg, active)
                assert np.array_equal(got, want) and n_got == n_want
                lib_next, lib_n = np.full(n, 9, np.uint8), C.c_uint32(77)
                assert L.ptrs_adaptive_freeze(t.ctypes.data, n, tg, np.ascontiguousarray(active).ctypes.data, lib_next.ctypes.data, C.addressof(lib_n)) == 0
                assert np.array_equal(lib_next, want) and lib_n.value == n_want
                if tg == 0.0:
                    assert np.array_equal(got, (active != 0).astype(np.uint8))  # a target of 0 freezes nothing
                inf = np.isinf(t["error"])
                assert (got[inf] == (active[inf] != 0)).all()  # a non-finite tile never freezes
                assert (got[t["error"] == F32(tg)] == (active[t["error"] == F32(tg)] != 0)).all()  # equal to the target: stays active
                if tg > 0.0:
                    assert not got[t["valid"] == 0].any()  # no valid pixel: error 0, frozen under any positive target
    # monotonic: over a run of checks with errors that go up and down, a tile once frozen never comes back
    n = 64
    active = np.ones(n, np.uint8)
    seen_frozen = np.zeros(n, bool)
    for k in range(8):
        t = np.zeros(n, A.TILE_DTYPE)
        t["error"], t["valid"] = rng.uniform(0.0, 0.2, n).astype(F32), 256
        active, cnt = adaptive_twin.freeze(t, 0.05, active)
        assert not active[seen_frozen].any() and cnt == int(active.sum())
        seen_frozen |= active == 0
    assert seen_frozen.sum() > n // 2 and L.ptrs_adaptive_freeze(None, 0, 0.1, None, None, None) == INVALID and b"null" in L.ptrs_last_error()


# ---- CPU: the tile form on the twin ---------------------------------------------------------------------------------------------------
_twin_cases = {}


def twin_case(orc, name):
    """Made once per scene: camera, scene, params, the oracle's samples, the start films, the converge twin's range render on them."""
    if name not in _twin_cases:
        (W, H), spp, depth, (b, e), _mn = CASES[name]
        cam, scene = make_scene(name)
        p = twin_params(orc, name)
        _fo, so, _sto = orc.OracleScene(scene).render(cam, p, n_threads=4, want_samples=True)
        start_f, start_h = start_films(W, H, 11)
        ref_f, ref_h = start_f.copy(), start_h.copy()
        rs = converge_twin.RangeScene(scene)
        _, ref_st = rs.render_range(cam, p, b, e, film=ref_f, half=ref_h)
        _twin_cases[name] = dict(cam=cam, scene=scene, p=p, so=so, start=(start_f, start_h), ref=(ref_f, ref_h), ref_st=ref_st, rs=rs, ts=adaptive_twin.TileScene(scene))
    return _twin_cases[name]


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("name", list(CASES))
def test_twin_tiles_equal_the_range_render(orc, name, mask):
    c = twin_case(orc, name)
    (W, H), spp, depth, (b, e), _mn = CASES[name]
    m = tile_mask(mask, W, H)
    f, h = c["start"][0].copy(), c["start"][1].copy()
    samples = np.full(c["so"].shape, SENTINEL, F32)
    st = c["ts"].render_tiles(c["cam"], c["p"], b, e, m, f, half=h, samples=samples)
    check_tiles_result("%s %s" % (name, mask), m, W, H, b, e, f, h, c["start"][0], c["start"][1], c["ref"][0], c["ref"][1], samples, c["so"], st.samples, c["ref_st"], st)


def test_twin_tiles_sample_chunks_and_row_splits(orc):
    """paths_per_pass of two samples: the same bits (and a pass per chunk).  A plan that splits the rows is held to the range form's 1e-6
    on the active tiles, and still changes no bit of an inactive one; passes whose rows hold no active sample pixel are not run."""
    c = twin_case(orc, "cornell")
    (W, H), spp, depth, (b, e), _mn = CASES["cornell"]
    for mask in ("checker", "lastcol", "row"):
        m = tile_mask(mask, W, H)
        px = tile_pixels(m, W, H)
        chunks = twin_params(orc, "cornell", paths_per_pass=(W + 4) * (H + 4) * 2)
        f, h = c["start"][0].copy(), c["start"][1].copy()
        st = c["ts"].render_tiles(c["cam"], chunks, b, e, m, f, half=h)
        assert st.passes == (e - b + 1) // 2 and st.samples == int(active_sample_pixels(m, W, H).sum()) * (e - b)
        assert same_px(f, c["ref"][0], px) and same_px(f, c["start"][0], ~px) and same_px(h, c["ref"][1], px) and same_px(h, c["start"][1], ~px), mask
        rows = twin_params(orc, "cornell", paths_per_pass=(W + 4) * 5)  # five sample rows per pass: tiles straddle the passes' first rows
        f = c["start"][0].copy()
        st = c["ts"].render_tiles(c["cam"], rows, b, e, m, f)
        act_rows = active_sample_pixels(m, W, H).any(axis=1)
        assert st.passes == sum(bool(act_rows[r:r + 5].any()) for r in range(0, H + 4, 5)) * (e - b), mask
        assert st.samples == int(active_sample_pixels(m, W, H).sum()) * (e - b)
        add, ref_add = values(f).astype(np.float64) - values(c["start"][0]), values(c["ref"][0]).astype(np.float64) - values(c["start"][0])
        rel = np.sqrt(((add - ref_add)[px] ** 2).sum() / (ref_add[px] ** 2).sum())
        print(mask, "row-split plan: relative difference of the added light on the active tiles %.3g" % rel)
        assert rel < 1e-6 and same_px(f, c["start"][0], ~px), mask


# ---- CPU: the adaptive loop on the twin -----------------------------------------------------------------------------------------------
def first_below(errors, target, schedule, spp):
    """tile_spp as the contract states it: the first schedule point at which the UNIFORM run's error of the tile is below the target, or spp."""
    out = np.full(errors.shape[1:], spp, np.uint32)
    for t in np.ndindex(out.shape):
        for k, n in enumerate(schedule):
            if errors[(k,) + t] < F32(target):
                out[t] = n
                break
    return out


def midpoint_target(errors_check2):
    """A target between two distinct tile errors of the second check: the midpoint of the middle pair of the sorted distinct errors."""
    e = np.unique(errors_check2.reshape(-1))
    assert e.size >= 2
    i = e.size // 2 - 1
    return 0.5 * (float(e[i]) + float(e[i + 1]))


def test_twin_adaptive_loop(orc):
    c = twin_case(orc, "cornell")
    (W, H), spp, depth, _rng, mn = CASES["cornell"]
    cam, p, ts, rs = c["cam"], c["p"], c["ts"], c["rs"]
    schedule = [e for (_b, _m, e) in ptrs.converge_schedule(spp, mn)]
    uni = ts.render_adaptive(cam, p, 0.0, mn)  # nothing freezes: the uniform run, with its tile errors at every check
    n_tiles = uni["tile_spp"].size
    full = np.zeros((H, W), A.FILM_DTYPE)
    rs.render_range(cam, p, 0, spp, film=full)
    assert same_film(uni["film"], full) and (uni["tile_spp"] == spp).all() and not uni["converged"]
    assert [(n, a) for n, a, _ in uni["history"]] == [(n, n_tiles) for n in schedule] and uni["samples"] == (W + 4) * (H + 4) * spp
    E = uni["tile_errors"]["error"]
    target = midpoint_target(E[1])
    want_spp = first_below(E, target, schedule, spp)
    frozen_at = set(int(n) for t, n in np.ndenumerate(want_spp) if (E[schedule.index(n)][t] < F32(target)))
    to_ceiling = [t for t, n in np.ndenumerate(want_spp) if n == spp and not (E[:-1, t[0], t[1]] < F32(target)).any()]
    print("target %.6g, tile_spp %s, tiles freeze at checks %s, %d tiles active to the ceiling" % (target, want_spp.tolist(), sorted(frozen_at), len(to_ceiling)))
    assert len(frozen_at) >= 2 and len(to_ceiling) >= 1, "precondition: the target must freeze tiles at two different checks and leave one active to the ceiling"
    r = ts.render_adaptive(cam, p, target, mn)
    assert np.array_equal(r["tile_spp"], want_spp)
    films = {}
    for n in sorted(set(want_spp.reshape(-1).tolist())):
        films[n] = np.zeros((H, W), A.FILM_DTYPE)
        rs.render_range(cam, p, 0, n, film=films[n])
    want_samples = 0
    for k, n in enumerate(schedule):
        m = (want_spp >= n).astype(np.uint8)
        assert r["history"][k][:2] == (n, int(m.sum()))
        want_samples += int(active_sample_pixels(m, W, H).sum()) * (n - (schedule[k - 1] if k else 0))
        for t in np.ndindex(want_spp.shape):  # an active tile's error is the uniform run's; a frozen tile's error is the one it froze with
            k_last = min(k, schedule.index(want_spp[t]))
            assert bits(r["tile_errors"]["error"][k][t]) == bits(E[k_last][t]), (k, t)
    assert r["samples"] == want_samples and r["samples"] < uni["samples"]
    for t, n in np.ndenumerate(want_spp):
        one = np.zeros(want_spp.shape, np.uint8)
        one[t] = 1
        assert same_px(r["film"], films[int(n)], tile_pixels(one, W, H)), "tile %s is not render_range(0, %d)'s" % (t, n)
    tiles, s = adaptive_twin.film_error(r["film"], r["half"])
    assert bits(F32(r["history"][-1][2])) == bits(F32(s.max_tile_error)) and r["converged"] == bool(s.max_tile_error < F32(target)) and not r["converged"]
    huge = ts.render_adaptive(cam, p, 1e30, mn)
    at_min = np.zeros((H, W), A.FILM_DTYPE)
    rs.render_range(cam, p, 0, mn, film=at_min)
    assert huge["converged"] and len(huge["history"]) == 1 and (huge["tile_spp"] == mn).all() and same_film(huge["film"], at_min)


# ---- CPU: argument checks that need no device ---------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments():
    """ptrs_render_tiles(_device) and ptrs_render_adaptive refuse bad arguments before their first device call (this test never reaches
    one: every call here is refused, or -- without a GPU -- ends at "no HIP device")."""
    L = ptrs.load_library()
    assert L.ptrs_abi_version() == 4
    assert (L.ptrs_abi_sizeof(15), L.ptrs_abi_sizeof(16)) == (C.sizeof(A.PtrsAdaptiveCheck), C.sizeof(A.PtrsAdaptiveResult)) == (12, 24 + 12 * 32)
    assert (L.ptrs_abi_sizeof(8), L.ptrs_abi_sizeof(14)) == (C.sizeof(A.PtrsStats), 16 + 8 * 32)  # (no existing struct changed)
    f, h = start_films(8, 8, 0)
    fp, hp = f.ctypes.data, h.ctypes.data
    cam, _scene = ptrs.import_scene(CORNELL, (8, 8))
    integ = ptrs.PathIntegrator(ptrs.SamplerBuilder(8, cam.film.get_sample_bounds()), 2)
    p, cabi = integ.params(cam), cam.to_abi()
    fake = C.addressof((C.c_char * 64)())
    pp, cp = C.addressof(p), C.addressof(cabi)
    st = A.PtrsStats()
    one = np.ones(1, np.uint8)
    tp = one.ctypes.data
    for fn, tail in ((L.ptrs_render_tiles, (None, None)), (L.ptrs_render_tiles_device, (None, None))):
        call = lambda scene, cam_, prm, b, e, tl, fl, hf: fn(scene, cam_, prm, b, e, tl, fl, hf, *tail)
        assert call(None, cp, pp, 0, 8, tp, fp, None) == INVALID and b"null" in L.ptrs_last_error()
        assert call(fake, None, pp, 0, 8, tp, fp, None) == INVALID and b"null" in L.ptrs_last_error()
        assert call(fake, cp, None, 0, 8, tp, fp, None) == INVALID and b"null" in L.ptrs_last_error()
        assert call(fake, cp, pp, 0, 8, None, fp, None) == INVALID and b"null" in L.ptrs_last_error()
        assert call(fake, cp, pp, 0, 8, tp, None, None) == INVALID and b"null" in L.ptrs_last_error()
        for (b, e) in ((0, 0), (3, 3), (5, 4), (0, 9), (8, 9), (8, 8), (0xffffffff, 1)):
            assert call(fake, cp, pp, b, e, tp, fp, None) == INVALID and b"sample range" in L.ptrs_last_error(), (b, e)
        assert call(fake, cp, pp, 0, 8, tp, fp, fp) == INVALID and b"half film" in L.ptrs_last_error()
        pb = integ.params(cam)
        pb.row_begin, pb.row_end = 2, 6
        assert call(fake, cp, C.addressof(pb), 0, 8, tp, fp, None) == INVALID and b"whole film" in L.ptrs_last_error()
        if not torch.cuda.is_available():
            assert call(fake, cp, pp, 0, 8, tp, fp, hp) == DEVICE and b"no HIP device" in L.ptrs_last_error()
    res = A.PtrsAdaptiveResult()
    spp_out = np.zeros(1, np.uint32)
    adp = lambda scene, prm, target, mn, fl, r: L.ptrs_render_adaptive(scene, cp, prm, target, mn, fl, None, spp_out.ctypes.data, r, C.addressof(st))
    assert adp(None, pp, 0.1, 2, fp, C.addressof(res)) == INVALID and b"null" in L.ptrs_last_error()
    assert adp(fake, pp, 0.1, 2, None, C.addressof(res)) == INVALID and b"null" in L.ptrs_last_error()
    assert adp(fake, pp, 0.1, 2, fp, None) == INVALID and b"null" in L.ptrs_last_error()
    for target in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert adp(fake, pp, target, 2, fp, C.addressof(res)) == INVALID and b"target_error" in L.ptrs_last_error()
    for mn in (0, 1, 3, 16):
        assert adp(fake, pp, 0.1, mn, fp, C.addressof(res)) == INVALID and b"min_spp" in L.ptrs_last_error()
    pb = integ.params(cam)
    pb.row_begin, pb.row_end = 2, 6
    assert adp(fake, C.addressof(pb), 0.1, 2, fp, C.addressof(res)) == INVALID and b"whole film" in L.ptrs_last_error()
    if not torch.cuda.is_available():
        assert adp(fake, pp, 0.1, 2, fp, C.addressof(res)) == DEVICE and b"no HIP device" in L.ptrs_last_error()
    with pytest.raises(ptrs.PtrsError, match="tiles_y x tiles_x"):
        integ.render_tiles(cam, _scene, 0, 8, np.ones((2, 2), np.uint8))


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def integrator(cam, name, **kw):
    (W, H), spp, depth, _rng, _mn = CASES[name]
    if name == "stratified":
        return ptrs.PathIntegrator(ptrs.StratifiedSamplerBuilder(3, 19), depth, **kw)
    return ptrs.PathIntegrator(ptrs.SamplerBuilder(spp, cam.film.get_sample_bounds()), depth, **kw)


_gpu_cases = {}


def gpu_case(name):
    """Made once per scene on the device: the start films, ptrs_render_range on them, ptrs_render_samples' samples."""
    if name not in _gpu_cases:
        (W, H), spp, depth, (b, e), _mn = CASES[name]
        cam, scene = make_scene(name)
        integ = integrator(cam, name)
        integ.render(cam, scene)  # (the scene's first render learns the survival profile the next ones use)
        cam.film.clear()
        so = integ.render(cam, scene, want_samples=True)
        start_f, start_h = start_films(W, H, 11)
        cam.film.pixels[...] = start_f
        ref_h = start_h.copy()
        ref_st = integ.render_range(cam, scene, b, e, half=ref_h)
        ref_f = cam.film.pixels.copy()
        cam.film.clear()
        _gpu_cases[name] = dict(cam=cam, scene=scene, integ=integ, so=so, start=(start_f, start_h), ref=(ref_f, ref_h), ref_st=ref_st)
    return _gpu_cases[name]


def gpu_tiles_check(c, name, mask, integ, what, expect=None):
    (W, H), spp, depth, (b, e), _mn = CASES[name]
    cam, scene = c["cam"], c["scene"]
    m = tile_mask(mask, W, H)
    cam.film.pixels[...] = c["start"][0]
    h = c["start"][1].copy()
    samples = np.full(c["so"].shape, SENTINEL, F32)
    st = integ.render_tiles(cam, scene, b, e, m, half=h, samples=samples)
    check_tiles_result("%s %s %s" % (name, mask, what), m, W, H, b, e, cam.film.pixels, h, c["start"][0], c["start"][1], c["ref"][0], c["ref"][1], samples, c["so"], st.samples, c["ref_st"], st)
    if expect and (m != 0).any():
        expect(st)
    cam.film.clear()
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("name", list(CASES))
def test_device_tiles_equal_the_range_render(name, mask):
    """ptrs_render_tiles on host films against ptrs_render_range / ptrs_render_samples on the device, bit for bit."""
    c = gpu_case(name)
    gpu_tiles_check(c, name, mask, c["integ"], "host films")


@pytest.mark.gpu
@pytest.mark.parametrize("mask", MASKS)
def test_device_tiles_device_form(mask):
    """ptrs_render_tiles_device: torch films, a stream of the caller's."""
    c = gpu_case("cornell")
    (W, H), spp, depth, (b, e), _mn = CASES["cornell"]
    m = tile_mask(mask, W, H)
    tf, th = torch.from_numpy(values(c["start"][0]).copy()).cuda(), torch.from_numpy(values(c["start"][1]).copy()).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    st = c["integ"].render_tiles_device(c["cam"], c["scene"], b, e, m, tf.data_ptr(), th.data_ptr(), stream=stream.cuda_stream)
    gf, gh = np.zeros((H, W), A.FILM_DTYPE), np.zeros((H, W), A.FILM_DTYPE)
    for g, t in ((gf, tf), (gh, th)):
        v = t.cpu().numpy()
        g["rgb"], g["weight"] = v[..., :3], v[..., 3]
    check_tiles_result("cornell %s device form" % mask, m, W, H, b, e, gf, gh, c["start"][0], c["start"][1], c["ref"][0], c["ref"][1], None, None, st.samples, c["ref_st"], st)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "zoo"])
def test_device_tiles_under_every_schedule_knob(name):
    """Lanes 1 and 4, the fused tail off, forced at round 2 (the Cornell box has an instantiation), two-sample chunks: the same bits."""
    c = gpu_case(name)
    (W, H), spp, depth, (b, e), _mn = CASES[name]
    masks = ("checker", "corners", "lastcol", "all")
    for lanes in (1, 4):
        def lanes_are(st, lanes=lanes):
            assert st.lanes == lanes
        with ptrs.options(lanes=lanes):
            for mask in masks:
                gpu_tiles_check(c, name, mask, c["integ"], "lanes %d" % lanes, lanes_are)
    chunked = integrator(c["cam"], name, paths_per_pass=(W + 4) * (H + 4) * 2)

    def passes_are(st):
        assert st.passes == (e - b + 1) // 2
    for lanes in (1, 4):
        with ptrs.options(lanes=lanes):
            for mask in masks:
                gpu_tiles_check(c, name, mask, chunked, "chunks of two samples, lanes %d" % lanes, passes_are)

    def no_tail(st):
        assert st.tail_launches == 0

    def tail_at_2(st):
        assert st.tail_launches == st.passes and st.tail_round == 2, "the scene has no fused-tail instantiation"
    with ptrs.options(tail=0):
        for mask in masks:
            gpu_tiles_check(c, name, mask, c["integ"], "tail off", no_tail)
    if name == "cornell":
        with ptrs.options(tail_at=2):
            for mask in masks:
                gpu_tiles_check(c, name, mask, c["integ"], "tail at 2", tail_at_2)


@pytest.mark.gpu
def test_device_tiles_row_split_plan():
    """A plan that splits the rows (five sample rows per pass: film tiles straddle the passes' first rows): held to the range form's
    1e-6 on the active tiles, no bit of an inactive tile changes, passes without an active sample pixel are not run."""
    c = gpu_case("cornell")
    (W, H), spp, depth, (b, e), _mn = CASES["cornell"]
    cam, scene = c["cam"], c["scene"]
    rows = integrator(cam, "cornell", paths_per_pass=(W + 4) * 5)
    for mask in ("checker", "row", "lastcol"):
        m = tile_mask(mask, W, H)
        px, act = tile_pixels(m, W, H), active_sample_pixels(m, W, H)
        cam.film.pixels[...] = c["start"][0]
        st = rows.render_tiles(cam, scene, b, e, m)
        f = cam.film.pixels.copy()
        cam.film.clear()
        assert st.samples == int(act.sum()) * (e - b)
        assert st.passes == sum(bool(act[r:r + 5].any()) for r in range(0, H + 4, 5)) * (e - b), mask
        add, ref_add = values(f).astype(np.float64) - values(c["start"][0]), values(c["ref"][0]).astype(np.float64) - values(c["start"][0])
        rel = np.sqrt(((add - ref_add)[px] ** 2).sum() / (ref_add[px] ** 2).sum())
        print(mask, "row-split plan: relative difference of the added light on the active tiles %.3g" % rel)
        assert rel < 1e-6 and same_px(f, c["start"][0], ~px), mask


@pytest.mark.gpu
def test_render_adaptive_against_the_uniform_run():
    """ptrs_render_adaptive against expectations built from existing calls only: the uniform run block by block (render_range into film
    and half film by the schedule, film_error behind every block) gives every tile's error at every check and the film at every
    schedule point; from those follow tile_spp, the per-tile film bits, the tiles active per block and the samples traced."""
    (W, H), spp, depth, _rng, mn = CASES["cornell"]
    cam, scene = make_scene("cornell")
    integ = integrator(cam, "cornell")
    integ.render(cam, scene)
    cam.film.clear()
    integ.render(cam, scene)
    full, tail_before = cam.film.pixels.copy(), integ.last_stats.tail_round
    cam.film.clear()
    blocks = ptrs.converge_schedule(spp, mn)
    schedule = [e for (_b, _m, e) in blocks]
    half = np.zeros_like(full)
    E, films, uniform_samples = [], {}, 0
    for (b, mid, e) in blocks:
        uniform_samples += integ.render_range(cam, scene, b, mid, half=half).samples
        uniform_samples += integ.render_range(cam, scene, mid, e).samples
        films[e] = cam.film.pixels.copy()
        tiles, _s = ptrs.film_error(cam.film.pixels, half)
        E.append(tiles["error"].copy())
    assert same_film(cam.film.pixels, full)
    cam.film.clear()
    E = np.stack(E)
    target = midpoint_target(E[1])
    want_spp = first_below(E, target, schedule, spp)
    frozen_at = set(int(n) for t, n in np.ndenumerate(want_spp) if (E[schedule.index(n)][t] < F32(target)))
    print("target %.6g, expected tile_spp %s" % (target, want_spp.tolist()))
    assert len(frozen_at) >= 2 and (want_spp == spp).any(), "precondition: tiles freeze at two different checks, one stays active to the ceiling"
    r = integ.render_adaptive(cam, scene, target, min_spp=mn, want_half=True)
    st = integ.last_stats
    got = cam.film.pixels.copy()
    cam.film.clear()
    print("history", r["history"], "tile_spp", r["tile_spp"].tolist())
    assert np.array_equal(r["tile_spp"], want_spp) and r["spp_done"] == spp and not r["converged"]
    want_samples = 0
    for k, n in enumerate(schedule):
        m = (want_spp >= n).astype(np.uint8)
        assert r["history"][k][:2] == (n, int(m.sum())), k
        want_samples += int(active_sample_pixels(m, W, H).sum()) * (n - (schedule[k - 1] if k else 0))
    for t, n in np.ndenumerate(want_spp):
        one = np.zeros(want_spp.shape, np.uint8)
        one[t] = 1
        assert same_px(got, films[int(n)], tile_pixels(one, W, H)), "tile %s is not render_range(0, %d)'s" % (t, n)
    _, s = converge_twin.film_error(got, r["half"])
    assert bits(F32(r["history"][-1][2])) == bits(F32(s.max_tile_error)) and r["worst_tile"] == s.worst_tile
    assert st.samples == want_samples and st.samples < uniform_samples, (st.samples, want_samples, uniform_samples)
    # the ends of the target's range
    r0 = integ.render_adaptive(cam, scene, 0.0, min_spp=mn)
    assert same_film(cam.film.pixels, full) and (r0["tile_spp"] == spp).all() and not r0["converged"] and integ.last_stats.samples == uniform_samples
    assert [(n, a) for n, a, _ in r0["history"]] == [(n, want_spp.size) for n in schedule]
    assert [bits(F32(e)) for _, _, e in r0["history"]] == [bits(E[k].max()) for k in range(len(schedule))]
    cam.film.clear()
    rh = integ.render_adaptive(cam, scene, 1e30, min_spp=mn)
    assert same_film(cam.film.pixels, films[mn]) and rh["converged"] and rh["spp_done"] == mn and len(rh["history"]) == 1 and (rh["tile_spp"] == mn).all()
    cam.film.clear()
    # the plain render afterwards: the same bits, the same hand-over to the tail -- the masked passes left the survival profile alone
    integ.render(cam, scene)
    assert same_film(cam.film.pixels, full) and integ.last_stats.tail_round == tail_before
    cam.film.clear()


@pytest.mark.gpu
def test_headless_cli_renders_adaptively(tmp_path):
    """ptrs_headless --adaptive: a target of 0 gives the plain render's render.png, a huge one that of --min_samples samples;
    samples.png is written; without --target_error the flag is refused."""
    importlib.import_module("pathtracer-rs_amd.build").build_host()
    dirs = {k: tmp_path / k for k in ("plain16", "plain4", "zero", "huge", "bad")}
    for d in dirs.values():
        d.mkdir()
    base = [CLI, CORNELL, "-r", "40x36", "-d", "3", "--headless"]
    subprocess.check_call(base + ["-s", "16", "-o", str(dirs["plain16"])])
    subprocess.check_call(base + ["-s", "4", "-o", str(dirs["plain4"])])
    zero = subprocess.run(base + ["-s", "16", "-o", str(dirs["zero"]), "--adaptive", "--target_error", "0", "--min_samples", "4"], check=True, capture_output=True, text=True).stderr
    huge = subprocess.run(base + ["-s", "16", "-o", str(dirs["huge"]), "--adaptive", "--target_error", "1e30", "--min_samples", "4"], check=True, capture_output=True, text=True).stderr
    assert re.findall(r"INFO check \d+: (\d+) spp, (\d+) of (\d+) tiles active, worst", zero) == [("4", "9", "9"), ("8", "9", "9"), ("16", "9", "9")]
    assert "INFO stopped at 16 spp (ceiling reached" in zero
    assert re.findall(r"INFO check \d+: (\d+) spp, (\d+) of (\d+) tiles active, worst", huge) == [("4", "9", "9")] and "INFO stopped at 4 spp (converged" in huge
    assert (dirs["zero"] / "render.png").read_bytes() == (dirs["plain16"] / "render.png").read_bytes()
    assert (dirs["huge"] / "render.png").read_bytes() == (dirs["plain4"] / "render.png").read_bytes()
    assert (dirs["zero"] / "samples.png").exists() and (dirs["huge"] / "samples.png").exists()
    bad = subprocess.run(base + ["-s", "16", "-o", str(dirs["bad"]), "--adaptive"], capture_output=True, text=True)
    assert bad.returncode != 0 and "--target_error" in bad.stderr and not (dirs["bad"] / "render.png").exists()
