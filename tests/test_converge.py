"""Sample ranges, the film's error and rendering until it has converged (ptrs_render_range, ptrs_film_error, ptrs_render_converged;
DESIGN 12) against answers from outside them.

On the CPU the converge twin (tests/converge_twin: pt_converge.h for the host over whole images, and the range form of render_impl on
the host twin's back end) is held against a float64 numpy restatement of the error contract written here, against the schedule's
properties, and -- the ranges -- against the full twin render and the oracle, bit for bit.  The argument checks of the entry points
call the library and need no device.  Under -m gpu the device must equal the twin on every tile record and the summary, chained range
renders must equal ptrs_render bit for bit under every schedule knob, and render_converged must stop where its history says.
"""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded: the library then runs on the HIP runtime torch brings along, and the process has one)

from conftest import CORNELL, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "converge_twin"))
import converge_twin  # noqa: E402
import twin  # noqa: E402

ptrs = importlib.import_module("pathtracer-rs_amd")
scenes_mod = importlib.import_module("pathtracer-rs_amd.scenes")
A = ptrs.abi
F32 = np.float32
CLI = os.path.join(ROOT, "pathtracer-rs_amd", "ptrs_headless")
INVALID, UNSUPPORTED, DEVICE = -1, -2, -3

# Twin against the float64 restatement: tile errors and the summary's maximum, relative to the float64 value.  Measured over every
# input of test_error_twin_against_float64 (1x1, 16x16, 17x33, 37x29, 64x48; with and without empty, half-only-empty and non-finite
# pixels; half films 5 % to 50 % away from the film): worst 1.12e-6, on the 17x33 input whose half film is 5 % away (its clipped tiles
# hold a column of pixels, and I - A cancels twenty-fold there); 6.16e-7 on the 1x1 input, at most 2.5e-7 elsewhere.  The bound is
# 8 x the worst, rounded up to a power of two.
TWIN_VS_F64 = 2.0 ** -16
ERROR_SIZES = [(1, 1), (16, 16), (17, 33), (37, 29)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def values(f):
    return np.concatenate([f["rgb"], f["weight"][..., None]], axis=-1)


def same_film(a, b):
    return np.array_equal(bits(a["rgb"]), bits(b["rgb"])) and np.array_equal(bits(a["weight"]), bits(b["weight"]))


def film(rgb, weight):
    f = np.zeros(weight.shape, A.FILM_DTYPE)
    f["rgb"], f["weight"] = rgb.astype(F32), weight.astype(F32)
    return f


def synthetic(W, H, seed=0, holes=True, bad=True, spread=0.3):
    """Two accumulated films as a render leaves them: weights around 4 and 2, a smooth colour, the half film's colour `spread` away
    from the film's; with `holes` some pixels empty in both films and some in the half film only, with `bad` one non-finite pixel."""
    rng = np.random.default_rng(1000 * W + H + seed)
    y, x = np.mgrid[0:H, 0:W]
    colour = np.stack([0.3 + 0.25 * np.sin(0.31 * x + 0.2 * y), 0.25 + 0.2 * np.cos(0.17 * x - 0.4 * y), 0.05 + 0.04 * np.sin(0.5 * x * y)], axis=-1)
    colour = np.abs(colour * rng.uniform(0.7, 1.3, (H, W, 1)))
    wf, wh = rng.uniform(3.0, 5.0, (H, W)), rng.uniform(1.5, 2.5, (H, W))
    ch = colour * rng.uniform(1.0 - spread, 1.0 + spread, (H, W, 3))
    f, h = film(colour * wf[..., None], wf), film(ch * wh[..., None], wh)
    if holes and W * H > 1:
        empty, half_empty = rng.random((H, W)) < 0.08, rng.random((H, W)) < 0.08
        f[empty] = 0
        h[empty | half_empty] = 0
    if bad:
        by, bx = H // 2, W // 3
        f[by, bx] = ((np.inf, 1.0, 1.0), 2.0)
        h[by, bx] = ((0.5, 0.5, 0.5), 1.0)
    return f, h


def error_f64(f, h):
    """The contract of ptrs_film_error restated in float64: (tile errors (ty, tx), tile counts, max, worst tile, valid pixels)."""
    H, W = f.shape
    fw, hw = f["weight"].astype(np.float64), h["weight"].astype(np.float64)
    valid = (fw > 0) & (hw > 0)
    with np.errstate(all="ignore"):
        I = f["rgb"].astype(np.float64) / np.where(valid, fw, 1.0)[..., None]
        Ah = h["rgb"].astype(np.float64) / np.where(valid, hw, 1.0)[..., None]
        d = np.abs(I - Ah).sum(axis=-1)
        e = d / np.sqrt(np.fmax(I.sum(axis=-1), 1e-3))
    e = np.where(np.isfinite(e), e, np.inf)
    e = np.where(valid, e, 0.0)
    ty, tx = (H + 15) // 16, (W + 15) // 16
    err, cnt = np.zeros((ty, tx)), np.zeros((ty, tx), dtype=np.int64)
    for j in range(ty):
        for i in range(tx):
            sl = (slice(16 * j, 16 * j + 16), slice(16 * i, 16 * i + 16))
            cnt[j, i] = valid[sl].sum()
            err[j, i] = e[sl].sum() / cnt[j, i] if cnt[j, i] else 0.0
    return err, cnt, err.max(), int(np.argmax(err.reshape(-1))), int(valid.sum())


def deviation(tiles, s, want):
    """Worst relative deviation of the finite tile errors and the maximum from float64; everything that must be exact is asserted."""
    err, cnt, emax, worst, nvalid = want
    assert tiles.shape == err.shape and (s.tiles_x, s.tiles_y) == (err.shape[1], err.shape[0])
    assert np.array_equal(tiles["valid"], cnt) and s.valid_pixels == nvalid
    assert s.worst_tile == worst
    assert np.array_equal(np.isinf(tiles["error"]), np.isinf(err)) and not np.isnan(tiles["error"]).any()
    assert bits(F32(s.max_tile_error)) == bits(tiles["error"].reshape(-1)[worst])
    fin = np.isfinite(err) & (err > 0)
    assert (tiles["error"][~fin & np.isfinite(err)] == 0).all()
    return float(np.max(np.abs(tiles["error"][fin].astype(np.float64) - err[fin]) / err[fin])) if fin.any() else 0.0


def error_inputs():
    for (W, H) in ERROR_SIZES + [(64, 48)]:
        for holes, bad, spread in ((True, True, 0.3), (True, False, 0.05), (False, False, 0.5)):
            yield "%dx%d holes=%d bad=%d spread=%g" % (W, H, holes, bad, spread), synthetic(W, H, 0, holes, bad, spread)


# ---- CPU: the error twin ------------------------------------------------------------------------------------------------------------
def test_error_twin_against_float64():
    worst = 0.0
    for name, (f, h) in error_inputs():
        f0, h0 = f.copy(), h.copy()
        tiles, s = converge_twin.film_error(f, h)
        dev = deviation(tiles, s, error_f64(f, h))
        print("%-44s twin vs float64: %.3g" % (name, dev))
        worst = max(worst, dev)
        assert same_film(f, f0) and same_film(h, h0)
    print("worst %.3g (bound %.3g)" % (worst, TWIN_VS_F64))
    assert worst < TWIN_VS_F64


def test_error_known_answers():
    """Answers that need no restatement: equal films have error 0; a film of empty pixels has no valid pixel; one pixel whose half
    is twice as bright; a non-finite pixel makes its tile +inf; a clipped tile divides by its own count."""
    f, h = synthetic(37, 29, 1, holes=False, bad=False)
    h2 = f.copy()
    h2["rgb"] *= F32(0.5)
    h2["weight"] *= F32(0.5)  # the same colours from half the weight (exact: a power of two)
    tiles, s = converge_twin.film_error(f, h2)
    assert (tiles["error"] == 0).all() and s.max_tile_error == 0 and s.worst_tile == 0 and s.valid_pixels == 37 * 29
    assert tiles["valid"].tolist() == [[256, 256, 80], [208, 208, 65]]
    z = np.zeros((29, 37), A.FILM_DTYPE)
    tiles, s = converge_twin.film_error(f, z)
    assert (tiles["valid"] == 0).all() and (tiles["error"] == 0).all() and s.valid_pixels == 0 and s.max_tile_error == 0
    one_f, one_h = film(np.full((1, 1, 3), 1.0), np.full((1, 1), 2.0)), film(np.full((1, 1, 3), 2.0), np.full((1, 1), 2.0))
    tiles, s = converge_twin.film_error(one_f, one_h)  # I = 0.5, A = 1: d = 1.5, s = 1.5
    assert tiles["valid"].tolist() == [[1]] and bits(tiles["error"])[0, 0] == bits(F32(1.5) / np.sqrt(F32(1.5)))
    dark = film(np.zeros((1, 1, 3)), np.ones((1, 1)))  # the floor under the square root: s = 0 -> 1e-3
    tiles, s = converge_twin.film_error(dark, film(np.full((1, 1, 3), 0.25), np.ones((1, 1))))
    assert bits(tiles["error"])[0, 0] == bits(F32(0.75) / np.sqrt(F32(1e-3)))
    for poison in (np.inf, -np.inf, np.nan):
        f3, h3 = synthetic(37, 29, 2, holes=True, bad=False)
        f3[20, 35] = ((poison, 1.0, 1.0), 1.0)
        h3[20, 35] = ((1.0, 1.0, 1.0), 1.0)
        tiles, s = converge_twin.film_error(f3, h3)
        assert np.isinf(tiles["error"][1, 2]) and tiles["error"][1, 2] > 0 and np.isfinite(np.delete(tiles["error"].reshape(-1), 5)).all()
        assert s.worst_tile == 5 and np.isinf(s.max_tile_error) and s.max_tile_error > 0


def test_error_lowest_index_wins():
    """Two tiles built equal: the summary names the lower index, whichever pair it is."""
    f, h = synthetic(16, 16, 3, holes=True, bad=False, spread=0.5)
    fl, hl = synthetic(16, 16, 4, holes=False, bad=False, spread=0.02)
    for order, want in (((f, h), (f, h), (fl, hl)), 0), (((fl, hl), (f, h), (f, h)), 1), (((f, h), (fl, hl), (f, h)), 0):
        F = np.concatenate([t[0] for t in order], axis=1)
        Hf = np.concatenate([t[1] for t in order], axis=1)
        tiles, s = converge_twin.film_error(F, Hf)
        e = tiles["error"].reshape(-1)
        assert (bits(e) == bits(e[want])).sum() == 2 and e[want] == e.max()
        assert s.worst_tile == want and bits(F32(s.max_tile_error)) == bits(e[want])
    F, Hf = np.concatenate([f, fl], axis=0), np.concatenate([h, hl], axis=0)  # tiles stacked in y: index = ty * tiles_x + tx
    tiles, s = converge_twin.film_error(np.concatenate([F, F[::-1]], axis=1)[:, :32], np.concatenate([Hf, Hf[::-1]], axis=1)[:, :32])
    assert tiles.shape == (2, 2) and s.worst_tile == int(np.argmax(tiles["error"].reshape(-1)))


# ---- CPU: the schedule ---------------------------------------------------------------------------------------------------------------
def test_schedule_tiles_the_samples_and_halves_them():
    L = ptrs.load_library()
    for log_spp in range(1, 11):
        spp = 1 << log_spp
        for log_min in range(1, log_spp + 1):
            mn = 1 << log_min
            blocks = ptrs.converge_schedule(spp, mn)
            assert len(blocks) == log_spp - log_min + 1 and blocks[0] == (0, mn // 2, mn) and blocks[-1][2] == spp
            n = half = 0
            for (b, m, e) in blocks:
                assert b == n and b < m < e and e == (2 * n if n else mn)  # the blocks tile [0, n) without gap or overlap
                half += m - b
                n = e
                assert 2 * half == n  # at every check the half film holds exactly half of the film's samples
    for spp, mn in ((8, 0), (8, 1), (8, 3), (8, 16), (0, 2), (6, 2), (1, 1), (1, 2)):
        b = (C.c_uint32 * 96)()
        n = C.c_uint32(7)
        assert L.ptrs_converge_schedule(spp, mn, b, C.byref(n)) == INVALID and b"power of two" in L.ptrs_last_error() and n.value == 7
        with pytest.raises(ptrs.PtrsError):
            ptrs.converge_schedule(spp, mn)
    assert L.ptrs_converge_schedule(8, 2, None, None) == INVALID and b"null" in L.ptrs_last_error()


# ---- CPU: argument checks that need no device -------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments():
    """ptrs_render_range(_device), ptrs_film_error(_device) and ptrs_render_converged refuse bad arguments before their first device
    call (this test never reaches one: every call here is refused, or -- without a GPU -- ends at "no HIP device")."""
    L = ptrs.load_library()
    assert L.ptrs_abi_version() == 4
    assert (L.ptrs_abi_sizeof(12), L.ptrs_abi_sizeof(13), L.ptrs_abi_sizeof(14)) == (C.sizeof(A.PtrsTileError), C.sizeof(A.PtrsFilmErrorSummary), C.sizeof(A.PtrsConvergeResult)) == (8, 24, 16 + 8 * 32)
    f, h = synthetic(8, 8, 0, holes=False, bad=False)
    tiles = np.zeros(1, A.TILE_DTYPE)
    s = A.PtrsFilmErrorSummary()
    fp, hp, tp, sp = f.ctypes.data, h.ctypes.data, tiles.ctypes.data, C.addressof(s)
    for fn, extra in ((L.ptrs_film_error, ()), (L.ptrs_film_error_device, (None,))):
        tiles_arg = (tp,)
        assert fn(0, 8, 8, None, hp, *tiles_arg, *extra, sp) == INVALID and b"null" in L.ptrs_last_error()
        assert fn(0, 8, 8, fp, None, *tiles_arg, *extra, sp) == INVALID and b"null" in L.ptrs_last_error()
        assert fn(0, 8, 8, fp, hp, *tiles_arg, *extra, None) == INVALID and b"null" in L.ptrs_last_error()
        assert fn(0, 0, 8, fp, hp, *tiles_arg, *extra, sp) == INVALID and b"positive" in L.ptrs_last_error()
        assert fn(0, 8, -1, fp, hp, *tiles_arg, *extra, sp) == INVALID and b"positive" in L.ptrs_last_error()
        assert fn(0, 8, 8, fp, fp, *tiles_arg, *extra, sp) == INVALID and b"two films" in L.ptrs_last_error()
        assert fn(0, 1 << 16, 1 << 15, fp, hp, *tiles_arg, *extra, sp) == INVALID and b"too large" in L.ptrs_last_error()
        if not torch.cuda.is_available():
            assert fn(0, 8, 8, fp, hp, *tiles_arg, *extra, sp) == DEVICE and b"no HIP device" in L.ptrs_last_error()
    assert L.ptrs_film_error_device(0, 8, 8, fp, hp, None, None, sp) == INVALID and b"tiles_out_device" in L.ptrs_last_error()
    # the render entry points: a scene pointer that is only compared with null before the refusals below
    cam, _scene = ptrs.import_scene(CORNELL, (8, 8))
    integ = ptrs.PathIntegrator(ptrs.SamplerBuilder(8, cam.film.get_sample_bounds()), 2)
    p, cabi = integ.params(cam), cam.to_abi()
    fake = C.addressof((C.c_char * 64)())
    pp, cp = C.addressof(p), C.addressof(cabi)
    st = A.PtrsStats()
    for fn, tail in ((L.ptrs_render_range, (None, None)), (L.ptrs_render_range_device, (None, None))):
        call = lambda scene, cam_, prm, b, e, fl, hf: fn(scene, cam_, prm, b, e, fl, hf, *tail)
        assert call(None, cp, pp, 0, 8, fp, None) == INVALID and b"null" in L.ptrs_last_error()
        assert call(fake, None, pp, 0, 8, fp, None) == INVALID and b"null" in L.ptrs_last_error()
        assert call(fake, cp, None, 0, 8, fp, None) == INVALID and b"null" in L.ptrs_last_error()
        assert call(fake, cp, pp, 0, 8, None, None) == INVALID and b"null" in L.ptrs_last_error()
        for (b, e) in ((0, 0), (3, 3), (5, 4), (0, 9), (8, 9), (8, 8), (0xffffffff, 1)):
            assert call(fake, cp, pp, b, e, fp, None) == INVALID and b"sample range" in L.ptrs_last_error(), (b, e)
        assert call(fake, cp, pp, 0, 8, fp, fp) == INVALID and b"half film" in L.ptrs_last_error()
        p5 = integ.params(cam)
        p5.spp = 5  # rounded up to 8: [0, 8) is inside, [0, 9) is not
        assert call(fake, cp, C.addressof(p5), 0, 9, fp, None) == INVALID and b"sample range" in L.ptrs_last_error()
        p5.spp = 0
        assert call(fake, cp, C.addressof(p5), 0, 1, fp, None) == INVALID
        pb = integ.params(cam)
        pb.row_begin, pb.row_end = 2, 9
        assert call(fake, cp, C.addressof(pb), 0, 8, fp, None) == INVALID and b"row band" in L.ptrs_last_error()
        if not torch.cuda.is_available():
            assert call(fake, cp, pp, 0, 8, fp, hp) == DEVICE and b"no HIP device" in L.ptrs_last_error()
    res = A.PtrsConvergeResult()
    conv = lambda scene, prm, target, mn, fl, r: L.ptrs_render_converged(scene, cp, prm, target, mn, fl, None, r, C.addressof(st))
    assert conv(None, pp, 0.1, 2, fp, C.addressof(res)) == INVALID and b"null" in L.ptrs_last_error()
    assert conv(fake, pp, 0.1, 2, None, C.addressof(res)) == INVALID and b"null" in L.ptrs_last_error()
    assert conv(fake, pp, 0.1, 2, fp, None) == INVALID and b"null" in L.ptrs_last_error()
    for target in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert conv(fake, pp, target, 2, fp, C.addressof(res)) == INVALID and b"target_error" in L.ptrs_last_error()
    for mn in (0, 1, 3, 16):
        assert conv(fake, pp, 0.1, mn, fp, C.addressof(res)) == INVALID and b"min_spp" in L.ptrs_last_error()
    pb = integ.params(cam)
    pb.row_begin, pb.row_end = 2, 6
    assert conv(fake, C.addressof(pb), 0.1, 2, fp, C.addressof(res)) == INVALID and b"whole film" in L.ptrs_last_error()
    if not torch.cuda.is_available():
        assert conv(fake, pp, 0.1, 2, fp, C.addressof(res)) == DEVICE and b"no HIP device" in L.ptrs_last_error()
        with pytest.raises(ptrs.PtrsError):
            ptrs.film_error(f, h)
    with pytest.raises(ptrs.PtrsError):
        ptrs.film_error(f, h[:4])


# ---- CPU: the range form of render_impl on the host twin's back end -----------------------------------------------------------------
_range_cases = {}


def range_case(orc, name):
    """(camera, scene, params, spp, the full twin render's film, the oracle's samples, the full twin render's stats), made once."""
    if name not in _range_cases:
        if name == "cornell":
            cam, scene = ptrs.import_scene(CORNELL, (24, 20))
            p, spp = orc.make_params(24, 20, 8, 5), 8
        elif name == "zoo":  # glass: passes that stay open for null-BSDF skips
            cam, scene = scenes_mod.material_zoo((48, 32))
            p, spp = orc.make_params(48, 32, 4, 8), 4
        else:  # the stratified sampler: 3 x 3 samples per pixel
            cam, scene = ptrs.import_scene(CORNELL, (24, 20))
            p, spp = orc.make_params(24, 20, 9, 5, sampler=A.SAMPLER_STRATIFIED, n_sampled_dimensions=19), 9
        _fo, so, _sto = orc.OracleScene(scene).render(cam, p, n_threads=4, want_samples=True)
        ft, st_, stt = twin.TwinScene(scene).render(cam, p, want_samples=True)
        assert np.array_equal(bits(st_), bits(so))
        _range_cases[name] = (cam, scene, p, spp, ft, so, stt)
    return _range_cases[name]


RANGE_SPLITS = {"cornell": [[(0, 8)], [(0, 3), (3, 8)], [(0, 1), (1, 2), (2, 8)]], "zoo": [[(0, 4)], [(0, 1), (1, 4)], [(0, 2), (2, 4)]], "stratified": [[(0, 9)], [(0, 4), (4, 9)]]}


@pytest.mark.parametrize("name", ["cornell", "zoo", "stratified"])
def test_range_twin_chains_to_the_full_render(orc, name):
    """Successive ranges on one film (and one half film) give the film of the plain render bit for bit, rgb and weight; every sample
    value equals the oracle's; the ranges' stats add up to the render's; a half film that takes part in some of the calls only equals
    a separate range call into it."""
    cam, scene, p, spp, full, so, st_full = range_case(orc, name)
    rs = converge_twin.RangeScene(scene)
    for split in RANGE_SPLITS[name]:
        f, h = np.zeros_like(full), np.zeros_like(full)
        samples = np.full(so.shape, 7.0, F32)
        tot = [0, 0, 0, 0, 0]
        for (b, e) in split:
            before = samples.copy()
            _, st = rs.render_range(cam, p, b, e, film=f, half=h, samples=samples)
            assert st.samples == (p.width + 4) * (p.height + 4) * (e - b)
            assert np.array_equal(bits(samples[:, :, :b]), bits(before[:, :, :b])) and np.array_equal(bits(samples[:, :, e:]), bits(before[:, :, e:]))
            for k, v in enumerate((st.samples, st.rays_extension, st.rays_shadow, st.rays_mis, st.passes)):
                tot[k] += v
        assert same_film(f, full) and same_film(h, full), (name, split)
        assert np.array_equal(bits(samples), bits(so)), (name, split)
        assert tuple(tot[:4]) == (st_full.samples, st_full.rays_extension, st_full.rays_shadow, st_full.rays_mis) and tot[4] == len(split)
    b, e = RANGE_SPLITS[name][1][0]
    f, h = np.zeros_like(full), np.zeros_like(full)
    rs.render_range(cam, p, b, e, film=f, half=h)
    rs.render_range(cam, p, e, spp, film=f)
    alone, _ = rs.render_range(cam, p, b, e)
    assert same_film(f, full) and same_film(h, alone) and not same_film(h, full)


def test_range_twin_refusals_and_row_split_plans(orc):
    """The range is checked by render_impl itself as well; a plan that splits rows keeps the existing 1e-6 bound; sample chunks inside
    a range (a plan that keeps the rows) change no bit."""
    cam, scene, p, spp, full, so, _ = range_case(orc, "cornell")
    rs = converge_twin.RangeScene(scene)
    for (b, e) in ((0, 0), (3, 3), (5, 4), (0, 9), (8, 9)):
        with pytest.raises(RuntimeError, match="sample range"):
            rs.render_range(cam, p, b, e)
    f = np.zeros_like(full)
    with pytest.raises(RuntimeError, match="half film"):
        rs.render_range(cam, p, 0, 8, film=f, half=f)
    chunks = orc.make_params(24, 20, 8, 5, paths_per_pass=28 * 24 * 2)  # two samples per pass: [0, 5) is three passes, [5, 8) two
    f, h = np.zeros_like(full), np.zeros_like(full)
    _, st0 = rs.render_range(cam, chunks, 0, 5, film=f, half=h)
    _, st1 = rs.render_range(cam, chunks, 5, 8, film=f, half=h)
    assert (st0.passes, st1.passes) == (3, 2) and same_film(f, full) and same_film(h, full)
    rows = orc.make_params(24, 20, 8, 5, paths_per_pass=28 * 5)  # five sample rows per pass
    f = np.zeros_like(full)
    rs.render_range(cam, rows, 0, 3, film=f)
    rs.render_range(cam, rows, 3, 8, film=f)
    rel = np.sqrt(((f["rgb"].astype(np.float64) - full["rgb"]) ** 2).sum() / (full["rgb"].astype(np.float64) ** 2).sum())
    assert rel < 1e-6 and np.abs(f["weight"] - full["weight"]).max() <= 1e-6 * full["weight"].max()
    band = np.zeros_like(full)
    for (a, b) in ((0, 7), (7, 20)):
        pb = orc.make_params(24, 20, 8, 5, row_begin=a, row_end=b)
        rs.render_range(cam, pb, 0, 3, film=band)
        rs.render_range(cam, pb, 3, 8, film=band)
    assert same_film(band, full)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def integrator(cam, spp, depth, **kw):
    return ptrs.PathIntegrator(ptrs.SamplerBuilder(spp, cam.film.get_sample_bounds()), depth, **kw)


def check_device_equals_twin(tiles, s, f, h, what):
    t_want, s_want = converge_twin.film_error(f, h)
    bad = (bits(tiles["error"]) != bits(t_want["error"])) | (tiles["valid"] != t_want["valid"])
    assert not bad.any(), "%s: %d of %d tile records differ from the twin, first %s: %r vs %r" % (what, bad.sum(), bad.size, np.argwhere(bad)[0], tiles[bad][0], t_want[bad][0])
    assert bits(F32(s.max_tile_error)) == bits(F32(s_want.max_tile_error)), (what, s.max_tile_error, s_want.max_tile_error)
    assert (s.worst_tile, s.valid_pixels, s.tiles_x, s.tiles_y) == (s_want.worst_tile, s_want.valid_pixels, s_want.tiles_x, s_want.tiles_y), what


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", ERROR_SIZES + [(64, 48)], ids=["%dx%d" % s for s in ERROR_SIZES + [(64, 48)]])
def test_device_error_equals_twin(W, H):
    """ptrs_film_error and ptrs_film_error_device (torch buffers, a stream of the caller's) against the twin: every tile record and the
    summary, bit for bit; the films are unchanged afterwards."""
    stream = torch.cuda.Stream()
    for holes, bad, spread in ((True, True, 0.3), (True, False, 0.05), (False, False, 0.5)):
        f, h = synthetic(W, H, 0, holes, bad, spread)
        f0, h0 = f.copy(), h.copy()
        what = "%dx%d holes=%d bad=%d" % (W, H, holes, bad)
        tiles, s = ptrs.film_error(f, h)
        check_device_equals_twin(tiles, s, f0, h0, what + " host form")
        _, s2 = ptrs.film_error(f, h, want_tiles=False)
        assert bytes(s2) == bytes(s) and same_film(f, f0) and same_film(h, h0)
        tf, th = torch.from_numpy(values(f).copy()).cuda(), torch.from_numpy(values(h).copy()).cuda()
        tt = torch.full((tiles.size, 2), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s3 = ptrs.film_error_device(W, H, tf.data_ptr(), th.data_ptr(), tt.data_ptr(), stream=stream.cuda_stream)
        got = tt.cpu().numpy().view(A.TILE_DTYPE).reshape(tiles.shape)
        check_device_equals_twin(got, s3, f0, h0, what + " device form")
        assert np.array_equal(bits(tf.cpu().numpy()), bits(values(f0))) and np.array_equal(bits(th.cpu().numpy()), bits(values(h0)))


@pytest.mark.gpu
def test_device_error_lowest_index_wins():
    f, h = synthetic(16, 16, 3, holes=True, bad=False, spread=0.5)
    fl, hl = synthetic(16, 16, 4, holes=False, bad=False, spread=0.02)
    for order, want in (((f, h), (f, h), (fl, hl)), 0), (((fl, hl), (f, h), (f, h)), 1):
        F = np.ascontiguousarray(np.concatenate([t[0] for t in order], axis=1))
        Hf = np.ascontiguousarray(np.concatenate([t[1] for t in order], axis=1))
        tiles, s = ptrs.film_error(F, Hf)
        check_device_equals_twin(tiles, s, F, Hf, "equal tiles")
        assert s.worst_tile == want


_gpu_cases = {}


def gpu_case(orc, name):
    """(camera, scene, spp, depth, render()'s film, render()'s samples, its stats), made once per scene; the oracle's samples are checked here."""
    if name not in _gpu_cases:
        if name == "cornell":
            cam, scene = ptrs.import_scene(CORNELL, (24, 20))
            spp, depth = 16, 5
        else:
            cam, scene = scenes_mod.material_zoo((48, 32))
            spp, depth = 4, 8
        integ = integrator(cam, spp, depth)
        integ.render(cam, scene)  # (the scene's first render learns the survival profile the next ones use)
        cam.film.clear()
        samples = integ.render(cam, scene, want_samples=True)
        st = integ.last_stats
        full = cam.film.pixels.copy()
        cam.film.clear()
        _fo, so, _ = orc.OracleScene(scene).render(cam, orc.make_params(cam.film.width, cam.film.height, spp, depth), n_threads=8, want_samples=True)
        assert np.array_equal(bits(samples), bits(so))
        _gpu_cases[name] = (cam, scene, spp, depth, full, samples, (st.samples, st.rays_extension, st.rays_shadow, st.rays_mis))
    return _gpu_cases[name]


def chain(integ, cam, scene, split, full, samples_full, rays_full, what, expect=None):
    """The split's ranges on one film and one half film: both equal render()'s film, the samples equal render()'s (and so the oracle's)."""
    cam.film.clear()
    half = np.zeros_like(full)
    samples = np.full(samples_full.shape, 7.0, F32)
    tot = [0, 0, 0, 0]
    for (b, e) in split:
        st = integ.render_range(cam, scene, b, e, half=half, samples=samples)
        assert st.samples == (cam.film.width + 4) * (cam.film.height + 4) * (e - b), what
        if expect:
            expect(st, e - b)
        for k, v in enumerate((st.samples, st.rays_extension, st.rays_shadow, st.rays_mis)):
            tot[k] += v
    assert same_film(cam.film.pixels, full), what + ": the chained film differs from render()'s"
    assert same_film(half, full), what + ": the half film differs from render()'s"
    assert np.array_equal(bits(samples), bits(samples_full)), what + ": samples differ"
    assert tuple(tot) == rays_full, what
    cam.film.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "zoo"])
def test_range_renders_chain_to_render(orc, name):
    """Chained ranges against ptrs_render, bit for bit, film, half film and samples: lanes 1 and 4, a paths_per_pass that forces
    sample chunks inside a range, the fused tail forced on (the Cornell box has an instantiation) and off."""
    cam, scene, spp, depth, full, samples, rays = gpu_case(orc, name)
    splits = [[(0, spp)], [(0, 3), (3, spp)], [(0, 1), (1, 2), (2, spp)]]
    integ = integrator(cam, spp, depth)
    for split in splits:
        chain(integ, cam, scene, split, full, samples, rays, "%s %s" % (name, split))
    for lanes in (1, 4):
        def lanes_are(st, ns, lanes=lanes):
            assert st.lanes == lanes
        with ptrs.options(lanes=lanes):
            chain(integ, cam, scene, splits[1], full, samples, rays, "%s lanes %d" % (name, lanes), lanes_are)
    per_sample = (cam.film.width + 4) * (cam.film.height + 4)
    chunked = integrator(cam, spp, depth, paths_per_pass=per_sample * 2)  # two samples per pass

    def passes_are(st, ns):
        assert st.passes == (ns + 1) // 2
    for lanes in (1, 4):
        with ptrs.options(lanes=lanes):
            chain(chunked, cam, scene, splits[1], full, samples, rays, "%s chunks of two samples, lanes %d" % (name, lanes), passes_are)

    def no_tail(st, ns):
        assert st.tail_launches == 0

    def tail_at_2(st, ns):
        assert st.tail_launches == st.passes and st.tail_round == 2, "the scene has no fused-tail instantiation"
    with ptrs.options(tail=0):
        chain(integ, cam, scene, splits[2], full, samples, rays, name + " tail off", no_tail)
    if name == "cornell":
        with ptrs.options(tail_at=2):
            chain(integ, cam, scene, splits[2], full, samples, rays, name + " tail at 2", tail_at_2)


@pytest.mark.gpu
def test_range_half_film_device_entry_bands_and_row_splits(orc):
    """A half film that takes part in one call only equals a separate range call; ptrs_render_range_device with torch films on a
    stream of the caller's; a band (row_begin / row_end) range; one row-split plan, held to the existing 1e-6."""
    cam, scene, spp, depth, full, samples, rays = gpu_case(orc, "cornell")
    integ = integrator(cam, spp, depth)
    half = np.zeros_like(full)
    integ.render_range(cam, scene, 0, 5, half=half)
    integ.render_range(cam, scene, 5, spp)
    assert same_film(cam.film.pixels, full)
    cam.film.clear()
    integ.render_range(cam, scene, 0, 5)
    assert same_film(cam.film.pixels, half) and not same_film(half, full)
    cam.film.clear()
    H, W = full.shape
    tf, th = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda"), torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for (b, e) in ((0, 5), (5, spp)):
        st = integ.render_range_device(cam, scene, b, e, tf.data_ptr(), th.data_ptr() if b == 0 else 0, stream=stream.cuda_stream)
        assert st.samples == (W + 4) * (H + 4) * (e - b)
    assert np.array_equal(bits(tf.cpu().numpy()), bits(values(full))) and np.array_equal(bits(th.cpu().numpy()), bits(values(half)))
    for (a, b) in ((0, 7), (7, 20)):
        for (s0, s1) in ((0, 3), (3, spp)):
            st = integ.render_range(cam, scene, s0, s1, row_begin=a, row_end=b)
            assert st.samples == (W + 4) * (b - a + 4) * (s1 - s0)
    assert same_film(cam.film.pixels, full)
    cam.film.clear()
    rows = integrator(cam, spp, depth, paths_per_pass=(W + 4) * 5)  # five sample rows per pass
    rows.render_range(cam, scene, 0, 3)
    rows.render_range(cam, scene, 3, spp)
    got = cam.film.pixels
    rel = np.sqrt(((got["rgb"].astype(np.float64) - full["rgb"]) ** 2).sum() / (full["rgb"].astype(np.float64) ** 2).sum())
    assert rel < 1e-6
    cam.film.clear()
    with pytest.raises(ptrs.PtrsError, match="sample range"):
        integ.render_range(cam, scene, 4, 4)
    with pytest.raises(ptrs.PtrsError, match="sample range"):
        integ.render_range(cam, scene, 0, spp + 1)


@pytest.mark.gpu
def test_render_converged_stops_where_its_history_says():
    """Cornell 32 x 32, ceiling 64, min 4: target 0 runs to 64 and gives render()'s film bit for bit; a huge target stops at 4; a
    target between two consecutive checks' errors stops at the first check below it; the reported errors are the twin's on the
    returned films; the film at n is render_range(0, n)'s."""
    cam, scene = ptrs.import_scene(CORNELL, (32, 32))
    integ = integrator(cam, 64, 5)
    integ.render(cam, scene)
    cam.film.clear()
    integ.render(cam, scene)
    full = cam.film.pixels.copy()
    cam.film.clear()
    r = integ.render_converged(cam, scene, 0.0, min_spp=4, want_half=True)
    hist = r["history"]
    print("history", hist)
    assert r["spp_done"] == 64 and not r["converged"] and [n for n, _ in hist] == [4, 8, 16, 32, 64]
    assert same_film(cam.film.pixels, full)
    _, s = converge_twin.film_error(cam.film.pixels, r["half"])
    assert bits(F32(hist[-1][1])) == bits(F32(s.max_tile_error)) and r["worst_tile"] == s.worst_tile and s.valid_pixels == 32 * 32
    assert integ.last_stats.samples == 36 * 36 * 64 and integ.last_stats.passes >= 10
    half32 = np.zeros_like(full)  # the half film by the schedule, through the range entry point
    cam.film.clear()
    for (b, m, e) in ptrs.converge_schedule(64, 4):
        integ.render_range(cam, scene, b, m, half=half32)
        integ.render_range(cam, scene, m, e)
    assert same_film(cam.film.pixels, full) and same_film(half32, r["half"])
    cam.film.clear()
    r = integ.render_converged(cam, scene, 1e30, min_spp=4)
    assert r["spp_done"] == 4 and r["converged"] and r["history"] == hist[:1]
    cam.film.clear()
    integ.render_range(cam, scene, 0, 4)
    at4 = cam.film.pixels.copy()
    cam.film.clear()
    r = integ.render_converged(cam, scene, 1e30, min_spp=4)
    assert same_film(cam.film.pixels, at4)
    cam.film.clear()
    errs = [e for _, e in hist]
    k = next(i for i in range(1, len(errs)) if errs[i] < min(errs[:i]))  # the first check that is lower than every check before it
    target = 0.5 * (errs[k] + min(errs[:k]))
    r = integ.render_converged(cam, scene, target, min_spp=4, want_half=True)
    assert r["converged"] and r["spp_done"] == hist[k][0] and r["history"] == hist[: k + 1]
    _, s = converge_twin.film_error(cam.film.pixels, r["half"])
    assert bits(F32(r["history"][-1][1])) == bits(F32(s.max_tile_error))
    cam.film.clear()
    integ.render_range(cam, scene, 0, hist[k][0])
    stopped = cam.film.pixels.copy()
    cam.film.clear()
    r = integ.render_converged(cam, scene, target, min_spp=4)
    assert same_film(cam.film.pixels, stopped)
    cam.film.clear()
    r = integ.render_converged(cam, scene, 0.0, min_spp=64)  # one block, one check
    assert r["spp_done"] == 64 and len(r["history"]) == 1 and same_film(cam.film.pixels, full)


@pytest.mark.gpu
def test_headless_cli_renders_until_converged(tmp_path):
    """ptrs_headless --target_error: prints every check and the count it stopped at; render.png is that film (a target of 0 gives the
    bytes of the plain render at the ceiling, a huge one those of a plain render of --min_samples samples)."""
    importlib.import_module("pathtracer-rs_amd.build").build_host()
    dirs = {k: tmp_path / k for k in ("plain16", "plain4", "zero", "huge")}
    for d in dirs.values():
        d.mkdir()
    base = [CLI, CORNELL, "-r", "32x32", "-d", "3", "--headless"]
    subprocess.check_call(base + ["-s", "16", "-o", str(dirs["plain16"])])
    subprocess.check_call(base + ["-s", "4", "-o", str(dirs["plain4"])])
    zero = subprocess.run(base + ["-s", "16", "-o", str(dirs["zero"]), "--target_error", "0", "--min_samples", "4"], check=True, capture_output=True, text=True).stderr
    huge = subprocess.run(base + ["-s", "16", "-o", str(dirs["huge"]), "--target_error", "1e30", "--min_samples", "4", "--aov"], check=True, capture_output=True, text=True).stderr
    assert re.findall(r"INFO check \d+: (\d+) spp", zero) == ["4", "8", "16"] and "INFO stopped at 16 spp (ceiling reached" in zero
    assert re.findall(r"INFO check \d+: (\d+) spp", huge) == ["4"] and "INFO stopped at 4 spp (converged" in huge
    assert (dirs["zero"] / "render.png").read_bytes() == (dirs["plain16"] / "render.png").read_bytes()
    assert (dirs["huge"] / "render.png").read_bytes() == (dirs["plain4"] / "render.png").read_bytes()
    assert (dirs["huge"] / "albedo.png").exists()
    bad = subprocess.run(base + ["-s", "16", "-o", str(dirs["zero"]), "--target_error", "0.1", "--min_samples", "3"], capture_output=True, text=True)
    assert bad.returncode != 0 and "min_spp" in bad.stderr
