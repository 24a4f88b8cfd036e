"""The edge-avoiding a-trous denoiser (ptrs_denoise) against answers from outside it.

On the CPU the denoise twin (tests/denoise_twin: pt_denoise.h's per-pixel functions compiled for the host and run over whole images) is
held against a float64 numpy restatement of the contract written here, against known answers that need no restatement, and against a
256-spp oracle render: the filter must bring a 4-spp Cornell frame closer to it.  None of these tests calls the library; the argument
checks of the entry points do, and need no device.  Under -m gpu the device must equal the twin bit for bit on every output value,
with both forms of the iteration kernel, through both entry points, end to end and through the headless CLI.
"""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded: the library then runs on the HIP runtime torch brings along, and the process has one)

from conftest import CORNELL, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "aov_twin"))
sys.path.insert(0, os.path.join(ROOT, "tests", "denoise_twin"))
import aov_twin  # noqa: E402
import denoise_twin  # noqa: E402
from test_camera_film_kat import Scatter, bits, cornell, integrator, outside_pfilm  # noqa: E402

ptrs = importlib.import_module("pathtracer-rs_amd")
A = ptrs.abi
F32 = np.float32
CLI = os.path.join(ROOT, "pathtracer-rs_amd", "ptrs_headless")
NAMES = ("albedo", "normal", "depth")
DEFAULTS = dict(iterations=5, sigma_color=0.25, sigma_normal=0.3, sigma_depth=0.1, demodulate=True)

# Twin against the float64 restatement, per value relative to max(|f64|, 1e-3).  Measured over every input of
# test_twin_against_float64 (1x1, 5x3, 37x29 synthetic, Cornell 64x64 at 4 spp; 1 and 5 iterations, demodulation on and off, each sigma
# dropped in turn): worst 8.35e-7, on the Cornell input (a float32 numpy prototype of the formulas measured 7.7e-7).  The bound is 8 x that, rounded up to a
# power of two.
TWIN_VS_F64 = 2.0 ** -17
# the LDS form's tile: 64 columns x 8 lattice rows of outputs (pt_hip_post.h: DN_TILE_W, DN_TILE_T), for steps up to 16
TILE_W, TILE_T, LDS_STEPS = 64, 8, (1, 2, 4, 8, 16)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def film(rgb, weight):
    f = np.zeros(weight.shape, A.FILM_DTYPE)
    f["rgb"], f["weight"] = rgb.astype(F32), weight.astype(F32)
    return f


def make_films(w, colour, albedo, normal, depth, cov):
    """Accumulated films from per-pixel values: sums = value x coverage x weight, as the film gathers them."""
    cw = (cov * w)[..., None]
    planes = dict(albedo=film(albedo * cw, w), normal=film(normal * cw, w),
                  depth=film(np.stack([depth * cov * w, cov * w, np.zeros_like(w)], axis=-1), w))
    return film(colour * w[..., None], w), planes


_synth = {}


def synthetic(W, H, seed=7):
    """A W x H input with 5 % empty pixels, 20 % uncovered ones, a normal discontinuity down the middle, albedo in 0.05 .. 1, partial
    coverage on a tenth of the rest, a depth ramp and a noisy irradiance.  Pixel (0, 0) is neither empty nor uncovered."""
    if (W, H, seed) not in _synth:
        rng = np.random.default_rng(seed * 100003 + W * 131 + H)
        w = rng.uniform(0.5, 4.0, (H, W))
        empty = rng.random((H, W)) < 0.05
        cov = np.where(rng.random((H, W)) < 0.2, 0.0, np.where(rng.random((H, W)) < 0.1, rng.uniform(0.3, 0.9, (H, W)), 1.0))
        empty[0, 0], cov[0, 0] = False, 1.0
        x = np.arange(W)[None, :] + np.zeros((H, 1))
        y = np.arange(H)[:, None] + np.zeros((1, W))
        n = np.where((x < W / 2)[..., None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0])) + rng.normal(0.0, 0.03, (H, W, 3))
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        depth = 2.0 + 0.02 * x + 0.01 * y + rng.normal(0.0, 0.002, (H, W))
        albedo = rng.uniform(0.05, 1.0, (H, W, 3))
        L = (0.6 + 0.3 * np.sin(0.2 * x + 0.1 * y))[..., None] * rng.uniform(0.5, 1.5, (H, W, 3))
        colour = (albedo * cov[..., None] + (1.0 - cov[..., None])) * L
        w = np.where(empty, 0.0, w)
        beauty, planes = make_films(w, colour, albedo, n, depth, cov)
        for f in [beauty] + list(planes.values()):
            f.setflags(write=False)
        _synth[(W, H, seed)] = (beauty, planes)
    return _synth[(W, H, seed)]


_cornell = {}


def cornell_inputs():
    """Cornell 64 x 64 at 4 spp, depth 5, built on the CPU: the beauty film from the host twin, the planes from the aov twin's
    per-sample values through the float64 scatter of test_camera_film_kat, rounded to float32."""
    if "in" not in _cornell:
        W = H = 64
        spp = 4
        cam, scene, tscene = cornell(W, H)
        beauty = tscene.render(cam, integrator(cam, spp, 5).params(cam))[0]
        pf, _ = outside_pfilm(W, H, spp, "twin")
        rows = aov_twin.aov_rows(scene, cam, float(F32(1.0) / np.sqrt(F32(spp))), pf.reshape(-1, 2))
        vals = dict(albedo=rows[:, 0:3], normal=rows[:, 4:7], depth=np.stack([rows[:, 7], rows[:, 3], np.zeros(len(rows), F32)], axis=-1))
        planes = {}
        for k in NAMES:
            sc = Scatter(np.zeros((H, W), A.FILM_DTYPE))
            sc.add(pf.reshape(-1, 2), vals[k], 0, H)
            planes[k] = film(sc.sum[..., :3], sc.sum[..., 3])
        for f in [beauty] + list(planes.values()):
            f.setflags(write=False)
        _cornell["in"] = (beauty, planes)
    return _cornell["in"]


# ---- the float64 restatement of the contract ------------------------------------------------------------------------------
def shifted(a, sx, sy, fill):
    """b[y, x] = a[y + sy, x + sx] inside the image, `fill` outside."""
    H, W = a.shape[:2]
    b = np.full(a.shape, fill, a.dtype)
    y0, y1, x0, x1 = max(0, -sy), min(H, H - sy), max(0, -sx), min(W, W - sx)
    if y1 > y0 and x1 > x0:
        b[y0:y1, x0:x1] = a[y0 + sy:y1 + sy, x0 + sx:x1 + sx]
    return b


def restatement(beauty, planes, iterations, sigma_color, sigma_normal, sigma_depth, demodulate):
    f = lambda a: np.asarray(a, dtype=np.float64)
    sigma_color, sigma_normal, sigma_depth = (float(F32(s)) for s in (sigma_color, sigma_normal, sigma_depth))
    w = f(beauty["weight"])
    ok = w > 0
    ws = np.where(ok, w, 1.0)
    c = f(beauty["rgb"]) / ws[..., None]
    dr, dg = f(planes["depth"]["rgb"][..., 0]), f(planes["depth"]["rgb"][..., 1])
    cov = dg / ws
    z = np.where(dg > 0, dr / np.where(dg > 0, dg, 1.0), 0.0)
    n = f(planes["normal"]["rgb"]) / ws[..., None]
    l = np.sqrt((n * n).sum(axis=-1, keepdims=True))
    n = np.where(l > 0, n / np.where(l > 0, l, 1.0), 0.0)
    a = np.maximum((f(planes["albedo"]["rgb"]) + (w - dg)[..., None]) / ws[..., None], 0.01) if demodulate else np.ones_like(c)
    x = c / a
    h = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]
    for i in range(iterations):
        s, sc = 2 ** i, sigma_color * 2.0 ** -i
        num, den = np.zeros_like(x), np.zeros_like(w)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                okq = shifted(ok, s * dx, s * dy, False)
                xq, nq, cq, zq = (shifted(v, s * dx, s * dy, 0.0) for v in (x, n, cov, z))
                e = np.zeros_like(w)
                if sigma_color > 0:
                    e = e + ((x - xq) ** 2).sum(axis=-1) / sc ** 2
                if sigma_normal > 0:
                    e = e + (((n - nq) ** 2).sum(axis=-1) + (cov - cq) ** 2) / sigma_normal ** 2
                if sigma_depth > 0:
                    e = e + ((z - zq) / np.maximum(np.maximum(z, zq), 1e-30)) ** 2 / sigma_depth ** 2
                wt = np.where(okq & ok, h[dy + 2] * h[dx + 2] * np.exp(-e), 0.0)
                num += wt[..., None] * xq
                den += wt
        x = np.where(ok[..., None], num / np.where(ok, den, 1.0)[..., None], x)
    out = np.where(ok[..., None], x * a, 0.0)
    return np.concatenate([out, np.where(ok, 1.0, 0.0)[..., None]], axis=-1)


def values(f):
    return np.concatenate([f["rgb"], f["weight"][..., None]], axis=-1)


def twin_vs_f64(beauty, planes, **p):
    got = values(denoise_twin.denoise(beauty, planes, **p)).astype(np.float64)
    want = restatement(beauty, planes, **p)
    return float((np.abs(got - want) / np.maximum(np.abs(want), 1e-3)).max())


PARAM_SETS = [params(iterations=1), params(), params(iterations=1, demodulate=False), params(demodulate=False),
              params(sigma_color=0.0), params(sigma_normal=-1.0), params(sigma_depth=0.0)]


# ---- CPU: 1. twin against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1x1", "5x3", "37x29", "cornell"])
def test_twin_against_float64(name):
    """dn_prepare / dn_atrous / dn_finish in float32 against the float64 restatement: 1 and 5 iterations (on the small images the step
    exceeds the image), demodulation on and off, each sigma <= 0 in turn."""
    beauty, planes = cornell_inputs() if name == "cornell" else synthetic(*[int(v) for v in name.split("x")])
    worst = 0.0
    for p in PARAM_SETS:
        err = twin_vs_f64(beauty, planes, **p)
        print("%s %r: worst |twin - f64| / max(|f64|, 1e-3) = %.3g" % (name, p, err))
        worst = max(worst, err)
    print("%s: worst %.3g, %.3f of the bound" % (name, worst, worst / TWIN_VS_F64))
    assert worst <= TWIN_VS_F64
    out = denoise_twin.denoise(beauty, planes)
    empty = beauty["weight"] == 0
    assert not values(out)[empty].any() and (out["weight"][~empty] == 1).all() and np.isfinite(out["rgb"]).all()
    if name == "37x29":
        assert 0.02 < empty.mean() < 0.1 and 0.1 < (planes["depth"]["rgb"][..., 1] == 0)[~empty].mean() < 0.3


# ---- CPU: 2. known answers -------------------------------------------------------------------------------------------------------------
def test_constant_colour_is_a_fixed_point():
    """A constant colour over arbitrary guides, demodulation off, comes out as it went in: every iteration is a weighted mean of equal
    values.  5 iterations x 27 roundings (25 products and sums, the division, the final product) x 2^-24 = 8e-6, rounded up."""
    beauty, planes = synthetic(37, 29)
    c = np.array([0.7, 0.05, 1.9])
    w = beauty["weight"].astype(np.float64)
    b = film(c * w[..., None], w)
    out = denoise_twin.denoise(b, planes, demodulate=False)
    ok = w > 0
    rel = np.abs(out["rgb"][ok].astype(np.float64) - c) / c
    print("constant colour: worst relative deviation %.3g" % rel.max())
    assert rel.max() <= 1e-5 and not values(out)[~ok].any()


def test_perpendicular_half_planes_do_not_mix():
    """Two half-planes with perpendicular normals and sigma_normal 0.1: |dn|^2 = 2, e >= 200, exp(-e) = 0 in binary32.  Whatever the
    right half's colours are, the left half's output is the same bits."""
    W, H = 24, 12
    rng = np.random.default_rng(3)
    w = rng.uniform(0.5, 4.0, (H, W))
    left = (np.arange(W) < W // 2)[None, :] & np.ones((H, 1), bool)
    n = np.where(left[..., None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    albedo, depth, cov = rng.uniform(0.2, 0.9, (H, W, 3)), np.full((H, W), 3.0), np.ones((H, W))
    c1 = rng.uniform(0.1, 2.0, (H, W, 3))
    c2 = np.where(left[..., None], c1, rng.uniform(0.1, 20.0, (H, W, 3)))
    outs = []
    for c in (c1, c2):
        b, planes = make_films(w, c, albedo, n, depth, cov)
        outs.append(denoise_twin.denoise(b, planes, sigma_normal=0.1))
    assert np.array_equal(bits(values(outs[0])[left]), bits(values(outs[1])[left]))
    assert not np.array_equal(bits(values(outs[0])[~left]), bits(values(outs[1])[~left]))
    b, planes = make_films(w, c1, albedo, n, depth, cov)
    assert (np.abs(outs[0]["rgb"] - b["rgb"] / b["weight"][..., None]) > 1e-3).any()  # (it did filter)


def test_demodulation_keeps_texture():
    """beauty = albedo x L with a one-pixel checker albedo in {0.2, 0.8}, constant L, flat guides: with demodulation the filter sees the
    constant L and returns the beauty to 1e-5 (the bound of the constant-colour test); without it the checker is blurred, by more than
    100 x that.  L = 0.1: neighbouring colours are then 0.06 apart per channel, |dc|^2 = 0.011 against sigma_color^2 = 0.0625, so the
    colour term alone does not keep the texture (at L = 1.5 it would: e = 39 between neighbours)."""
    W, H = 20, 14
    yy, xx = np.mgrid[0:H, 0:W]
    albedo = np.where(((xx + yy) % 2 == 0)[..., None], 0.2, 0.8) * np.ones(3)
    w = np.random.default_rng(5).uniform(0.5, 4.0, (H, W))
    colour = albedo * 0.1
    b, planes = make_films(w, colour, albedo, np.zeros((H, W, 3)) + np.array([0.0, 1.0, 0.0]), np.full((H, W), 2.5), np.ones((H, W)))
    dev = {}
    for demod in (True, False):
        out = denoise_twin.denoise(b, planes, demodulate=demod)
        dev[demod] = float((np.abs(out["rgb"].astype(np.float64) - colour) / colour).max())
    print("checker albedo: worst relative deviation with demodulation %.3g, without %.3g" % (dev[True], dev[False]))
    assert dev[True] <= 1e-5 and dev[False] > 100 * 1e-5


def test_empty_pixels_are_no_taps():
    """Empty pixels come out as zeros with weight 0, and as taps they are what the outside of the image is: a frame of empty pixels
    around an image leaves the inside's output bit-identical to the cropped image's."""
    b, planes = synthetic(21, 17)
    f = 3
    big_b = np.zeros((17 + 2 * f, 21 + 2 * f), A.FILM_DTYPE)
    big = {k: big_b.copy() for k in NAMES}
    big_b[f:-f, f:-f] = b
    for k in NAMES:
        big[k][f:-f, f:-f] = planes[k]
        big[k]["rgb"][:f] = 0.5  # whatever the planes hold where the beauty film has no weight is not looked at
    for p in (params(), params(iterations=8, demodulate=False)):
        small, large = denoise_twin.denoise(b, planes, **p), denoise_twin.denoise(big_b, big, **p)
        assert np.array_equal(bits(values(large[f:-f, f:-f])), bits(values(small)))
        frame = np.ones(large.shape, bool)
        frame[f:-f, f:-f] = False
        assert not values(large)[frame].any()


# ---- CPU: 3. it denoises ---------------------------------------------------------------------------------------------------------------
def test_it_denoises_cornell():
    """Cornell 64 x 64 at 4 spp, depth 5, default parameters, against a 256-spp oracle render: the all-pixel mean squared RGB error goes
    down, and over the pixels whose reference luminance is <= 1 (everything but the emitter) to at most 0.6 of the input's.  Measured:
    masked after / before = 0.412, all-pixel 0.872 (the float64 prototype against a 1024-spp reference: 0.41 and 0.87)."""
    from oracle import orc
    beauty, planes = cornell_inputs()
    cam, scene, _ = cornell(64, 64)
    o = orc.OracleScene(scene)
    ref = o.render(cam, orc.make_params(64, 64, 256, 5), n_threads=16)[0]
    o.close()
    ref = ref["rgb"].astype(np.float64) / ref["weight"].astype(np.float64)[..., None]
    noisy = beauty["rgb"].astype(np.float64) / beauty["weight"].astype(np.float64)[..., None]
    out = denoise_twin.denoise(beauty, planes)["rgb"].astype(np.float64)
    mask = ref @ np.array([0.212671, 0.715160, 0.072169]) <= 1.0
    mse = lambda img, m: float(((img - ref) ** 2)[m].mean())
    every = np.ones(mask.shape, bool)
    print("cornell 64x64 4 spp: masked MSE %.4g -> %.4g (ratio %.3f, %.1f %% of the pixels), all-pixel %.4g -> %.4g (ratio %.3f), mean %.4f -> %.4f" % (
        mse(noisy, mask), mse(out, mask), mse(out, mask) / mse(noisy, mask), 100 * mask.mean(), mse(noisy, every), mse(out, every),
        mse(out, every) / mse(noisy, every), noisy.mean(), out.mean()))
    assert mask.mean() > 0.95
    assert mse(out, every) < mse(noisy, every)
    assert mse(out, mask) <= 0.6 * mse(noisy, mask)


# ---- CPU: 4. argument errors, through the library --------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments():
    """Every refusal of the C ABI is PTRS_ERR_INVALID with a message, made before any device call: this runs without a GPU."""
    L = ptrs.load_library()
    INVALID, DEVICE = -1, -3
    d = C.c_void_p()
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert L.ptrs_denoiser_create(0, w, h, C.byref(d)) == INVALID and b"positive" in L.ptrs_last_error() and not d
    assert L.ptrs_denoiser_create(0, 8, 8, None) == INVALID and b"null" in L.ptrs_last_error()
    assert L.ptrs_denoiser_create(0, 8, 8, C.byref(d)) == 0 and d
    films = [np.zeros((8, 8), A.FILM_DTYPE) for _ in range(5)]
    ptr = [C.c_void_p(f.ctypes.data) for f in films]
    arr = lambda a, b, c: (C.c_void_p * 3)(a, b, c)
    good = A.PtrsDenoiseParams()
    L.ptrs_denoise_default_params(C.byref(good))
    assert (good.iterations, good.flags) == (5, A.PtrsDenoiseDemodulate)
    assert np.array_equal(np.array([good.sigma_color, good.sigma_normal, good.sigma_depth], F32), np.array([0.25, 0.3, 0.1], F32))
    st = A.PtrsStats()
    host = lambda dn, p, b, pl, out: L.ptrs_denoise(dn, p, b, pl, out, C.byref(st))
    dev = lambda dn, p, b, pl, out: L.ptrs_denoise_device(dn, p, b, pl, out, None, C.byref(st))
    planes = arr(ptr[1], ptr[2], ptr[3])
    for fn in (host, dev):
        for args in ((None, C.byref(good), ptr[0], planes, ptr[4]), (d, None, ptr[0], planes, ptr[4]), (d, C.byref(good), None, planes, ptr[4]),
                     (d, C.byref(good), ptr[0], None, ptr[4]), (d, C.byref(good), ptr[0], planes, None),
                     (d, C.byref(good), ptr[0], arr(None, ptr[2], ptr[3]), ptr[4]), (d, C.byref(good), ptr[0], arr(ptr[1], None, ptr[3]), ptr[4]),
                     (d, C.byref(good), ptr[0], arr(ptr[1], ptr[2], None), ptr[4])):
            assert fn(*args) == INVALID and b"null" in L.ptrs_last_error()
        for it in (0, -1, 9):
            p = ptrs.denoise_params(iterations=it)
            assert fn(d, C.byref(p), ptr[0], planes, ptr[4]) == INVALID and b"iterations" in L.ptrs_last_error()
        for field in ("sigma_color", "sigma_normal", "sigma_depth"):
            for v in (float("nan"), float("inf"), -float("inf")):
                p = ptrs.denoise_params(**{field: v})
                assert fn(d, C.byref(p), ptr[0], planes, ptr[4]) == INVALID and b"sigma" in L.ptrs_last_error()
        for out in ptr[:4]:
            assert fn(d, C.byref(good), ptr[0], planes, out) == INVALID and b"inputs" in L.ptrs_last_error()
        if not torch.cuda.is_available():
            assert fn(d, C.byref(good), ptr[0], planes, ptr[4]) == DEVICE and b"no HIP device" in L.ptrs_last_error()
    L.ptrs_denoiser_destroy(d)
    L.ptrs_denoiser_destroy(None)
    assert L.ptrs_abi_sizeof(11) == C.sizeof(A.PtrsDenoiseParams) == 20
    assert ptrs.get_option("denoise_lds") == -1
    with pytest.raises(ptrs.PtrsError):
        ptrs.Denoiser(0, 4)
    with pytest.raises(ptrs.PtrsError):
        ptrs.Denoiser(8, 8).denoise(films[0], dict(albedo=films[1], normal=films[2], depth=films[3][:4]))


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
GPU_SIZES = [(1, 1), (5, 3), (37, 29)] + [(TILE_W + 1, TILE_T * s + 1) for s in LDS_STEPS]


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", GPU_SIZES, ids=["%dx%d" % s for s in GPU_SIZES])
def test_device_equals_twin(W, H):
    """ptrs_denoise against the twin, bit for bit on every output value: both forms of the iteration kernel (denoise_lds 0 and 1), 1, 5
    and 8 iterations (steps 32 .. 128 have the direct form only), demodulation on and off; sizes 1x1, 5x3, 37x29 and one column and one
    row more than the LDS tile's output extent at every step (64 columns x 8 s rows).  The inputs are unchanged afterwards."""
    beauty, planes = synthetic(W, H)
    b, pl = beauty.copy(), {k: v.copy() for k, v in planes.items()}
    dn = ptrs.Denoiser(W, H)
    for it in (1, 5, 8):
        for demod in (True, False):
            want = denoise_twin.denoise(beauty, planes, iterations=it, demodulate=demod)
            for lds in (0, 1):
                with ptrs.options(denoise_lds=lds):
                    got = dn.denoise(b, pl, iterations=it, demodulate=demod)
                bad = bits(values(got)) != bits(values(want))
                assert not bad.any(), "%dx%d, %d iterations, demodulate %d, denoise_lds %d: %d of %d values differ from the twin, first (y, x, c) %s: %r vs %r" % (
                    W, H, it, demod, lds, bad.sum(), bad.size, np.argwhere(bad)[0], values(got)[bad][0], values(want)[bad][0])
                st = dn.last_stats
                assert st.kernel_launches == it + 2 and st.device_bytes == W * H * (64 + 5 * 16) and st.ms_total > 0
                assert (st.samples, st.rays_extension, st.passes, st.film_launches, st.lanes) == (0, 0, 0, 0, 0)
    dn.close()
    assert np.array_equal(bits(values(b)), bits(values(beauty))) and all(np.array_equal(bits(values(pl[k])), bits(values(planes[k]))) for k in NAMES)


@pytest.mark.gpu
def test_device_form_on_a_stream_equals_host_form():
    """ptrs_denoise_device on a stream of the caller's, with torch buffers, against ptrs_denoise, bit for bit; two denoisers of
    different sizes in one process, used in turn, do not disturb each other."""
    cases = [synthetic(37, 29), synthetic(65, 33)]
    dns = [ptrs.Denoiser(37, 29), ptrs.Denoiser(65, 33)]
    host = [dn.denoise(b, pl) for dn, (b, pl) in zip(dns, cases)]
    to_dev = lambda f: torch.from_numpy(values(f).copy()).cuda()
    stream = torch.cuda.Stream()
    for rnd in range(2):
        for dn, (b, pl), want in zip(dns, cases, host):
            tb, tp = to_dev(b), {k: to_dev(pl[k]) for k in NAMES}
            out = torch.full((dn.height, dn.width, 4), 7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            st = dn.denoise_device(tb.data_ptr(), {k: v.data_ptr() for k, v in tp.items()}, out.data_ptr(), stream=stream.cuda_stream)
            assert st.kernel_launches == 7 and st.device_bytes == dn.width * dn.height * 64
            assert np.array_equal(bits(out.cpu().numpy()), bits(values(want))), (rnd, dn.width)
            assert np.array_equal(bits(tb.cpu().numpy()), bits(values(b))) and all(np.array_equal(bits(tp[k].cpu().numpy()), bits(values(pl[k]))) for k in NAMES)
            assert np.array_equal(bits(values(dn.denoise(b, pl))), bits(values(want)))
    for dn in dns:
        dn.close()


@pytest.mark.gpu
def test_render_denoised_end_to_end():
    """render_denoised on Cornell 64 x 64 at 4 spp: the twin's bits when the twin is fed the device's films; the noisy film stays in
    camera.film; and the beauty film of a render made after a denoise call is bit-identical to one made before it."""
    cam, scene = ptrs.import_scene(CORNELL, (64, 64))
    integ = integrator(cam, 4, 5)
    integ.render(cam, scene)  # (the scene's first render learns the survival profile the next ones use)
    cam.film.clear()
    s1 = integ.render(cam, scene, want_samples=True)
    f1, t1 = cam.film.pixels.copy(), integ.last_stats.tail_round
    cam.film.clear()
    out = integ.render_denoised(cam, scene)
    assert np.array_equal(bits(values(cam.film.pixels)), bits(values(f1)))
    planes = integ.render_aov(cam, scene)
    want = denoise_twin.denoise(cam.film.pixels, planes)
    assert np.array_equal(bits(values(out)), bits(values(want)))
    assert out.shape == (64, 64) and (out["weight"] == 1).all()
    noisy = f1["rgb"] / f1["weight"][..., None]
    assert abs(float(out["rgb"].mean()) / float(noisy.mean()) - 1.0) < 0.02 and (np.abs(out["rgb"] - noisy) > 1e-3).any()
    cam.film.clear()
    s2 = integ.render(cam, scene, want_samples=True)
    assert np.array_equal(bits(s1), bits(s2))
    assert np.array_equal(bits(values(cam.film.pixels)), bits(values(f1)))
    assert integ.last_stats.tail_round == t1


@pytest.mark.gpu
def test_headless_cli_writes_denoised_png(tmp_path):
    """ptrs_headless --denoise at 32 x 32: denoised.png within one code value of the Python host's result, encoded like render.png;
    render.png byte-identical to a run without the flag."""
    from PIL import Image
    importlib.import_module("pathtracer-rs_amd.build").build_host()
    a, b = tmp_path / "plain", tmp_path / "denoise"
    a.mkdir()
    b.mkdir()
    base = [CLI, CORNELL, "-s", "4", "-r", "32x32", "-d", "3", "--headless"]
    subprocess.check_call(base + ["-o", str(a)])
    subprocess.check_call(base + ["-o", str(b), "--denoise"])
    assert (a / "render.png").read_bytes() == (b / "render.png").read_bytes()
    assert not (a / "denoised.png").exists()
    cam, scene = ptrs.import_scene(CORNELL, (32, 32))
    out = integrator(cam, 4, 3).render_denoised(cam, scene)
    v = out["rgb"].astype(np.float64)
    srgb = np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(np.maximum(v, 0.0), 1.0 / 2.4) - 0.055)  # math.rs:133-139
    want = np.clip(np.floor(srgb * 255.0 + 0.5), 0, 255).astype(int)
    png = np.asarray(Image.open(str(b / "denoised.png"))).astype(int)
    assert png.shape == (32, 32, 4) and (png[..., 3] == 255).all()
    assert np.abs(png[..., :3] - want).max() <= 1
    assert not np.array_equal(png, np.asarray(Image.open(str(b / "render.png"))).astype(int))
