"""The shade kernels' LDS context (ptrs_hip.hip: ShadeCtxLds, stage_shade_tables, HipBackend::shade_cfg) through
ptrs_probe_shade_tables, against answers from outside it.

Sobol' draws: every batch size at every alignment against the round's window, on both nibble counts, bit for bit against the value
computed in integers from the generator matrices of data/sobol_tables.bin (never from the nibble table the kernels stage), and the
route each batch took against the route the returned configuration implies.  Environment samples: the staged marginal tables against
the host twin's walk of the global tables and the device's own ptrs_probe_light, bit for bit, with u.y on every marginal cdf value
and its neighbours -- where a staged table read one element off its end would pick another row."""
import numpy as np
import pytest

import shade_cases as sc
import twin

ptrs, A = sc.ptrs, sc.A
INF = np.float32(np.inf)

# width, height, spp: 2 log2(resolution) + log2(spp) = 2 * 7 + 2 = 16 and 2 * 16 + 2 = 34, then the two sides of the rule's edge,
# 2 * 15 + 2 = 32 (the last 8-nibble sampler) and 2 * 16 + 1 = 33 (the first 13-nibble one)
PARAMS = {"8": (64, 64, 4), "13": (40000, 8, 4), "8-edge": (32764, 8, 4), "13-edge": (32772, 2, 2)}
ROUNDS = (0, 1, 2, 3, 15, 127)                # 127: 12 + 8 * 127 = 1028 > 1024, the window's top is clamped to the tables' end
CAMERA_DIMS = (2, 3, 5, 6, 7, 8, 9, 10)       # the camera vertex's batch: dimension 4 is skipped


def _params(orc, case):
    w, h, spp = PARAMS[case]
    assert 2 * (max(w, h) + 4 - 1).bit_length() + spp.bit_length() - 1 == {"8": 16, "13": 34, "8-edge": 32, "13-edge": 33}[case]
    return orc.make_params(w, h, spp, 15)


def _indices(rng):
    """Every single bit 0 .. 51, all-ones per nibble, random 52-bit and random 32-bit values (the latter keep the 8-nibble window in play)."""
    idx = [1 << b for b in range(52)] + [0xF << (4 * k) for k in range(13)] + [0, (1 << 52) - 1, (1 << 32) - 1, 1 << 32]
    idx += [int(v) for v in rng.integers(0, 1 << 52, 40)] + [int(v) for v in rng.integers(0, 1 << 32, 40)]
    return np.array(idx, np.uint64)


def _batches(lo, n):
    """(N, dims[8]) for every N at every alignment against the window [lo, lo + n): consecutive batches from lo - N - 1 to
    lo + n + 1, the same first dimensions with gaps, reversed, and the camera vertex's pattern slid across both edges."""
    out = []
    for N in (1, 2, 3, 8):
        for d0 in range(lo - N - 1, lo + n + 2):
            forms = [d0 + np.arange(N)]
            if N > 1:
                forms += [d0 + 2 * np.arange(N), (d0 + np.arange(N))[::-1]]
            if N == 8:
                forms.append(d0 - 2 + np.array(CAMERA_DIMS))
            for dims in forms:
                if dims.min() >= 0 and dims.max() < 1024:
                    out.append((N, np.concatenate([dims, np.zeros(8 - N, np.int64)])))
    out.append((8, np.array(CAMERA_DIMS)))
    return out


def _rows(h, seed):
    rng = np.random.default_rng(seed)
    idx = _indices(rng)
    bt = _batches(h["sob_lo"], h["sob_n"] if h["sob_n"] else 24)
    N = np.repeat(np.array([b[0] for b in bt], np.uint32), len(idx))
    dims = np.repeat(np.array([b[1] for b in bt], np.int64), len(idx), axis=0)
    index = np.tile(idx, len(bt))
    scramble = rng.integers(0, 1 << 32, len(index)).astype(np.uint32)
    scramble[0::3] = 0
    scramble[1::3] = 0xFFFFFFFF
    rows = np.zeros((len(index), 12), np.uint32)
    rows[:, 0], rows[:, 1] = (index & np.uint64(0xFFFFFFFF)).astype(np.uint32), (index >> np.uint64(32)).astype(np.uint32)
    rows[:, 2], rows[:, 3], rows[:, 4:12] = scramble, N, dims
    return rows, index, scramble, N, dims


def _check_values(out, mats, index, scramble, N, dims):
    want = sc.sobol_reference(mats, index.astype(np.int64), scramble, dims).view(np.uint32)
    used = np.arange(8)[None, :] < N[:, None]
    bad = ((out[:, 0:8] != want) & used).any(axis=1)
    assert not bad.any(), "%d of %d rows differ, first: index %#x dims %s N %d route %d" % (bad.sum(), len(bad), int(index[bad][0]), dims[bad][0], N[bad][0], out[bad][0, 8])
    assert not (out[:, 0:8][~used]).any()


def test_sobol_reference_matches_the_oracle(orc):
    """The reference of this file (integers over the generator matrices) against the oracle's SobolSampler on pixels, samples and
    dimensions of three sampler sizes, 33-bit indices among them; CPU only."""
    mats = sc.sobol_matrices()
    rng = np.random.default_rng(23)
    for (w, h, spp) in [(64, 64, 4), (3840, 2160, 512), (40000, 8, 4)]:
        p = orc.make_params(w, h, spp, 4)
        n = 4000
        px, py, sn = rng.integers(-2, w + 2, n), rng.integers(-2, h + 2, n), rng.integers(0, spp, n)
        dims = rng.integers(2, 1024, n)
        dims[:8] = [2, 3, 255, 256, 511, 512, 1022, 1023]
        want, idx = orc.sobol_samples(p, px, py, sn, dims)
        got = sc.sobol_reference(mats, idx.astype(np.int64), sc.cantor_scramble(px, py), dims[:, None])[:, 0]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        if spp > 4 or w > 32768:
            assert int(idx.max()).bit_length() >= 33


def _tiny_scene():
    s = ptrs.RenderScene()
    m = s.add_material(A.MAT_MATTE, [s.const_rgb([0.5, 0.5, 0.5])])
    s.add_mesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32), m, emission_rgb=[1.0, 1.0, 1.0])
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(PARAMS))
def test_sobol_draws_at_every_alignment_of_the_window(orc, case):
    """ShadeCtxLds::sobol<N>, N in 1, 2, 3, 8, with the batch's first dimension from sob_lo - N - 1 to sob_lo + sob_n + 1, consecutive
    and not, at rounds 0, 1, 2, 3, 15 and 127 (top clamped): values bit-equal to the matrices' on every row, the route taken equal to
    the route the returned window implies, and the window itself where the round arithmetic puts it (cap = 24 dimensions of 8
    nibbles, 15 of 13; top = min(1024, 12 + 8 it)).  With 8 nibbles all three routes occur; with 13 the run shortcut does not exist
    (it is compiled for the 8-nibble stride), so the two others do.  shade_lds = 0: no window, the global route everywhere, the same
    bits."""
    mats = sc.sobol_matrices()
    nib = int(case.split("-")[0])
    scene, p = _tiny_scene(), _params(orc, case)
    seen, total = set(), 0
    for it in (ROUNDS if case in ("8", "13") else (2, 127)):  # (the samplers next to the rule's edge: two rounds)
        h, _ = ptrs.probe_shade_tables(scene, p, it, A.PROBE_SHADE_SOBOL, np.array([[0, 0, 0, 1, 2, 0, 0, 0, 0, 0, 0, 0]], np.uint32))
        assert h["sob_nib"] == nib and (h["sob_lo"], h["sob_n"]) == sc.window_expected(nib, it), (it, h)
        assert h["sob_lo"] + h["sob_n"] <= 1024 and h["sob_n"] * (16 * nib + 4) <= sc.SH_SOB_WORDS
        rows, index, scramble, N, dims = _rows(h, 100 * len(case) + 1000 * nib + it)
        h2, out = ptrs.probe_shade_tables(scene, p, it, A.PROBE_SHADE_SOBOL, rows)
        assert h2 == h
        _check_values(out, mats, index, scramble, N, dims)
        route = sc.sobol_route(h, index, dims, N)
        assert np.array_equal(out[:, 8], route), "first row off its route: %s" % (rows[out[:, 8] != route][:1],)
        if nib == 8:
            assert (route[rows[:, 1] != 0] == A.SOB_ROUTE_GLOBAL).all() and (rows[:, 1] != 0).sum() > 1000  # a high word: never the staged nibbles
        seen |= set(int(r) for r in np.unique(route))
        total += len(rows)
    assert seen == ({A.SOB_ROUTE_GLOBAL, A.SOB_ROUTE_RUN, A.SOB_ROUTE_LOOP} if nib == 8 else {A.SOB_ROUTE_GLOBAL, A.SOB_ROUTE_LOOP}), seen
    assert total > (150000 if case in ("8", "13") else 50000)
    with ptrs.options(shade_lds=0):
        h, out = ptrs.probe_shade_tables(scene, p, 2, A.PROBE_SHADE_SOBOL, rows)
    assert h["sob_n"] == 0 and h["n_lights_lds"] == 0 and h["tri_lds"] == 0
    assert (out[:, 8] == A.SOB_ROUTE_GLOBAL).all()
    _check_values(out, mats, index, scramble, N, dims)


# ---- the staged marginal tables --------------------------------------------------------------------------------------------------
def _env_case(name):
    import test_bsdf_kat as bk
    if name in sc.ENV_SIZES:
        rows, cols = sc.ENV_SIZES[name]
        s = ptrs.RenderScene()
        m = s.add_material(A.MAT_MATTE, [s.const_rgb([0.5, 0.5, 0.5])])
        s.add_mesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32), m)
        li = sc.tx.add_infinite_light(s, sc.env_map_of(rows, cols), light_to_world=sc._env_l2w())
        s.preprocess_lights()
        return s, twin.TwinScene(s), li
    kind, rotated = name.split("-")
    s, ts, li, _, _ = bk.env_scene(kind, rotated == "rot")
    return s, ts, li


def _env_rows(scene, li, n=1 << 16):
    rng = np.random.default_rng(77)
    cdf = np.asarray(scene.lights[li]["dist"]["marg_cdf"], np.float32)
    uy = np.concatenate([cdf, np.nextafter(cdf, INF), np.nextafter(cdf, -INF), [0.0, sc.ONE_MINUS_EPS, 0.5]]).astype(np.float32)
    uy = np.unique(uy[(uy >= 0) & (uy < 1)])
    ux = np.array([0.0, 0.37, sc.ONE_MINUS_EPS], np.float32)
    edge = np.stack([np.tile(ux, len(uy)), np.repeat(uy, len(ux))], 1)[:n // 2]
    u = np.concatenate([edge, rng.random((n - len(edge), 2), dtype=np.float32)]).astype(np.float32)
    assert len(u) == n and len(uy) >= len(np.unique(cdf[cdf < 1])) and 3 * len(uy) <= n // 2 and (u < 1).all()  # every distinct cdf value is among the rows
    return u


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["odd-plain", "odd-rot", "texel-plain", "texel-rot", "256x256", "1x1", "512x256"])
def test_staged_marginal_tables_give_the_twins_samples(orc, name):
    """inf_light_sample through ShadeCtxLds::inf_marginal -- the marginal function, cdf and guide out of LDS -- on 2^16 u, with u.y at
    0, at 1 - eps and at every value of the marginal cdf with its float neighbours, on maps from nv = 2 to nv = 1024, the largest
    that is staged (cdf[1024] is the staged area's last word but the guide's): bit-equal to the host twin (global tables; held to
    float64 statistics by test_bsdf_kat.test_environment_light_sampling) and to the device's ptrs_probe_light.  The same rows with
    shade_lds = 0 take the global tables on the device and give the same bits."""
    s, ts, li = _env_case(name)
    u = _env_rows(s, li)
    rows = np.zeros((len(u), 12), np.uint32)
    rows[:, 0:2], rows[:, 2] = u.view(np.uint32), li
    p = orc.make_params(64, 64, 4, 15)
    h, out = ptrs.probe_shade_tables(s, p, 1, A.PROBE_SHADE_ENV, rows)
    assert h["marg_li"] == li and h["pre_li"] == li and h["envpre"] == 1 and h["feat"] == A.FEAT_IMG_ENV, h
    assert (out[:, 8] == 1).all()
    lp = np.concatenate([u, np.tile(np.array([0, 0, 1], np.float32), (len(u), 1))], 1)
    ref0 = np.array([0, 0, 0, 0, 0, 1], np.float32)
    want = twin.light_probe(ts, li, ref0, lp)
    dev = ptrs.probe_light(s, li, ref0, lp)
    for ref, who in ((want, "twin"), (dev, "ptrs_probe_light")):
        assert np.array_equal(out[:, 0:7], ref[:, 0:7].view(np.uint32)), who
        assert np.array_equal(out[:, 7], (ref[:, 7] > 0).astype(np.uint32)), who
    assert (out[:, 7] == 1).mean() > 0.5
    with ptrs.options(shade_lds=0):
        h0, out0 = ptrs.probe_shade_tables(s, p, 1, A.PROBE_SHADE_ENV, rows)
    assert h0["marg_li"] == A.NO_LIGHT and h0["pre_li"] == li and (out0[:, 8] == 0).all()
    assert np.array_equal(out0[:, 0:8], out[:, 0:8])
