"""The shade kernels' forms and the capacity edges of their staged tables, as whole renders against the oracle: per-sample radiance
bits, the four ray counts, the film at 1e-5 relative L2 (test_gpu_parity._gpu_vs_oracle).  Every case first asks
ptrs_probe_shade_tables for the configuration its render stages -- the header proves which side of an edge, which feature set and
which environment route the case runs on.  Scenes: tests/shade_cases.py.  The CPU half holds the host twin to the oracle on every
one of these scenes at a small size."""
import numpy as np
import pytest

import shade_cases as sc
import twin

ptrs, A = sc.ptrs, sc.A
ALL_KINDS = {A.MAT_MATTE, A.MAT_METAL, A.MAT_MIRROR, A.MAT_GLASS, A.MAT_DISNEY, A.MAT_SUBSTRATE}
STRAT = dict(dim=2, depth=15, nd=63)  # 2 x 2 = 4 spp at the zoo's depth; 63 dimensions, the most the sampler holds (3 * 16 + 1 = 49 are the least for depth 15; the rest is room for the zoo's null-BSDF skips, and the oracle's error_flags say that no path drew past them)


def _header(cam, scene, spp, depth, it=1, sampler=None, **opts):
    integ = ptrs.PathIntegrator(sampler or ptrs.SamplerBuilder(spp, cam.film.get_sample_bounds()), depth)
    with ptrs.options(**opts):
        h, _ = ptrs.probe_shade_tables(scene, integ.params(cam), it, A.PROBE_SHADE_SOBOL, np.array([[0, 0, 0, 1, 2, 0, 0, 0, 0, 0, 0, 0]], np.uint32))
    return h


def _vs_oracle(orc, cam, scene, spp, depth, oracle=None, expect_tail=True, **opts):
    from test_gpu_parity import _gpu_vs_oracle
    cam.film.clear()
    return _gpu_vs_oracle(ptrs, orc, cam, scene, spp, depth, expect_tail=expect_tail, oracle=oracle, **opts)


# ---- CPU: the host twin against the oracle on every new scene --------------------------------------------------------------------
def _twin_vs_oracle(orc, cam, scene, spp, depth, **kw):
    p = orc.make_params(cam.film.width, cam.film.height, spp, depth, **kw)
    fo, so, sto = orc.OracleScene(scene).render(cam, p, n_threads=4, want_samples=True)
    ft, stw, stt = twin.TwinScene(scene).render(cam, p, want_samples=True)
    assert sto.error_flags == 0
    assert (stt.samples, stt.rays_extension, stt.rays_shadow, stt.rays_mis) == (sto.samples, sto.rays_extension, sto.rays_shadow, sto.rays_mis)
    assert np.array_equal(so.view(np.uint32), stw.view(np.uint32))
    assert stt.rays_shadow > 0


@pytest.mark.parametrize("feat", sc.ZOO_FEATS)
def test_twin_open_zoo(orc, feat):
    """All six material kinds are first hits of the camera rays at the GPU cases' size; twin == oracle per sample at a small one, with
    the second environment light and with the stratified sampler where the GPU cases use them."""
    cam, scene, _ = sc.open_zoo(feat)
    assert sc.first_hit_kinds(cam, scene) == ALL_KINDS
    cam, scene, _ = sc.open_zoo(feat, (42, 28))
    _twin_vs_oracle(orc, cam, scene, 2, 15)
    if feat == "img_env":
        cam, scene, env = sc.open_zoo(feat, (42, 28), second_env=True)
        assert len(env) == 2
        _twin_vs_oracle(orc, cam, scene, 2, 15)
        cam, scene, _ = sc.open_zoo(feat)  # (at the GPU case's own size: whether a path outruns the 63 dimensions depends on it)
        _twin_vs_oracle(orc, cam, scene, STRAT["dim"] ** 2, STRAT["depth"], sampler=A.SAMPLER_STRATIFIED, n_sampled_dimensions=STRAT["nd"])


@pytest.mark.parametrize("extra,textured", [(3, False), (4, False), (3, True), (4, True)])
def test_twin_cornell_39_40(orc, extra, textured):
    cam, scene = sc.cornell_plus(extra, (30, 30), textured)
    assert scene.num_triangles() == 36 + extra and (sc.SH_TRIS, sc.SH_TRIS + 1) == (36 + 3, 36 + 4)
    _twin_vs_oracle(orc, cam, scene, 2, 6)


@pytest.mark.parametrize("extra", [None, "area", "point", "env"])
def test_twin_lights_floor(orc, extra):
    cam, scene = sc.lights_floor(extra, (36, 24))
    assert len(scene.lights) == sc.SH_LIGHTS + (extra is not None)
    _twin_vs_oracle(orc, cam, scene, 2, 4)


@pytest.mark.parametrize("size", list(sc.ENV_SIZES))
def test_twin_env_sizes(orc, size):
    cam, scene = sc.env_spheres(size, (30, 20))
    assert [l["kind"] for l in scene.lights] == [A.LIGHT_INFINITE] and scene.lights[0]["dist"]["nv"] == 2 * sc.ENV_SIZES[size][0]
    _twin_vs_oracle(orc, cam, scene, 2, 6)


def test_twin_glass_panes(orc):
    cam, scene = sc.glass_panes_box((40, 25))
    _twin_vs_oracle(orc, cam, scene, 2, 12)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("feat", sc.ZOO_FEATS)
def test_zoo_under_every_feature_set(orc, feat):
    """Mirror, metal, glass, Disney, substrate and matte vertices through the shade kernels of one feature set (the header names it),
    with the environment light presampled or walked in the kernel and the tables staged or not: 120 x 80, 4 spp, depth 15."""
    cam, scene, env = sc.open_zoo(feat)
    oracle = None
    for pre, lds in ((1, 1), (0, 1), (1, 0), (0, 0)):
        h = _header(cam, scene, 4, 15, env_presample=pre, shade_lds=lds)
        assert h["feat"] == sc.FEAT_OF[feat], h
        if env:
            assert h["pre_li"] == (env[0] if pre else A.NO_LIGHT) and h["envpre"] == pre and h["marg_li"] == (env[0] if lds else A.NO_LIGHT), h
        else:
            assert (h["pre_li"], h["marg_li"], h["envpre"]) == (A.NO_LIGHT, A.NO_LIGHT, 0), h
        assert h["n_lights_lds"] == (min(len(scene.lights), sc.SH_LIGHTS) if lds else 0) and h["tri_lds"] == 0
        oracle = _vs_oracle(orc, cam, scene, 4, 15, oracle=oracle, env_presample=pre, shade_lds=lds)


@pytest.mark.gpu
def test_zoo_with_two_environment_lights(orc):
    """The first environment light is presampled, the second is walked inside a shade kernel built with the walk (ENVPRE false) that
    also loads pre0 / pre1 -- and whose staged marginal tables are the FIRST light's, not the one it walks."""
    cam, scene, env = sc.open_zoo("img_env", second_env=True)
    h = _header(cam, scene, 4, 15)
    assert h["feat"] == A.FEAT_IMG_ENV and h["pre_li"] == env[0] and h["marg_li"] == env[0] and h["envpre"] == 0, h
    oracle = _vs_oracle(orc, cam, scene, 4, 15)
    _vs_oracle(orc, cam, scene, 4, 15, oracle=oracle, shade_lds=0)


@pytest.mark.gpu
def test_zoo_with_the_stratified_sampler(orc):
    """An environment-lit scene under the stratified sampler: nothing is presampled, the marginal tables are staged, the shade
    kernels walk them."""
    cam, scene, env = sc.open_zoo("img_env")
    sb = ptrs.StratifiedSamplerBuilder(STRAT["dim"], STRAT["nd"])
    h = _header(cam, scene, 4, STRAT["depth"], sampler=sb)
    assert h["feat"] == A.FEAT_IMG_ENV and h["pre_li"] == A.NO_LIGHT and h["envpre"] == 0 and h["marg_li"] == env[0], h
    from test_gpu_parity import rel_l2
    integ = ptrs.PathIntegrator(sb, STRAT["depth"])
    cam.film.clear()
    got = integ.render(cam, scene, want_samples=True)
    st = integ.last_stats
    p = orc.make_params(cam.film.width, cam.film.height, 4, STRAT["depth"], sampler=A.SAMPLER_STRATIFIED, n_sampled_dimensions=STRAT["nd"])
    film_ref, so, sto = orc.OracleScene(scene).render(cam, p, n_threads=8, want_samples=True)
    assert sto.error_flags == 0 and st.error_flags == 0
    assert (st.samples, st.rays_extension, st.rays_shadow, st.rays_mis) == (sto.samples, sto.rays_extension, sto.rays_shadow, sto.rays_mis)
    bad = (got.view(np.uint32) != so.view(np.uint32)).any(axis=-1)
    assert bad.sum() == 0, "%d of %d samples differ" % (bad.sum(), bad.size)
    assert rel_l2(cam.film.to_rgb(), film_ref["rgb"] / film_ref["weight"][..., None]) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("extra,textured", [(3, False), (4, False), (3, True), (4, True)])
def test_39_and_40_triangles(orc, extra, textured):
    """39 triangles fill 507 of the 512 staged vectors, 40 need 520 and stay in global memory (the header says which); the round-by-round
    schedule and the fused tail from round 0, which stages the same records.  Textured: an image texture on a wall puts the
    records' dpdu / dpdv fields in use (FEAT_IMG; that form has no fused tail for a Matte scene, so it runs round by round only)."""
    cam, scene = sc.cornell_plus(extra, (64, 64), textured)
    h = _header(cam, scene, 8, 15)
    assert h["tri_lds"] == (1 if extra == 3 else 0) and h["feat"] == (A.FEAT_IMG if textured else A.FEAT_SIMPLE), h
    assert _header(cam, scene, 8, 15, shade_lds=0)["tri_lds"] == 0
    oracle = _vs_oracle(orc, cam, scene, 8, 15)
    if not textured:
        _vs_oracle(orc, cam, scene, 8, 15, oracle=oracle, tail_at=0)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [None, "area", "point", "env"])
def test_16_and_17_lights(orc, extra):
    """16 lights are all staged; of 17 the last one is read from global memory: an emissive triangle, a point light, or the
    environment light -- presampled (and its marginal tables staged) at an index whose record is not."""
    cam, scene = sc.lights_floor(extra)
    n = len(scene.lights)
    h = _header(cam, scene, 8, 6)
    assert h["n_lights_lds"] == sc.SH_LIGHTS and n == sc.SH_LIGHTS + (extra is not None), h
    if extra == "env":
        assert scene.lights[16]["kind"] == A.LIGHT_INFINITE and (h["pre_li"], h["marg_li"], h["envpre"]) == (16, 16, 1), h
    oracle = _vs_oracle(orc, cam, scene, 8, 6, expect_tail=False)
    if extra == "env":
        _vs_oracle(orc, cam, scene, 8, 6, oracle=oracle, env_presample=0)
    else:
        _vs_oracle(orc, cam, scene, 8, 6, oracle=oracle, tail_at=0)  # one Matte bucket, no textures: the fused tail stages the same light records


@pytest.mark.gpu
@pytest.mark.parametrize("size", list(sc.ENV_SIZES))
def test_environment_map_sizes(orc, size):
    """nv = 2, 512 and 1024 (the area's exact size) are staged and presampled; nv = 2048 does not fit: no staging, no presample, the
    shade kernels with the in-kernel walk over the global tables.  Each also with env_presample = 0, where the shade kernels walk
    the staged tables themselves.  48 x 32, 2 spp."""
    cam, scene = sc.env_spheres(size)
    nv = scene.lights[0]["dist"]["nv"]
    h = _header(cam, scene, 2, 8)
    fits = nv <= sc.SH_MARG_N
    assert nv == 2 * sc.ENV_SIZES[size][0] and h["feat"] == A.FEAT_FULL
    assert (h["marg_li"], h["pre_li"], h["envpre"]) == ((0, 0, 1) if fits else (A.NO_LIGHT, A.NO_LIGHT, 0)), h
    oracle = _vs_oracle(orc, cam, scene, 2, 8, expect_tail=False)
    h0 = _header(cam, scene, 2, 8, env_presample=0)
    assert (h0["marg_li"], h0["pre_li"], h0["envpre"]) == ((0 if fits else A.NO_LIGHT), A.NO_LIGHT, 0), h0
    _vs_oracle(orc, cam, scene, 2, 8, oracle=oracle, env_presample=0)


@pytest.mark.gpu
@pytest.mark.parametrize("nib", [8, 13])
def test_specular_chains_across_the_window(orc, nib):
    """A path starts round `it` at dimension 4 + 8 it if every vertex before drew 8 dimensions; a specular vertex (glass) draws 3, so
    after k of them the path is at dim0 = 4 + 8 it - 5 k.  The staged window starts at sob_lo = 8 it - 12 (8 nibbles, 24 dimensions,
    from round 2) or 8 it - 3 (13 nibbles, 15 dimensions, from round 1), so a batch straddles the lower edge from k = 4 with 8
    nibbles and from k = 2 with 13.  Here every camera path crosses two glass panes, four specular surfaces: the first matte
    vertex (k = 4, it = 4) draws from dimension 16 with the window at 20 (8 nibbles) or 29 (13) -- below it, the global route --
    and the vertices after it draw 24 .. 31, 32 .. 39, ... against windows from 28, 36, ... (8 nibbles: each batch straddles
    the edge, four dimensions outside and four staged) or from 37, 45, ... (13 nibbles: wholly below); the paths that were reflected inside
    a pane (k = 6, 8) lie further down, the camera vertex and the panes' own (it <= 3, k <= it) inside the window.  Depth 12, no
    fused tail (its draws never use the window).  13 nibbles: the smallest frame whose index needs 33 bits, 32 772 x 2 at 2 spp."""
    res, spp = ((160, 100), 4) if nib == 8 else ((32772, 2), 2)
    cam, scene = sc.glass_panes_box(res)
    if nib == 13:  # the same horizontal view through a slit two pixels high
        import math
        cam = ptrs.look_at_camera([0.0, 0.0, 3.0], [0.0, 0.0, -2.0], [0, 1, 0], 2.0 * math.degrees(math.atan(math.tan(math.radians(25.0)) * res[1] / res[0])), res)
    for it in (1, 4, 5):
        h = _header(cam, scene, spp, 12, it=it, tail=0)
        assert h["sob_nib"] == nib and (h["sob_lo"], h["sob_n"]) == sc.window_expected(nib, it), h
    assert sc.window_expected(nib, 4)[0] > 4 + 8 * 4 - 5 * 4  # the first matte vertex behind the panes draws below the window
    _vs_oracle(orc, cam, scene, spp, 12, expect_tail=False, tail=0)
