"""Queue segments of several 64-path chunks, on every kernel form.

A pass's paths are cut into chunks of 64 and dealt to G = min(chunks, grid_max) queue segments, one wave each; grid_max is at least
CUs x 8 (2 048 on an MI355X), so a pass below 131 072 paths has one chunk per segment and every segment loop of the queue kernels --
the lane refill with rays in flight, the shade stage's software pipeline over items, the `i0 += 64` loops of the epilogue, the
resolve, the presampling, the plane and the dump kernels, k_generate's walk and the ticket counters below TK_SUB segments -- runs its
first trip only.  The option `segments` (a test hook: grid_max = min(grid_max, k)) makes segments long on passes small enough to render
with the oracle.  Every comparison here is bit equality; every device case asserts through PtrsStats.queue_segments that it ran the
geometry it is in the suite for, so that none can pass at one chunk per segment."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded: one HIP runtime per process)

import twin
from conftest import CORNELL

import test_accel_shapes as shapes
from test_adaptive import SENTINEL, check_tiles_result, start_films, tile_mask
from test_aov_ranges import aov_plan_twin, as_dict, check_aov_tiles, same, start_planes
from test_camera_film_kat import outside_pfilm, sorted_rows

F32 = np.float32


def cdiv(a, b):
    return (a + b - 1) // b


# ---- the dealing, restated from the comment above k_generate ---------------------------------------------------------------------
def deal_round_robin(chunks, G):
    """deal = 0: chunk c goes to segment c mod G; a segment's chunks stand in the order they come."""
    segs = [[] for _ in range(G)]
    for c in range(chunks):
        segs[c % G].append(c)
    return segs


def column_major_walk(chunks, cpp):
    """deal = 1: the chunks form a matrix, rows = samples, columns = the cpp chunks of one sample's pixels (chunk c = row c // cpp,
    column c mod cpp; the last row may be short), walked column by column."""
    rows = cdiv(chunks, cpp)
    return [r * cpp + col for col in range(cpp) for r in range(rows) if r * cpp + col < chunks]


def deal_by_region(chunks, G, cpp):
    """deal = 1: segment s takes the s-th run of ceil(chunks / G) cells of the walk."""
    walk, cps = column_major_walk(chunks, cpp), cdiv(chunks, G)
    return [walk[s * cps:(s + 1) * cps] for s in range(G)]


def kernel_cell(cc, chunks, cpp):
    """k_generate's closed form of the walk's cc-th cell (the columns with a cell in the last row come first, `full` cells in all) --
    transliterated, to hold the arithmetic against the walk above."""
    nsr = cdiv(chunks, cpp)
    r_last = chunks - (nsr - 1) * cpp
    full = r_last * nsr
    if cc < full:
        pc, k = cc // nsr, cc % nsr
    else:
        d = cc - full
        pc, k = r_last + d // (nsr - 1), d % (nsr - 1)
    return k * cpp + pc


# chunks -> the chunks of one sample's pixels (the matrix's columns) of the render that has so many chunks, and other widths
DEAL_SHAPES = {1: (1,), 51: (1, 7, 51), 70: (18, 1, 70), 103: (26, 5), 578: (73, 17)}  # 70: Cornell 37 x 23 / 4 spp (41 x 27 = 1 107 sample pixels); 578: Cornell 64 x 64 / 8 spp (4 624)


@pytest.mark.parametrize("chunks", sorted(DEAL_SHAPES))
def test_dealing_restated(chunks):
    """Every chunk lands in exactly one segment, no segment holds more than seg_cap / 64 = ceil(chunks / G) chunks, by region segment s
    holds the cells s cps .. min((s + 1) cps, chunks) of the column-major walk -- for every G in 1 .. chunks and both settings.  This
    guards the numbers in the GPU cases' comments; it cannot see the kernel (only its closed form of the walk, kernel_cell)."""
    for cpp in DEAL_SHAPES[chunks]:
        walk = column_major_walk(chunks, cpp)
        assert sorted(walk) == list(range(chunks))
        assert [kernel_cell(cc, chunks, cpp) for cc in range(chunks)] == walk
        for G in range(1, chunks + 1):
            cps = cdiv(chunks, G)
            for segs in (deal_round_robin(chunks, G), deal_by_region(chunks, G, cpp)):
                assert sorted(c for s in segs for c in s) == list(range(chunks))
                assert max(len(s) for s in segs) == cps  # (some segment is full: seg_cap is not larger than needed)
            rr, reg = deal_round_robin(chunks, G), deal_by_region(chunks, G, cpp)
            assert all(rr[s] == list(range(s, chunks, G)) for s in range(G)) and not [s for s in range(G) if not rr[s]]
            assert all(reg[s] == walk[s * cps:min((s + 1) * cps, chunks)] for s in range(G))
            assert [s for s in range(G) if not reg[s]] == list(range(cdiv(chunks, cps), G))


def test_dealing_of_the_gpu_cases():
    """The geometry the GPU cases below name in their comments."""
    sizes = lambda segs: [len(s) for s in segs]
    empty = lambda segs: [s for s in range(len(segs)) if not segs[s]]
    assert (41 * 27 * 4, cdiv(41 * 27 * 4, 64), 41 * 27 * 4 % 64) == (4428, 70, 12)
    assert sizes(deal_round_robin(70, 3)) == [24, 23, 23] and sizes(deal_by_region(70, 3, 18)) == [24, 24, 22]
    assert sizes(deal_round_robin(70, 69)) == [2] + [1] * 68
    assert sizes(deal_by_region(70, 69, 18)) == [2] * 35 + [0] * 34 and empty(deal_by_region(70, 69, 18)) == list(range(35, 69))
    assert sizes(deal_round_robin(70, 64)) == [2] * 6 + [1] * 58 and sizes(deal_round_robin(70, 7)) == [10] * 7
    assert (68 * 68 * 8, cdiv(68 * 68 * 8, 64), 68 * 68 * 8 % 64) == (36992, 578, 0)
    assert cdiv(578, 65) == 9 and cdiv(65, 64) == 2  # nine chunks per segment; the ticket counters hand out two numbers each: 0 .. 32 are open, 32's second number (65) is surplus
    assert empty(deal_by_region(578, 100, 73)) == [97, 98, 99] and sizes(deal_by_region(578, 100, 73))[96] == 2
    assert (65 * 43 * 8, cdiv(65 * 43 * 8, 64), 65 * 43 * 8 % 64) == (22360, 350, 24)
    assert (52 * 36 * 8, cdiv(52 * 36 * 8, 64)) == (14976, 234) and (68 * 68 * 4, cdiv(68 * 68 * 4, 64)) == (18496, 289)
    assert (84 * 49 * 4, cdiv(84 * 49 * 4, 64)) == (16464, 258)
    # 51 x 2 + 1 chunks over 51 segments: three cells per segment, 34 full segments, one cell in segment 34, the rest empty
    assert cdiv(103, 51) == 3 and empty(deal_by_region(103, 51, 26)) == list(range(35, 51))


def test_segments_option_round_trip(ptrs):
    """`segments`: default 0 (no cap), 0 .. 2^20 accepted process-wide, -1 and 2^20 + 1 refused -- no GPU needed."""
    L = ptrs.load_library()
    assert ptrs.get_option("segments") == 0
    for v in (1, 69, 1 << 20):
        with ptrs.options(segments=v):
            assert ptrs.get_option("segments") == v
    assert ptrs.get_option("segments") == 0
    for bad in (-1, (1 << 20) + 1):
        assert L.ptrs_set_option(b"segments", bad) != 0 and L.ptrs_last_error()
    assert ptrs.get_option("segments") == 0


# ---- the device against the oracle -----------------------------------------------------------------------------------------------
_oracles = {}


def oracle_of(orc, key, cam, scene, spp, depth, **kw):
    """The oracle's render of a scene and size, made once and shared by that scene's option sets: (film, samples, stats)."""
    if key not in _oracles:
        film, ref, ost = orc.OracleScene(scene).render(cam, orc.make_params(cam.film.width, cam.film.height, spp, depth, **kw), n_threads=8, want_samples=True)
        ref.setflags(write=False)
        assert ost.error_flags == 0
        _oracles[key] = (film, ref, ost)
    return _oracles[key]


def passes_of_plan(rows, NX, ns, capacity):
    """plan_passes for a band whose sample rows fit one pass (rows x NX <= capacity) and a paths_per_pass given: equal sample chunks."""
    assert rows * NX <= capacity
    spp_max = max(1, min(ns, capacity // (rows * NX)))
    per = cdiv(ns, cdiv(ns, spp_max))
    return cdiv(ns, per), rows * NX * per


def render_capped(ptrs, integ, cam, scene, oracle, k, what, n_paths, several=True, tail=None, lanes=1, passes=1, pass_paths=None, **opts):
    """One device render under segments = k against the oracle's: the geometry first, then the counts, then every sample's bits.
    tail: None = no k_tail launch (a fresh scene has no survival profile), r = handed over at round r in every pass, "learned" = where
    the passes behind the scene's first finished one are handed over by its profile (several passes: nothing to assert)."""
    with ptrs.options(lanes=lanes, segments=k, **opts):
        samples = integ.render(cam, scene, want_samples=True)
    st = integ.last_stats
    _, ref, ost = oracle
    assert st.samples == n_paths == ost.samples, (what, st.samples, n_paths)
    assert st.lanes == lanes and st.passes == passes, (what, st.lanes, st.passes)
    chunks = cdiv(pass_paths or st.samples, 64)
    assert st.queue_segments == min(k, chunks), (what, st.queue_segments, chunks)
    if several:
        assert cdiv(chunks, st.queue_segments) >= 2, what
    assert st.error_flags == 0, what
    if tail is None:
        assert st.tail_launches == 0, (what, st.tail_launches)
    elif tail != "learned":
        assert st.tail_launches == st.passes and st.tail_round == tail, (what, st.tail_launches, st.tail_round)
    assert (st.rays_extension, st.rays_shadow, st.rays_mis) == (ost.rays_extension, ost.rays_shadow, ost.rays_mis), what
    bad = (samples.view(np.uint32) != ref.view(np.uint32)).any(axis=-1)
    assert bad.sum() == 0, "%s: %d of %d samples differ from the oracle's" % (what, bad.sum(), bad.size)
    return st


def sobol_integrator(ptrs, cam, spp, depth, **kw):
    return ptrs.PathIntegrator(ptrs.SamplerBuilder(spp, cam.film.get_sample_bounds()), depth, **kw)


# Cornell 37 x 23, 4 spp: 41 x 27 x 4 = 4 428 paths, 70 chunks, the last one of 12 paths.  k = 1: the whole pass in one wave; 3: 24 + 23 + 23
# chunks round-robin, 24 + 24 + 22 by region; 7: ten each; 64: six segments of two (G = TK_SUB); 69: seg_cap = 128, round-robin segment 0
# holds two chunks, by region segments 0 - 34 hold two and 35 - 68 nothing.
SMALL = dict(res=(37, 23), spp=4, depth=15, paths=4428)
# (options, the round the fused tail takes over at or None) -- the expectations of test_fused_tail_matches_oracle: k_tail is compiled
# with one vote policy, and without tail_at a scene's first render has no survival profile to place it by
SMALL_SETS = [({"tail_at": 0}, 0), ({"tail_at": 2}, 2), ({"node_form": 2}, None), ({"vote": 0}, None), ({"vote": 1}, None), ({"vote": 2}, None),
              ({"refill": 0}, None), ({"refill": 1}, None), ({"refill": 48}, None), ({"refill_connect": 0}, None), ({"refill_connect": 1}, None), ({"refill_connect": 48}, None),
              ({"fused_epilogue": 0}, None), ({"fused_resolve": 0}, None), ({"shade_lds": 0}, None)]


def small_cornell(ptrs, orc):
    cam, scene = ptrs.import_scene(CORNELL, SMALL["res"])  # (a fresh scene per render: node_form is read when the device scene is created, and no profile places a tail)
    return cam, scene, sobol_integrator(ptrs, cam, SMALL["spp"], SMALL["depth"]), oracle_of(orc, "cornell-small", cam, scene, SMALL["spp"], SMALL["depth"])


@pytest.mark.gpu
@pytest.mark.parametrize("deal", [0, 1])
@pytest.mark.parametrize("k", [1, 3, 7, 64, 69])
def test_cornell_small_every_cap(ptrs, orc, k, deal):
    cam, scene, integ, oracle = small_cornell(ptrs, orc)
    st = render_capped(ptrs, integ, cam, scene, oracle, k, "k=%d deal=%d" % (k, deal), SMALL["paths"], deal=deal)
    assert st.queue_segments == k


@pytest.mark.gpu
@pytest.mark.parametrize("deal", [0, 1])
@pytest.mark.parametrize("k", [3, 69])
def test_cornell_small_option_sets(ptrs, orc, k, deal):
    """The traversal kernels' forms (quad nodes, the three vote policies, the idle-lane thresholds 64 / 1 / 48 of either kernel), the
    separate epilogue and resolve kernels, the shade tables out of global memory and the fused tail from rounds 0 and 2, each on
    segments of 22 - 24 chunks and on the 69 segments of which one (round-robin) or 35 (by region) hold two chunks."""
    for opts, tail in SMALL_SETS:
        cam, scene, integ, oracle = small_cornell(ptrs, orc)
        render_capped(ptrs, integ, cam, scene, oracle, k, "k=%d deal=%d %s" % (k, deal, opts), SMALL["paths"], tail=tail, deal=deal, **opts)


# Cornell 64 x 64, 8 spp: 36 992 paths, 578 chunks, no partial chunk
MID = dict(res=(64, 64), spp=8, depth=15, paths=36992)


def mid_cornell(ptrs, orc, **kw):
    cam, scene = ptrs.import_scene(CORNELL, MID["res"])
    return cam, scene, sobol_integrator(ptrs, cam, MID["spp"], MID["depth"], **kw), oracle_of(orc, "cornell-mid", cam, scene, MID["spp"], MID["depth"])


@pytest.mark.gpu
def test_cornell_ticket_counters_and_empty_segments(ptrs, orc):
    """k = 65: the 64 ticket counters hand out two numbers each, counters 0 - 32 are open and the number 65 is skipped as surplus.
    k = 100 by region: six cells per segment, segment 96 holds two, 97 - 99 nothing."""
    cam, scene, integ, oracle = mid_cornell(ptrs, orc)
    render_capped(ptrs, integ, cam, scene, oracle, 65, "k=65", MID["paths"])
    cam, scene, integ, oracle = mid_cornell(ptrs, orc)
    render_capped(ptrs, integ, cam, scene, oracle, 100, "k=100 deal=1", MID["paths"], deal=1)


@pytest.mark.gpu
@pytest.mark.parametrize("ppp", [10000, 5000])
def test_cornell_four_lanes_of_long_segments(ptrs, orc, ppp):
    """Four pipeline lanes, passes of two samples (paths_per_pass 10 000: four passes of 9 248 paths, one per lane) and of one (5 000:
    eight passes of 4 624 paths, two per lane), five segments each: 29 and 15 chunks per segment, the last chunk partial.  A lane's
    second pass finds the survival profile its first one left and hands its thin rounds to the fused tail."""
    cam, scene, integ, oracle = mid_cornell(ptrs, orc, paths_per_pass=ppp)
    passes, pass_paths = passes_of_plan(68, 68, MID["spp"], ppp)
    assert (passes, pass_paths) == {10000: (4, 9248), 5000: (8, 4624)}[ppp]
    st = render_capped(ptrs, integ, cam, scene, oracle, 5, "lanes=4 ppp=%d" % ppp, MID["paths"], tail="learned", lanes=4, passes=passes, pass_paths=pass_paths)
    assert st.tail_launches <= passes - 1


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5, 349])
def test_material_zoo_long_segments(ptrs, orc, scenes, k):
    """Material zoo 61 x 39, 8 spp: 65 x 43 x 8 = 22 360 paths, 350 chunks, the last one partial.  Every material kernel appends behind the
    others in one long segment (next_base, nee_base), the null-BSDF skip is reached; the zoo has no fused-tail instantiation."""
    cam, scene = scenes.material_zoo((61, 39))
    oracle = oracle_of(orc, "zoo", cam, scene, 8, 15)
    render_capped(ptrs, sobol_integrator(ptrs, cam, 8, 15), cam, scene, oracle, k, "zoo k=%d" % k, 22360, tail_at=0)  # (tail_at: inert here)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 233])
def test_textured_env_long_segments(ptrs, orc, scenes, k):
    """The textured-env scene 48 x 32, 8 spp: 14 976 paths, 234 chunks.  FEAT_FULL kernels with alpha-masked cards, k_env_presample's
    loops and the pre0 / pre1 prefetch slots on the second and later items; the light's samples presampled or not, tables in LDS or not."""
    for pre, lds in ((1, 1), (0, 1), (1, 0), (0, 0)):
        with ptrs.options(env_presample=pre, shade_lds=lds):
            cam, scene = scenes.textured_env((48, 32))
            oracle = oracle_of(orc, "env", cam, scene, 8, 15)
            render_capped(ptrs, sobol_integrator(ptrs, cam, 8, 15), cam, scene, oracle, k, "env k=%d presample=%d lds=%d" % (k, pre, lds), 14976)


@pytest.mark.gpu
def test_stratified_sampler_long_segments(ptrs, orc):
    """Cornell 37 x 23 with the stratified sampler (2 x 2 strata, depth 5, 3 (depth + 1) + 1 sampled dimensions as in test_stratified.py)
    on three segments: the table-reading shade kernels over many items."""
    cam, scene = ptrs.import_scene(CORNELL, (37, 23))
    nd = 3 * (5 + 1) + 1
    oracle = oracle_of(orc, "cornell-strat", cam, scene, 4, 5, sampler=ptrs.abi.SAMPLER_STRATIFIED, n_sampled_dimensions=nd)
    render_capped(ptrs, ptrs.PathIntegrator(ptrs.StratifiedSamplerBuilder(2, nd), 5), cam, scene, oracle, 3, "stratified k=3", 4428)


@pytest.mark.gpu
@pytest.mark.parametrize("stack_lds", [8, 16])
@pytest.mark.parametrize("k", [3, 288])
def test_triangle_soup_long_segments(ptrs, orc, scenes, k, stack_lds):
    """Triangle soup of 20 000, 64 x 64, 4 spp, depth 8: 18 496 paths, 289 chunks.  A tree deeper than the LDS column: the refill takes a
    new ray onto a column that has spilled."""
    with ptrs.options(stack_lds=stack_lds):
        cam, scene = scenes.triangle_soup(20000, resolution=(64, 64))
        oracle = oracle_of(orc, "soup", cam, scene, 4, 8)
        integ = sobol_integrator(ptrs, cam, 4, 8)
        st = render_capped(ptrs, integ, cam, scene, oracle, k, "soup k=%d stack_lds=%d" % (k, stack_lds), 18496)
    assert st.stack_lds == stack_lds


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 257])
def test_colonnade_quad_form_long_segments(ptrs, orc, scenes, k):
    """The colonnade at detail 0.01 with 64-texel textures, as test_cfg5_band builds it: quad nodes out of global memory, Disney + image
    textures.  80 x 45, 4 spp: 84 x 49 x 4 = 16 464 paths, 258 chunks; round by round, with the fused tail from rounds 0 and 3, by region."""
    for opts, tail in (({}, None), ({"tail_at": 0}, 0), ({"tail_at": 3}, 3), ({"deal": 1}, None)):
        cam, scene = scenes.colonnade((80, 45), detail=0.01, tex_size=64)
        oracle = oracle_of(orc, "colonnade", cam, scene, 4, 15)
        st = render_capped(ptrs, sobol_integrator(ptrs, cam, 4, 15), cam, scene, oracle, k, "colonnade k=%d %s" % (k, opts), 16464, tail=tail, **opts)
        assert st.lds_form_v4 == 0, "the scene was meant to take the quad form"


# ---- ptrs_trace_bench on the badly behaved trees of test_accel_shapes.py ---------------------------------------------------------
def trace_bench_capped(ptrs, scene, rays, ref, hit, k, what):
    with ptrs.options(segments=k):
        st, hits = ptrs.trace_bench(scene, rays, repeats=1, want_hits=True)
    chunks = cdiv(len(rays), 64)
    assert st.queue_segments == min(k, chunks) and cdiv(chunks, st.queue_segments) >= 2, (what, st.queue_segments, chunks)  # seg_cap / 64 = ceil(chunks / G)
    assert np.array_equal(hits["prim"], ref["prim"]), "%s: %d rays name another primitive" % (what, int((hits["prim"] != ref["prim"]).sum()))
    for f in ("b0", "b1", "b2"):
        assert np.array_equal(hits[f][hit].view(np.uint32), ref[f][hit].view(np.uint32)), (what, f)


@pytest.mark.gpu
@pytest.mark.parametrize("filler", [0, 3000])
@pytest.mark.parametrize("n", [17, 300])
@pytest.mark.parametrize("family", ["dup-z", "corners"])
def test_long_leaf_trace_bench_long_segments(ptrs, orc, family, n, filler):
    """The frame's extension kernel on over-long leaves (pair form, and quad form by size or by filler) with the whole ray set in one
    wave and in seven: the oracle's primitive and barycentrics, bit for bit."""
    scene, rays, ref, _occ, hit = shapes._leaf_case(ptrs, orc, family, n, filler)
    shapes._twin_leaf_check(ptrs, orc, family, n, filler)  # (first the host: no ray stacks more than stack_bound)
    inf = np.isinf(rays[:, 6])  # (the extension kernel traces every ray to infinity, as in a frame)
    assert inf.sum() >= 14 * 64
    shapes._device_scene(ptrs, scene)
    for k in (1, 7):
        trace_bench_capped(ptrs, scene, rays[inf], ref[inf], hit[inf], k, "%s n=%d filler=%d k=%d" % (family, n, filler, k))


# 512 copies of the line's two rays = 1 024 rays = 16 chunks.  test_full_stack_gpu_matches_oracle takes 32 768 copies so that every
# workgroup of an uncapped grid holds deep stacks at once; under a cap of 7 the launch has at most seven waves = two workgroups however
# many rays there are, and what the cap adds is that each of them takes new rays again and again onto columns that ran full (LDS and
# spill): 16 chunks give the one wave of k = 1 sixteen refills' worth and the seven waves of k = 7 two or three chunks each.
CHAIN_COPIES = 512


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain-10", "chain-41"])
def test_full_stack_trace_bench_long_segments(ptrs, orc, name):
    """The chains of 10 (the 9-entry LDS form, full) and 41 triangles (32 entries past the LDS column) with one and seven segments."""
    c = shapes._stack_case(ptrs, orc, name, copies=CHAIN_COPIES)  # (the host first: these very rays stay within the bound)
    hit = np.ones(len(c["rays"]), bool)
    for opts, lds in shapes.STACK_GPU[name]:
        with ptrs.options(**opts):
            shapes._device_scene(ptrs, c["scene"], c["bvh"])
            for k in (1, 7):
                trace_bench_capped(ptrs, c["scene"], c["rays"], c["ref"], hit, k, "%s %s k=%d" % (name, opts, k))


# ---- entry points around the path loop, Cornell 64 x 64 on five segments ----------------------------------------------------------
K5 = 5


@pytest.mark.gpu
def test_render_tiles_long_segments(ptrs):
    """ptrs_render_tiles with a checkerboard and a single-tile mask (k_generate_tiles compacts partly masked chunks into five segments)
    against ptrs_render_range's bits on the active tiles; inactive tiles untouched, the exported samples those of the whole render."""
    W, H, spp, depth, (b, e) = 64, 64, 8, 5, (1, 7)
    cam, scene = ptrs.import_scene(CORNELL, (W, H))
    integ = sobol_integrator(ptrs, cam, spp, depth)
    with ptrs.options(lanes=1):
        so = integ.render(cam, scene, want_samples=True)
        start_f, start_h = start_films(W, H, 11)
        cam.film.pixels[...] = start_f
        ref_h = start_h.copy()
        ref_st = integ.render_range(cam, scene, b, e, half=ref_h)
        ref_f = cam.film.pixels.copy()
        assert ref_st.queue_segments == cdiv(ref_st.samples, 64)  # the reference ran one chunk per segment
    single = np.zeros((4, 4), np.uint8)
    single[1, 2] = 1
    for name, m in (("checker", tile_mask("checker", W, H)), ("single", single), ("all", tile_mask("all", W, H))):
        cam.film.pixels[...] = start_f
        h = start_h.copy()
        samples = np.full(so.shape, SENTINEL, F32)
        with ptrs.options(lanes=1, segments=K5):
            st = integ.render_tiles(cam, scene, b, e, m, half=h, samples=samples)
        assert st.passes == 1 and st.queue_segments == K5 and st.samples >= 2 * 64 * K5 and st.error_flags == 0, (name, st.passes, st.queue_segments, st.samples)
        check_tiles_result("%s, five segments" % name, m, W, H, b, e, cam.film.pixels, h, start_f, start_h, ref_f, ref_h, samples, so, st.samples, ref_st, st)


def aov_case(ptrs, orc):
    W, H, spp = 64, 64, 8
    cam, scene = ptrs.import_scene(CORNELL, (W, H))
    return W, H, spp, cam, scene, aov_plan_twin.AovScene(scene), orc.make_params(W, H, spp, 5), sobol_integrator(ptrs, cam, spp, 5)


@pytest.mark.gpu
def test_render_aov_long_segments(ptrs, orc):
    """ptrs_render_aov (k_aov, k_film_aov; per plane k_film) against the plan twin: planes and the 12 floats of every sample, bit for bit."""
    W, H, spp, cam, scene, ts, p, integ = aov_case(ptrs, orc)
    want, want_s = np.zeros((3, H, W), ptrs.abi.FILM_DTYPE), np.zeros((H + 4, W + 4, spp, 12), F32)
    wst = ts.render(cam, p, want, samples=want_s)
    for fused in (1, 0):
        with ptrs.options(lanes=1, segments=K5, aov_fused_film=fused):
            planes, samples = integ.render_aov(cam, scene, want_samples=True)
        st = integ.last_stats
        assert st.passes == 1 and st.queue_segments == K5 and st.samples == 36992 and st.error_flags == 0
        assert (st.samples, st.rays_extension, st.rays_shadow, st.rays_mis) == (wst.samples, wst.rays_extension, 0, 0)
        assert np.array_equal(samples.view(np.uint32), want_s.view(np.uint32))
        got = np.stack([planes[n] for n in ("albedo", "normal", "depth")])
        assert same(got, want), "fused %d: the planes differ from the twin's" % fused


@pytest.mark.gpu
def test_render_aov_tiles_long_segments(ptrs, orc):
    """ptrs_render_aov_tiles on the checkerboard against the twin's range call on the active tiles; inactive tiles untouched."""
    W, H, spp, cam, scene, ts, p, integ = aov_case(ptrs, orc)
    b, e = 1, 7
    start = start_planes(W, H, 5)
    dense_s = np.zeros((H + 4, W + 4, spp, 12), F32)
    ts.render(cam, p, start.copy(), samples=dense_s)
    rng_f = start.copy()
    rng_st = ts.render(cam, p, rng_f, sample_range=(b, e))
    m = tile_mask("checker", W, H)
    f, s = start.copy(), np.full(dense_s.shape, SENTINEL, F32)
    with ptrs.options(lanes=1, segments=K5):
        integ.render_aov_tiles(cam, scene, b, e, m, samples=s, into=as_dict(f))
    st = integ.last_stats
    assert st.passes == 1 and st.queue_segments == K5 and st.samples >= 2 * 64 * K5 and st.error_flags == 0
    check_aov_tiles("checker, five segments", m, W, H, b, e, f, start, rng_f, s, dense_s, st, rng_st)
    want = ts.render(cam, p, start.copy(), sample_range=(b, e), tiles=m)
    assert (st.samples, st.rays_extension) == (want.samples, want.rays_extension)


@pytest.mark.gpu
def test_dump_rays_long_segments(ptrs, orc):
    """ptrs_render_dump_rays (k_dump_rays walks the extension queue's segments).  Round 0: the camera rays of every (pixel, sample) as a
    multiset, computed outside the sampler (test_camera_film_kat).  Round 2: as many rays as the oracle traces at bounce 2 -- its
    extension rays at max_depth 2 less those at max_depth 1: Russian roulette starts later and Cornell has no null-BSDF skips -- and,
    as a multiset, the rays the uncapped device dumps (the oracle does not hand out its rays)."""
    W, H, spp = 64, 64, 8
    cam, scene = ptrs.import_scene(CORNELL, (W, H))
    integ = sobol_integrator(ptrs, cam, spp, 15)
    n = (W + 4) * (H + 4) * spp
    with ptrs.options(lanes=1, segments=K5):
        r0 = ptrs.dump_rays(integ, cam, scene, 0, 2 * n)
        r2 = ptrs.dump_rays(integ, cam, scene, 2, 2 * n)
        integ.render(cam, scene)  # (the dump's own render has no stats: the geometry of the same call without the dump)
    st = integ.last_stats
    assert st.passes == 1 and st.queue_segments == K5 and st.samples == n
    pf, _ = outside_pfilm(W, H, spp, "twin")
    want0 = twin.camera_rays(cam, 1.0 / math.sqrt(spp), pf.reshape(-1, 2))[:, :6]
    assert len(r0) == n and np.isinf(r0[:, 6]).all()
    assert np.array_equal(sorted_rows(r0[:, :6]), sorted_rows(want0))
    O = orc.OracleScene(scene)
    ext = [O.render(cam, orc.make_params(W, H, spp, d), n_threads=8)[2].rays_extension for d in (1, 2)]
    assert len(r2) == ext[1] - ext[0] and 0 < len(r2) < n
    with ptrs.options(lanes=1):
        r2_free = ptrs.dump_rays(integ, cam, scene, 2, 2 * n)
    assert np.array_equal(sorted_rows(r2), sorted_rows(r2_free))


@pytest.mark.gpu
def test_row_cost_probe_long_segments(ptrs):
    """ptrs_render_row_cost on five segments: the per-row counters sum to the ray counts of band renders, as
    test_row_cost_probe_counts_every_ray_once asserts, and are the uncapped probe's."""
    par = importlib.import_module("pathtracer-rs_amd.parallel")
    integ_mod = importlib.import_module("pathtracer-rs_amd.integrator")
    cam, scene = ptrs.import_scene(CORNELL, (64, 64))
    h, depth = 64, 15
    integ = sobol_integrator(ptrs, cam, 1, depth)
    free = par.probe_row_cost(ptrs, cam, scene, depth, cache=False)
    cost, st, c = np.zeros(h, np.float32), ptrs.abi.PtrsStats(), cam.to_abi()
    p = integ.params(cam)
    with ptrs.options(lanes=1, segments=K5):
        integ_mod._check(ptrs.load_library().ptrs_render_row_cost(integ_mod._device_scene(scene, 0).handle, C.byref(c), C.byref(p), C.c_void_p(cost.ctypes.data), C.byref(st)))
        assert st.passes == 1 and st.queue_segments == K5 and st.samples == 68 * 68 and cdiv(cdiv(st.samples, 64), K5) >= 2
        assert np.array_equal(cost, free) and cost.min() > 0
        for a, b in ((2, h - 2), (10, 31), (h // 2, h // 2 + 1)):
            integ.render(cam, scene, row_begin=a, row_end=b)
            assert integ.last_stats.rays == int(cost[a - 2:b + 2].astype(np.float64).sum()), (a, b)
