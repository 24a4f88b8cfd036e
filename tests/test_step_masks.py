"""The traversal step's lane masks (ptrs_hip.hip: StepMasks, lf_node_visit; pt_bvh.h: slab_finish_mask).  The LDS-form node visit takes
its two slab decisions as ballots of the single compares, and one set of masks per step serves the vote, the step loop's exit test and the
retire / refill bookkeeping of the lane-refill kernels.  None of it changes a visit or a test, so everything here is held bit for bit
against the oracle: rays in the planes of the tree's boxes (the `ordered` compare of the mask form) through the frame's own extension
kernel under every vote policy, queue segments whose size sits on either side of the refill thresholds (a wave that never fills, fills
exactly, drains), and whole renders handed to the fused tail, which calls the same segment functions (and, under the votes the tail is
not compiled for, through the three kernels per round)."""
import numpy as np
import pytest

from conftest import CORNELL

pytestmark = pytest.mark.gpu

VOTES = (-1, 0, 1, 2)  # every value the `vote` option accepts (include/ptrs.h)
BITS = ("b0", "b1", "b2")


def _lattice_scene(ptrs, n):
    """n^3 axis-aligned unit squares on integer planes (two triangles each): every box face of the tree lies in a coordinate plane."""
    s = ptrs.RenderScene()
    m = s.add_material(ptrs.abi.MAT_MATTE, [s.const_rgb([0.5, 0.5, 0.5])])
    pos, idx = [], []
    for i in range(n):
        for j in range(n):
            for k in range(n):
                ax = (i + j + k) % 3
                o = np.array([i, j, k], np.float32) * 2.0
                u, v = np.eye(3, dtype=np.float32)[(ax + 1) % 3], np.eye(3, dtype=np.float32)[(ax + 2) % 3]
                b = len(pos)
                pos += [o, o + u, o + u + v, o + v]
                idx += [[b, b + 1, b + 2], [b, b + 2, b + 3]]
    s.add_mesh(np.array(pos, np.float32), np.array(idx, np.uint32), m)
    return s


def _same_hits(got, ref, fields):
    assert np.array_equal(got["prim"], ref["prim"])
    hit = ref["prim"] >= 0
    for f in fields:
        assert np.array_equal(got[f][hit].view(np.uint32), ref[f][hit].view(np.uint32)), f


@pytest.mark.parametrize("n,form", ((3, 0), (3, 2), (6, 0)))
def test_box_plane_rays_through_the_frame_kernels(ptrs, orc, n, form):
    """The rays of test_gpu_parity.test_rays_inside_box_planes (origins on the half-integer lattice, the 26 axis-sign directions: 0 * inf =
    NaN in the slab test) through ptrs_trace_bench, which launches the frame's lane-refill extension kernel, under every vote policy.
    The hit record of that kernel carries the primitive and the barycentrics and no distance (trace_bench returns t = 0), so prim, b0,
    b1, b2 are compared on trace_bench's answer and t on ptrs_trace_rays' answer for the same rays."""
    dirs = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)], np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    with ptrs.options(node_form=form):
        scene = _lattice_scene(ptrs, n)
        g = np.arange(-1, 2 * n + 1, 0.5, dtype=np.float32)
        rng = np.random.default_rng(11 + n)
        o = rng.choice(g, (6000, 3))
        d = dirs[rng.integers(0, len(dirs), 6000)]
        rays = np.concatenate([o, d, np.full((6000, 1), np.inf, np.float32)], axis=1).astype(np.float32)
        ho, _ = orc.OracleScene(scene).trace_rays(rays)
        assert (ho["prim"] >= 0).sum() > 500
        _same_hits(ptrs.trace_rays(scene, rays)[0], ho, ("t",) + BITS)
        for vote in VOTES:
            with ptrs.options(vote=vote):
                _, hits = ptrs.trace_bench(scene, rays, repeats=1, want_hits=True)
            _same_hits(hits, ho, BITS)


@pytest.fixture(scope="module")
def cornell_round1(ptrs, orc):
    """Cornell 48 x 48: the extension rays of round 1 (origins on the room's surfaces, every direction) and the oracle's hits."""
    cam, scene = ptrs.import_scene(CORNELL, (48, 48))
    integ = ptrs.PathIntegrator(ptrs.SamplerBuilder(4, cam.film.get_sample_bounds()), 6)
    with ptrs.options(lanes=1):
        rays = ptrs.dump_rays(integ, cam, scene, 1, 1 << 20)
    assert len(rays) >= 129
    rays = rays[:129].copy()
    ref, _ = orc.OracleScene(scene).trace_rays(rays)
    assert (ref["prim"] >= 0).sum() > 64
    return scene, rays, ref


@pytest.mark.parametrize("refill", (16, 32, 64))
def test_segment_sizes_around_the_refill_thresholds(ptrs, cornell_round1, refill):
    """The first n rays, n on either side of 16, 32, 64 and of two waves' worth, under the three idle-lane thresholds: the exit test of the
    step loop and the refill decision read the step's masks where a wave never fills, fills exactly, and drains.  n records come back,
    each the oracle's."""
    scene, rays, ref = cornell_round1
    for n in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129):
        with ptrs.options(refill=refill):
            _, hits = ptrs.trace_bench(scene, rays[:n], repeats=1, want_hits=True)
        assert len(hits) == n
        assert (hits["prim"] >= 0).sum() == (ref["prim"][:n] >= 0).sum()
        _same_hits(hits, ref[:n], BITS)


@pytest.fixture(scope="module")
def cornell_oracle(ptrs, orc):
    cam, scene = ptrs.import_scene(CORNELL, (48, 48))
    _, ref, ost = orc.OracleScene(scene).render(cam, orc.make_params(48, 48, 8, 15), n_threads=8, want_samples=True)
    return ref, (ost.samples, ost.rays_extension, ost.rays_shadow, ost.rays_mis)


@pytest.mark.parametrize("vote", (-1, 2, 0, 1))
@pytest.mark.parametrize("lanes", (1, 4))
def test_whole_pass_handed_to_the_tail_matches_oracle(ptrs, cornell_oracle, lanes, vote):
    """Cornell 48 x 48, 8 spp, depth 15, handed over at round 0 (tail_at = 0), on one lane and on four: sample by sample and ray count
    by ray count against the oracle.  k_tail is compiled with ONE vote policy, for the LDS form "the extension stage votes, the
    connection stage does not": that is vote = -1 (the default) and vote = 2, and under those the whole pass runs in k_tail (one launch
    per pass, from round 0), whose extension and connection stages are the same segment functions.  vote = 0 and vote = 1 ask
    for other votes: no tail is launched, and the same segment functions run in the three kernels per round -- without the vote in
    either (0) and with it in both (1), which is the only place the LDS-form connect kernel votes."""
    ref, counts = cornell_oracle
    cam, scene = ptrs.import_scene(CORNELL, (48, 48))
    integ = ptrs.PathIntegrator(ptrs.SamplerBuilder(8, cam.film.get_sample_bounds()), 15)
    with ptrs.options(tail_at=0, lanes=lanes, vote=vote):
        samples = integ.render(cam, scene, want_samples=True)
    st = integ.last_stats
    assert st.lanes == lanes
    if vote in (-1, 2):
        assert st.tail_launches == st.passes and st.tail_round == 0
    else:
        assert st.tail_launches == 0
    assert (st.samples, st.rays_extension, st.rays_shadow, st.rays_mis) == counts
    bad = (samples.view(np.uint32) != ref.view(np.uint32)).any(axis=-1)
    assert bad.sum() == 0, "%d of %d samples differ" % (bad.sum(), bad.size)
