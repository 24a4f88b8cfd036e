"""The 9-entry-column LDS form at its accounted size (9 x 2 048 B of stack column + 528 vectors of staging = 26 880 B = 21 LDS
allocation granules, six workgroups per CU; tools/lds_residency.hip, profiles/lds_residency.json) against the oracle, per sample and
bit for bit: Cornell, which fills 527 of the 528 vectors; the same scene with one more triangle, which no longer fits and must take
the 8 / 640 + overflow form; the fused tail's instantiation of the form; and the traversal-only entry point."""
import numpy as np
import pytest

from conftest import CORNELL

pytestmark = pytest.mark.gpu

LDS9_V4 = 528  # the staging area of the 9-entry form, in 16-byte vectors (ptrs_hip.hip LDS9_V4)


def _render_vs_oracle(ptrs, orc, cam, scene, spp, depth, ref=None, flags=0, **opts):
    """One render against the oracle's samples and ray counts; returns the call's stats and the oracle's answer (for the next caller)."""
    integ = ptrs.PathIntegrator(ptrs.SamplerBuilder(spp, cam.film.get_sample_bounds()), depth)
    cam.film.clear()
    with ptrs.options(**opts):
        samples = integ.render(cam, scene, want_samples=True, flags=flags)
    st = integ.last_stats
    if ref is None:
        _, s_ref, ost = orc.OracleScene(scene).render(cam, orc.make_params(cam.film.width, cam.film.height, spp, depth), n_threads=8, want_samples=True)
        ref = (s_ref, (ost.samples, ost.rays_extension, ost.rays_shadow, ost.rays_mis))
    assert (st.samples, st.rays_extension, st.rays_shadow, st.rays_mis) == ref[1]
    bad = (samples.view(np.uint32) != ref[0].view(np.uint32)).any(axis=-1)
    assert bad.sum() == 0, "%d of %d samples differ" % (bad.sum(), bad.size)
    return st, ref


def test_cornell_fills_the_528_vector_form(ptrs, orc):
    """527 of 528 vectors: the smallest shape at which a staging area one vector too small would corrupt node data.  The form is the
    overflow-free 9-deep one, and the launches are sized for the six workgroups per CU that fit in granules."""
    cam, scene = ptrs.import_scene(CORNELL, (64, 64))
    st, _ = _render_vs_oracle(ptrs, orc, cam, scene, 8, 15, flags=ptrs.abi.FLAG_COUNTERS)
    assert st.stack_lds == 9 and st.lds_form_v4 == 527 and st.lds_form_v4 <= LDS9_V4
    assert st.nodes_visited > 0 and st.tris_tested > 0
    assert (st.resident_wgs_per_cu[0], st.resident_wgs_per_cu[1]) == (6, 6)  # extend, connect


def cornell_plus_one_triangle(ptrs, res):
    """Cornell with one more triangle inside the room: a small quad half floating under the ceiling, away from every surface."""
    cam, scene = ptrs.import_scene(CORNELL, res)
    pos = np.array([[-0.55, 1.60, 0.35], [-0.35, 1.60, 0.35], [-0.35, 1.60, 0.55]], np.float32)
    scene.add_mesh(pos, np.array([[0, 1, 2]], np.uint32), scene.meshes[0]["material"])
    return cam, scene


def test_one_triangle_more_takes_the_8_640_form(ptrs, orc):
    """Just over the limit: more than 528 and at most 544 vectors (what the form held before it was cut to the granule), pair tree of
    depth 9 -- the 8-entry column with 640 vectors and the overflow column, as before the 9-deep form existed."""
    cam, scene = cornell_plus_one_triangle(ptrs, (48, 48))
    st, _ = _render_vs_oracle(ptrs, orc, cam, scene, 4, 6)
    assert LDS9_V4 < st.lds_form_v4 <= 544, st.lds_form_v4
    assert st.stack_lds == 8
    assert (st.resident_wgs_per_cu[0], st.resident_wgs_per_cu[1]) == (6, 6)  # 16 384 + 10 240 B: 21 granules as well


def test_tail_and_trace_entry_points_on_the_528_form(ptrs, orc):
    """k_tail<..., 528, false, 9> takes the whole pass (tail_at = 0) on one lane and on four; ptrs_trace_rays (closest and any hit) on
    rays of test_gpu_parity.test_trace_rays_matches_oracle."""
    cam, scene = ptrs.import_scene(CORNELL, (33, 21))
    ref = None
    for lanes in (1, 4):
        st, ref = _render_vs_oracle(ptrs, orc, cam, scene, 2, 15, ref=ref, tail_at=0, lanes=lanes)
        assert st.lanes == lanes and st.tail_launches == st.passes and st.tail_round == 0
        assert st.stack_lds == 9
    from test_gpu_parity import _camera_rays
    cam, scene = ptrs.import_scene(CORNELL, (64, 64))
    rng = np.random.default_rng(3)
    rays = _camera_rays(cam, 50000, rng, 64, 64)
    tmax = rng.uniform(0.1, 3.0, rays.shape[0]).astype(np.float32)
    pick = np.arange(0, 40000, 2) + 5000  # 20 000 of them: 10 000 from the eye, 10 000 from inside the room
    rays, tmax = rays[pick], tmax[pick]
    o = orc.OracleScene(scene)
    ref_h, _ = o.trace_rays(rays)
    got, _ = ptrs.trace_rays(scene, rays)
    assert np.array_equal(got["prim"], ref_h["prim"])
    hit = ref_h["prim"] >= 0
    assert hit.mean() > 0.5
    for f in ("t", "b0", "b1", "b2"):
        assert np.array_equal(got[f][hit].view(np.uint32), ref_h[f][hit].view(np.uint32)), f
    rays2 = rays.copy()
    rays2[:, 6] = tmax
    ref2, _ = o.trace_rays(rays2, any_hit=True)
    got2, _ = ptrs.trace_rays(scene, rays2, any_hit=True)
    assert np.array_equal(got2["prim"], ref2["prim"])
