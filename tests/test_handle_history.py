"""Every render call gives its own bits whatever its scene handle ran before.

A PtrsScene is not stateless (struct PtrsScene and HipBackend in csrc/ptrs_hip.hip, the pass loop of pt_render.h): it keeps the render
workspace (grown on demand, never shrunk, so a small call runs inside a large call's buffers, on top of their contents), the survival
profile of the last finished unmasked pass of at least 4 096 paths (which places the NEXT call's hand-over to the fused tail), the
traversal stacks' spill columns (one set per lane of the widest render so far), lane streams and events, the event pool, the
occupancy cache and the per-scene option overrides; the Sobol' tables, the process-wide options and the error string are shared by
all handles.  The Python host caches the handle on the RenderScene, so an animated camera, another size, planes or a convergence loop
between frames all live on one handle.  The rest of the suite calls an entry point first or second on its handle, or repeats a call.

Here every case of a menu (tests/handle_cases.py) runs on ONE handle in a given order, and each result is compared with an answer from
the CPU right behind its call: a scripted order in which each hazard happens at least once, the menu backwards, and three shuffles
with fixed seeds.  The cases of S1 (Cornell 64 x 48; S2, textured_env 60 x 40, has A B D E F G H H1 I L P R):

  A  render, 8 spp, depth 15, with samples (two passes of 14 144 paths: feeds the profile)    oracle samples and rays, twin film
  B  render, 4 spp, depth 1 (leaves a three-entry profile whose last entry is 0)              as A
  C  A from a camera beside the box: nine camera rays in ten miss                             as A
  D  render 96 x 80, 16 spp, depth 6, four passes on four lanes (grows the workspace)         as A
  E  render 16 x 16, 1 spp, from C's viewpoint (400 paths: too few to speak for the scene)    as A
  F  A as three row bands into one film                                                       A's film bits
  G  render_range [0, 4) with a half film, then [4, 8)                                        A's film bits; half = the range twin's
  H  render_tiles [0, 8) on a checkerboard of tiles, the other tiles hold a sentinel          active = A's film bits, others untouched
  H1 the same at B's parameters (a masked pass whose profile would differ from A's)           active = B's film bits, others untouched
  I  render_aov with samples                                                                  aov_twin rows
  J  A under a lens                                                                           the host twin under the lens
  K  render with the stratified sampler (3 x 3, 19 dimensions), depth 5                       oracle
  L  trace_rays, closest hit, then any hit with finite t_max, 5 000 rays                      oracle hits, bits of t and barycentrics
  M  render_single_pixel, an interior and an apron pixel                                      oracle
  N  render_adaptive, ceiling 16, min_spp 4 (scripted: right behind D's 30 tiles)             adaptive_twin: film, tile_spp, history
  O  render_progressive of A                                                                  A's film bits
  P  A under segments=64, persist=0, tail=0, fused_epilogue=0, shade_lds=0, lanes=1, tail_paths=16   A's bits
  R  three refusals: spp 0, a stratified sampler with too few dimensions, a negative lens     code and message, the film untouched

No case is skipped in any order: include/ptrs.h names no call that may not follow another ("one render at a time per PtrsScene" is
the only rule).  The scripted orders also assert from PtrsStats that the states were reached (profile placement, workspace growth,
lanes, spill); those assertions compare rounds and byte counts with one another, never with a measured value.
"""
import threading
import time

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded: one HIP runtime per process)

import handle_cases as hc
from handle_cases import NO_TAIL, bits, same_film

SHUFFLE_SEEDS = (20261, 733, 4099)  # constants of the test
ORDERS = ["scripted", "reversed"] + ["shuffle-%d" % s for s in SHUFFLE_SEEDS]
MENUS = {"S1": (hc.s1, hc.s1_scripted), "S2": (hc.s2, hc.s2_scripted), "S3": (hc.s3, hc.s3_scripted)}


def order_of(menu, scripted, which):
    names = list(menu.cases)
    if which == "scripted":
        order = scripted()
    elif which == "reversed":
        order = names[::-1]
    else:
        order = [names[i] for i in np.random.RandomState(int(which.split("-")[1])).permutation(len(names))]
    assert set(order) == set(names), "an order leaves out %s" % sorted(set(names) - set(order))
    return order


# ---- CPU: the menu's answers, cross-checked -------------------------------------------------------------------------------------------
def test_menu_answers_agree_on_the_cpu():
    """Builds every case's expectation and, where two CPU sources exist for it, holds one against the other: oracle samples and ray
    counts against the host twin's for every beauty render of the menus; the twin film of the chained ranges against the twin film of the
    dense call (and the half film against a range call of its own); the tile twin's film against A's on the active tiles; the adaptive
    twin's film against the range twin on every tile, at the tile's own sample count.  About 4 s of CPU time on 16 threads."""
    t0 = time.time()
    n_beauty = 0
    for name, (make, scripted) in MENUS.items():
        m = make()
        m.build()
        for which in ORDERS:
            order_of(m, scripted, which)
        for key, e in m._cache.items():
            if key[0] == "beauty":
                n_beauty += 1
                assert np.array_equal(bits(e["samples"]), bits(e["twin_samples"])) and e["rays"] == e["twin_rays"], (name, key)
                assert e["samples"].max() > 0.0
    assert n_beauty >= 12
    for m in (hc.s1(), hc.s2()):
        a, g, h = m.cases["A"].expect(), m.cases["G"].expect()["g"], m.cases["H"].expect()["twin_tiles"]
        cam = m.cams["A"]
        W, H = cam.film.width, cam.film.height
        assert same_film(g["film"], a["film"]) and same_film(g["half"], g["alone"]) and not same_film(g["half"], a["film"]), m.name
        px = hc.tile_pixels(hc.checkerboard(W, H), W, H)
        assert px.any() and (~px).any()
        assert np.array_equal(bits(h["rgb"][px]), bits(a["film"]["rgb"][px])) and np.array_equal(bits(h["weight"][px]), bits(a["film"]["weight"][px])), m.name
        assert (h["rgb"][~px] == hc.SENTINEL).all() and (h["weight"][~px] == hc.SENTINEL).all()
    m = hc.s1()
    n, cam = m.cases["N"].expect(), m.cams["A"]
    W, H = cam.film.width, cam.film.height
    rs, p = hc.converge_twin.RangeScene(m.scene), hc.orc.make_params(W, H, 16, 5)
    for spp in sorted(set(n["tile_spp"].reshape(-1).tolist())):
        f, _ = rs.render_range(cam, p, 0, spp)
        px = hc.tile_pixels(n["tile_spp"] == spp, W, H)
        assert np.array_equal(bits(n["film"]["rgb"][px]), bits(f["rgb"][px])) and np.array_equal(bits(n["film"]["weight"][px]), bits(f["weight"][px])), spp
    s3 = hc.s3()
    assert s3.stack_bound > 8
    hc.s4().build()
    print("menus built and cross-checked in %.1f s: %d beauty renders; adaptive tile_spp %s" % (time.time() - t0, n_beauty, n["tile_spp"].tolist()))


# ---- GPU: the orders -----------------------------------------------------------------------------------------------------------------
def stats_of(log, pos, name):
    assert log[pos][0] == name, (pos, name, log[pos][0])
    return log[pos][1]


def check_workspace(log, what):
    """The scripted orders start A, A, A and have an A behind their first D: nothing is allocated per call, D grows the workspace, and
    the A behind D runs inside D's buffers."""
    d = [i for i, (nm, _) in enumerate(log) if nm == "D"][0]
    a3 = [stats_of(log, i, "A").device_bytes for i in range(3)]
    d_bytes, after = stats_of(log, d, "D").device_bytes, stats_of(log, d + 1, "A").device_bytes
    print("%s: device_bytes of A, A, A = %s; of D = %d; of the A behind D = %d" % (what, a3, d_bytes, after))
    assert a3[0] == a3[1] == a3[2] > 0, "identical calls report different workspace sizes: something is allocated per call"
    assert d_bytes > a3[2], "D is meant to grow the workspace"
    assert after >= d_bytes, "the workspace shrank: DevBuf::ensure only grows"


def check_s1_script(log):
    """The states the scripted order of S1 is there for, from PtrsStats.  The order runs under tail_paths = 16: with the default 192
    every segment of these passes is below the limit and the hand-over is round 0 whatever the profile says."""
    def a_at(pos):
        st = stats_of(log, pos, "A")
        if st.tail_round != NO_TAIL:
            assert st.tail_launches == st.passes, "A at %d: a hand-over round was chosen but %d of %d passes ran the tail" % (pos, st.tail_launches, st.passes)
        else:
            assert st.tail_launches == 0
        return st.tail_round
    names = [nm for nm, _ in log]
    first, after_a = a_at(0), a_at(1)
    assert first == NO_TAIL, "the handle's first render has no profile to place a hand-over by"
    assert a_at(2) == after_a
    after = {}
    for pos in range(3, len(log)):
        if names[pos] == "A" and names[pos - 1] not in after:
            after[names[pos - 1]] = a_at(pos)
    print("tail_round of A behind A: %d; behind C: %d; behind B: %d; behind D: %d; behind the others: %s" % (
        after_a, after["C"], after["B"], after["D"], {k: v for k, v in after.items() if k not in "CBD"}))
    assert after_a != NO_TAIL, "A's own profile is meant to place a hand-over under tail_paths = 16"
    assert after["C"] < after_a, "the profile of a camera that mostly misses must hand over earlier than A's own"
    # B's pass ends behind round 1, so its profile reads: nothing is alive at round 2 -- and A hands over there, while most of its
    # paths still live (a stale profile costs time, never bits)
    assert after["B"] != after_a and after["B"] <= 2
    # E (400 paths), the feature planes, a masked tile pass, one pixel's paths, plain traversal and refused calls leave the profile alone
    # (DESIGN 4.6, 10, 13, 14): the A behind each of them -- itself behind an A -- hands over where A behind A does
    fed = []
    for k in ("E", "I", "H", "H1", "M", "L", "R"):
        assert names[names.index(k) - 1] == "A"
        if after[k] != after_a:
            fed.append("A behind (A, %s) hands over at round %d" % (k, after[k]))
    assert not fed, "A behind A hands over at round %d, but %s: these calls fed the survival profile" % (after_a, "; ".join(fed))
    check_workspace(log, "S1")
    n_pos = names.index("N")
    assert names[n_pos - 1] == "D"  # (N's 12 tiles run in the tile records, flags and list that D's 30 tiles never used: they are N's own; D leaves the workspace at its largest)


def check_s2_script(log):
    for pos, (nm, st) in enumerate(log):
        if st is not None:
            assert st.tail_launches == 0 and st.tail_round == NO_TAIL, "S2 has several material buckets and glass: no fused tail (%s at %d)" % (nm, pos)
    check_workspace(log, "S2")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ORDERS)
@pytest.mark.parametrize("scene", list(MENUS))
def test_calls_in_any_order_give_their_own_bits(scene, which):
    make, scripted = MENUS[scene]
    m = make()
    m.build()
    order = order_of(m, scripted, which)
    t0 = time.time()
    if scene == "S1" and which == "scripted":
        with hc.ptrs.options(tail_paths=16):
            log = hc.run_order(m, order)
        check_s1_script(log)
    else:
        log = hc.run_order(m, order)
        if scene == "S2" and which == "scripted":
            check_s2_script(log)
    print("%s %s: %d calls on one handle in %.2f s" % (scene, which, len(log), time.time() - t0))
    m.fresh_handle()


@pytest.mark.gpu
def test_refused_render_between_good_ones():
    """S4: Y (depth 100 without roulette: the oracle's bits) and X (depth 200: the library runs the passes, finds a path past Sobol'
    dimension 1024 and answers PTRS_ERR_UNSUPPORTED, a contract test_sobol_dimension_overrun_is_an_error already holds) in the order
    Y, X, Y, X, X, Y on one handle: the error flag of an X must not reach the next call, nor its 201-row counters a 101-row Y."""
    m = hc.s4()
    m.build()
    log = hc.run_order(m, ["Y", "X", "Y", "X", "X", "Y"])
    assert [st is not None for _, st in log] == [True, False, True, False, False, True]
    m.fresh_handle()


@pytest.mark.gpu
def test_two_handles_driven_from_two_threads():
    """include/ptrs.h: "one render at a time per PtrsScene" -- so two handles may be driven from two host threads.  S1's scripted order
    on its handle and S2's on its own, started together behind a barrier on the default device (ctypes releases the GIL during a call);
    each thread holds every result against the CPU answers, which are complete before the threads start.  The knobs of the P and D
    cases are set as per-scene overrides here (ptrs_scene_set_option): a thread must not turn the other's process-wide knobs."""
    menus = [(hc.s1(), hc.s1_scripted()), (hc.s2(), hc.s2_scripted())]
    for m, _ in menus:
        m.build()
        m.per_scene = True
    barrier, errors, done = threading.Barrier(len(menus)), [], []

    def drive(m, order):
        try:
            barrier.wait(timeout=60)
            done.append((m.name, len(hc.run_order(m, order))))
        except BaseException as e:  # noqa: B902  (handed to the main thread)
            errors.append(e)
    threads = [threading.Thread(target=drive, args=mo, daemon=True) for mo in menus]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in threads), "a thread is still inside the library after 120 s"
        if errors:
            raise errors[0]
        assert sorted(done) == sorted((m.name, len(o)) for m, o in menus)
    finally:
        for m, _ in menus:
            m.per_scene = False
            if not any(t.is_alive() for t in threads):
                m.fresh_handle()
