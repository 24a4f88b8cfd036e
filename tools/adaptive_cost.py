#!/usr/bin/env python3
"""What adaptive sampling saves, and what thin, ragged passes cost: python tools/adaptive_cost.py [--rounds 7] [--out profiles/adaptive_cost.json]

One process, two workloads (Cornell 1024^2, ceiling 256, min 16, depth 15; scenes.colonnade() 1280x720, ceiling 64, min 8, depth 15).
Per workload the target comes from the UNIFORM run: the schedule is rendered block by block with render_range up to a quarter of the
ceiling, film_error is asked there, and the target is the median of its tile errors -- about half of the tiles are below it at that
check.  Then, after a warm-up of both, render_converged (the yardstick: every block traces the whole frame and the render stops when the
WORST tile is below the target) and render_adaptive (every block traces the tiles still above it) alternate `rounds` times at that
target, through host films like for like.  Per arm: the host clock around the call (a call returns with its streams drained), the
samples traced, the tiles active per block, and ms per million traced samples.  Two ratios with the spread (min .. max) of the
rounds' own ratios: time adaptive / uniform, and ms per traced sample adaptive / uniform.
The file records the build id of the library measured (pathtracer-rs_amd/build.py: source_hash)."""
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

ptrs = importlib.import_module("pathtracer-rs_amd")
scenes = importlib.import_module("pathtracer-rs_amd.scenes")


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v)


def measure(label, cam, scene, ceiling, min_spp, depth, rounds):
    integ = ptrs.PathIntegrator(ptrs.SamplerBuilder(ceiling, cam.film.get_sample_bounds()), depth)
    # the uniform run up to a quarter of the ceiling, block by block: the target (this is also the warm-up: workspace, survival profile)
    half = np.zeros_like(cam.film.pixels)
    cam.film.clear()
    for (b, m, e) in ptrs.converge_schedule(ceiling, min_spp):
        integ.render_range(cam, scene, b, m, half=half)
        integ.render_range(cam, scene, m, e)
        if e >= max(ceiling // 4, min_spp):
            break
    tiles, _s = ptrs.film_error(cam.film.pixels, half)
    target = float(np.median(tiles["error"]))
    at = e

    def timed(fn):
        cam.film.clear()
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        return out, (time.perf_counter() - t) * 1e3, int(integ.last_stats.samples)
    uniform = lambda: integ.render_converged(cam, scene, target, min_spp=min_spp)
    adaptive = lambda: integ.render_adaptive(cam, scene, target, min_spp=min_spp)
    for fn in (uniform, adaptive, uniform, adaptive):
        timed(fn)
    ms = {"uniform": [], "adaptive": []}
    for _ in range(rounds):
        ru, tu, su = timed(uniform)
        ra, ta, sa = timed(adaptive)
        ms["uniform"].append(tu)
        ms["adaptive"].append(ta)
    per_m = lambda t, s: t / (s / 1e6)
    res = dict(workload=label, width=cam.film.width, height=cam.film.height, ceiling_spp=ceiling, min_spp=min_spp, max_depth=depth, target=target, target_from_check_at=at,
               uniform=dict(ms=spread(ms["uniform"]), samples=su, stopped_at=ru["spp_done"], converged=ru["converged"], history=ru["history"],
                            ms_per_msample=per_m(statistics.median(ms["uniform"]), su)),
               adaptive=dict(ms=spread(ms["adaptive"]), samples=sa, stopped_at=ra["spp_done"], converged=ra["converged"], history=ra["history"], n_tiles=int(ra["tile_spp"].size),
                             tiles_active=[a for _, a, _ in ra["history"]], mean_tile_spp=float(ra["tile_spp"].mean()), ms_per_msample=per_m(statistics.median(ms["adaptive"]), sa)),
               time_ratio=spread([a / u for a, u in zip(ms["adaptive"], ms["uniform"])]),
               ms_per_sample_ratio=spread([per_m(a, sa) / per_m(u, su) for a, u in zip(ms["adaptive"], ms["uniform"])]))
    u, a, tr, pr = res["uniform"], res["adaptive"], res["time_ratio"], res["ms_per_sample_ratio"]
    print("%-10s target %.4g (median tile error at %d spp)" % (label, target, at))
    print("%-10s uniform : %.2f ms (%.2f .. %.2f), stopped at %d spp, %.1f M samples, %.4f ms / M samples" % (label, u["ms"]["median"], u["ms"]["min"], u["ms"]["max"], u["stopped_at"], su / 1e6, u["ms_per_msample"]))
    print("%-10s adaptive: %.2f ms (%.2f .. %.2f), stopped at %d spp, %.1f M samples, %.4f ms / M samples, tiles active per block %s of %d" % (
        label, a["ms"]["median"], a["ms"]["min"], a["ms"]["max"], a["stopped_at"], sa / 1e6, a["ms_per_msample"], a["tiles_active"], a["n_tiles"]))
    print("%-10s time adaptive / uniform %.3f (%.3f .. %.3f); ms per traced sample adaptive / uniform %.3f (%.3f .. %.3f)" % (label, tr["median"], tr["min"], tr["max"], pr["median"], pr["min"], pr["max"]))
    cam.film.clear()
    return res


def main():
    rounds = int(arg("--rounds", 7))
    path = arg("--out", os.path.join(ROOT, "profiles", "adaptive_cost.json"))
    res = dict(build_id=ptrs.build_id(), device=torch.cuda.get_device_name(0), rounds=rounds, workloads=[])
    cam, scene = ptrs.import_scene(os.path.join(ROOT, "data", "cornell-box.xml"), (1024, 1024))
    res["workloads"].append(measure("cornell", cam, scene, 256, 16, 15, rounds))
    cam, scene = scenes.colonnade()
    res["workloads"].append(measure("colonnade", cam, scene, 64, 8, 15, rounds))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
