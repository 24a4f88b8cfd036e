#!/usr/bin/env python3
"""What the planes of an adaptive film cost: python tools/aov_adaptive_cost.py [--rounds 7] [--out profiles/aov_adaptive_cost.json]

One process, tools/adaptive_cost.py's two workloads and targets (Cornell 1024^2, ceiling 256, min 16, depth 15; scenes.colonnade()
1280x720, ceiling 64, min 8, depth 15; the target is the median tile error of the uniform run at a quarter of the ceiling).  After a
warm-up of all three, per round and in this order: render_adaptive (host films; the run whose tile_spp the planes follow),
render_aov_adaptive_device on that tile_spp (planes in device memory, cleared before the clock starts) and a dense render_aov_device
at the ceiling -- `rounds` times, alternated.  Per arm: the host clock around the call (a call returns with its streams drained),
medians with min .. max, the samples traced, ms per million traced samples; and the ratio masked / dense of the ms per traced sample
with the spread of the rounds' own ratios -- the figure to hold against the beauty's tile form (1.21 .. 1.27 x).
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
NAMES = ("albedo", "normal", "depth")


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v)


def measure(label, cam, scene, ceiling, min_spp, depth, rounds):
    integ = ptrs.PathIntegrator(ptrs.SamplerBuilder(ceiling, cam.film.get_sample_bounds()), depth)
    W, H = cam.film.width, cam.film.height
    half = np.zeros_like(cam.film.pixels)
    cam.film.clear()
    for (b, m, e) in ptrs.converge_schedule(ceiling, min_spp):  # (tools/adaptive_cost.py's target; also the warm-up of the beauty path)
        integ.render_range(cam, scene, b, m, half=half)
        integ.render_range(cam, scene, m, e)
        if e >= max(ceiling // 4, min_spp):
            break
    tiles, _s = ptrs.film_error(cam.film.pixels, half)
    target = float(np.median(tiles["error"]))
    dev = {k: torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for k in NAMES}
    dptr = {k: v.data_ptr() for k, v in dev.items()}

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        return out, (time.perf_counter() - t) * 1e3, int(integ.last_stats.samples)

    def beauty():
        cam.film.clear()
        return clock(lambda: integ.render_adaptive(cam, scene, target, min_spp=min_spp))

    def planes(run):
        for v in dev.values():
            v.zero_()
        return clock(run)
    masked = lambda ts: planes(lambda: integ.render_aov_adaptive_device(cam, scene, ts, dptr, min_spp=min_spp))
    dense = lambda: planes(lambda: integ.render_aov_device(cam, scene, dptr))
    for _ in range(2):
        r, _t, _n = beauty()
        masked(r["tile_spp"])
        dense()
    ms = {"adaptive": [], "aov_adaptive": [], "aov_dense": []}
    for _ in range(rounds):
        r, tb, sb = beauty()
        _o, tm, sm = masked(r["tile_spp"])
        _o, td, sd = dense()
        ms["adaptive"].append(tb)
        ms["aov_adaptive"].append(tm)
        ms["aov_dense"].append(td)
    per_m = lambda t, s: t / (s / 1e6)
    res = dict(workload=label, width=W, height=H, ceiling_spp=ceiling, min_spp=min_spp, max_depth=depth, target=target,
               n_tiles=int(r["tile_spp"].size), tiles_active=[a for _, a, _ in r["history"]], mean_tile_spp=float(r["tile_spp"].mean()),
               adaptive=dict(ms=spread(ms["adaptive"]), samples=sb, ms_per_msample=per_m(statistics.median(ms["adaptive"]), sb)),
               aov_adaptive=dict(ms=spread(ms["aov_adaptive"]), samples=sm, ms_per_msample=per_m(statistics.median(ms["aov_adaptive"]), sm)),
               aov_dense=dict(ms=spread(ms["aov_dense"]), samples=sd, ms_per_msample=per_m(statistics.median(ms["aov_dense"]), sd)),
               aov_time_over_beauty=spread([a / b for a, b in zip(ms["aov_adaptive"], ms["adaptive"])]),
               ms_per_sample_ratio=spread([per_m(a, sm) / per_m(d, sd) for a, d in zip(ms["aov_adaptive"], ms["aov_dense"])]))
    for k in ("adaptive", "aov_adaptive", "aov_dense"):
        print("%-10s %-13s %.2f ms (%.2f .. %.2f), %.1f M samples, %.4f ms / M samples" % (label, k, res[k]["ms"]["median"], res[k]["ms"]["min"], res[k]["ms"]["max"], res[k]["samples"] / 1e6, res[k]["ms_per_msample"]))
    tb, pr = res["aov_time_over_beauty"], res["ms_per_sample_ratio"]
    print("%-10s planes / the adaptive render they follow %.3f (%.3f .. %.3f); ms per traced sample masked / dense %.3f (%.3f .. %.3f); tiles active per block %s of %d" % (
        label, tb["median"], tb["min"], tb["max"], pr["median"], pr["min"], pr["max"], res["tiles_active"], res["n_tiles"]))
    cam.film.clear()
    return res


def main():
    rounds = int(arg("--rounds", 7))
    path = arg("--out", os.path.join(ROOT, "profiles", "aov_adaptive_cost.json"))
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
