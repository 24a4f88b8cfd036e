#!/usr/bin/env python3
"""What the first-hit feature planes cost: python tools/aov_cost.py [--rounds 5] [--calls 50] [--out profiles/aov_cost.json]

One process, after a warm-up of every variant, alternating the variants `rounds` times on two workloads (Cornell 1024^2 at 16 spp,
scenes.colonnade() at 4 spp):
  (a) ptrs_render_device at max_depth 0 -- the closest thing a library without the planes can do: one film, no surface work
  (b) ptrs_render_aov_device, three planes, aov_fused_film = 1 (one k_film_aov launch per pass)
  (c) the same with aov_fused_film = 0 (k_film once per plane)
A call takes a millisecond or two, so a round times a window of `calls` consecutive calls of one variant (host clock, the device idle
before and after: every call returns with its stream drained) and reports the time per call; per variant the median and the spread
(min .. max) of the rounds.
The file records the build id of the library measured (pathtracer-rs_amd/build.py: source_hash)."""
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

ptrs = importlib.import_module("pathtracer-rs_amd")
scenes = importlib.import_module("pathtracer-rs_amd.scenes")


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def measure(label, cam, scene, spp, rounds, calls):
    W, H = cam.film.width, cam.film.height
    integ = ptrs.PathIntegrator(ptrs.SamplerBuilder(spp, cam.film.get_sample_bounds()), 0)
    film = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    planes = {k: torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for k in ("albedo", "normal", "depth")}
    ptr = {k: v.data_ptr() for k, v in planes.items()}

    def beauty0():
        return integ.render_device(cam, scene, film.data_ptr())

    def aov(fused):
        with ptrs.options(aov_fused_film=fused):
            return integ.render_aov_device(cam, scene, ptr)

    variants = [("render_depth0", beauty0), ("aov_fused", lambda: aov(1)), ("aov_per_plane", lambda: aov(0))]
    ms = {name: [] for name, _ in variants}
    launches = {}
    for name, fn in variants:  # warm-up: workspace, occupancy queries, code objects
        fn()
    for _ in range(rounds):
        for name, fn in variants:
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(calls):
                st = fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t) * 1e3 / calls)
            launches[name] = dict(kernel_launches=int(st.kernel_launches), film_launches=int(st.film_launches), passes=int(st.passes), lanes=int(st.lanes), samples=int(st.samples))
    out = dict(workload=label, width=W, height=H, spp=spp, n_tris=scene.num_triangles())
    for name, _ in variants:
        v = ms[name]
        out[name] = dict(ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v), ms=v, **launches[name])
        print("%-10s %-14s median %8.3f ms  (%.3f .. %.3f)  %s" % (label, name, out[name]["ms_median"], min(v), max(v), launches[name]))
    b, c = out["aov_fused"], out["aov_per_plane"]
    out["fused_faster_than_per_plane_beyond_spread"] = bool(b["ms_max"] < c["ms_min"])
    return out


def main():
    rounds, calls = int(arg("--rounds", 5)), int(arg("--calls", 50))
    path = arg("--out", os.path.join(ROOT, "profiles", "aov_cost.json"))
    res = dict(build_id=ptrs.build_id(), device=torch.cuda.get_device_name(0), rounds=rounds, calls_per_round=calls, workloads=[])
    cam, scene = ptrs.import_scene(os.path.join(ROOT, "data", "cornell-box.xml"), (1024, 1024))
    res["workloads"].append(measure("cornell", cam, scene, 16, rounds, calls))
    cam, scene = scenes.colonnade()
    res["workloads"].append(measure("colonnade", cam, scene, 4, rounds, calls))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
