#!/usr/bin/env python3
"""What a thin lens costs a frame: python tools/lens_cost.py [--rounds 7] [--out profiles/lens_cost.json]

One process, bench.py's two first workloads (Cornell 1024^2 at 256 spp; scenes.colonnade() 1280x720 at 64 spp; depth 15).  Per workload
the focus is taken by ptrs_camera_focus_distance at the film's centre and the aperture is 2 % of it.  After a warm-up of both, the pinhole
render and the lens render of the same camera alternate `rounds` times through render_device into one device film (cleared before each;
the host clock around the call, which returns with its streams drained).  Per arm: ms per frame and the rays traced; the ratio lens /
pinhole with the spread (min .. max) of the rounds' own ratios.  A lens changes the paths, so the ratio of ms per ray is given too.
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


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v)


def measure(label, cam, scene, spp, depth, rounds):
    W, H = cam.film.width, cam.film.height
    focus = ptrs.focus_distance(cam, scene, (W / 2.0, H / 2.0))
    lens = cam.with_lens(0.02 * focus, focus)
    integ = ptrs.PathIntegrator(ptrs.SamplerBuilder(spp, cam.film.get_sample_bounds()), depth)
    film = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")

    def timed(camera):
        film.zero_()
        torch.cuda.synchronize()
        t = time.perf_counter()
        st = integ.render_device(camera, scene, film.data_ptr())
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, int(st.rays)
    for camera in (cam, lens, cam, lens):
        timed(camera)
    ms = {"pinhole": [], "lens": []}
    rays = {}
    for _ in range(rounds):
        for name, camera in (("pinhole", cam), ("lens", lens)):
            t, rays[name] = timed(camera)
            ms[name].append(t)
    ratio = [b / a for a, b in zip(ms["pinhole"], ms["lens"])]
    per_ray = [r * rays["pinhole"] / rays["lens"] for r in ratio]
    out = dict(workload=label, spp=spp, depth=depth, focal_distance=focus, lens_radius=0.02 * focus, rays=rays,
               ms={k: spread(v) for k, v in ms.items()}, lens_over_pinhole=spread(ratio), lens_over_pinhole_per_ray=spread(per_ray))
    print("%s: focus %.4g, pinhole %.2f ms (%.2f - %.2f), lens %.2f ms (%.2f - %.2f), lens / pinhole %.4f (%.4f - %.4f), per ray %.4f (%.4f - %.4f)" % (
        label, focus, out["ms"]["pinhole"]["median"], min(ms["pinhole"]), max(ms["pinhole"]), out["ms"]["lens"]["median"], min(ms["lens"]), max(ms["lens"]),
        statistics.median(ratio), min(ratio), max(ratio), statistics.median(per_ray), min(per_ray), max(per_ray)), flush=True)
    return out


def main():
    rounds = int(arg("--rounds", 7))
    out_path = arg("--out", os.path.join(ROOT, "profiles", "lens_cost.json"))
    res = []
    cam, scene = ptrs.import_scene(os.path.join(ROOT, "data", "cornell-box.xml"), (1024, 1024))
    res.append(measure("cornell 1024x1024", cam, scene, 256, 15, rounds))
    cam, scene = scenes.colonnade((1280, 720))
    res.append(measure("colonnade 1280x720", cam, scene, 64, 15, rounds))
    doc = dict(tool="tools/lens_cost.py", build_id=ptrs.build_id(), device=torch.cuda.get_device_name(0), rounds=rounds, workloads=res)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
