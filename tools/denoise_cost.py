#!/usr/bin/env python3
"""What the a-trous denoiser costs: python tools/denoise_cost.py [--rounds 7] [--calls 20] [--out profiles/denoise_cost.json]

One process, two workloads (Cornell 1024^2 at 16 spp, scenes.colonnade() 1280x720 at 4 spp, depth 15): the frame is rendered into
device films (ptrs_render_device, ptrs_render_aov_device), then ptrs_denoise_device runs on them with the default parameters.  After a
warm-up of every variant the two forms of the iteration kernel (denoise_lds 0: direct global loads, 1: the LDS-staged tile) alternate
`rounds` times; a round is `calls` consecutive calls of one form.
  per step and form  the iteration kernel's time from the call's own events (PTRS_DENOISE_TIMING): per round the median over its calls,
                     per form the median and the spread (min .. max) of the rounds -- beside the floor of a kernel that reads colour
                     and guide once and writes colour once (48 B / pixel at 8 TB/s) and beside the render call the filter follows
  per form           the whole call on the host clock without the timing events (a call returns with its stream drained)
  ships_lds          per step: the LDS form is faster by more than the spread (its slowest round beats the direct form's fastest)
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
NAMES = ("albedo", "normal", "depth")
ITERATIONS = 5
FLOOR_BYTES_PER_PIXEL, HBM_BYTES_PER_S = 48, 8e12


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v)


def measure(label, cam, scene, spp, depth, rounds, calls):
    W, H = cam.film.width, cam.film.height
    integ = ptrs.PathIntegrator(ptrs.SamplerBuilder(spp, cam.film.get_sample_bounds()), depth)
    new = lambda: torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    film, out, planes = new(), new(), {k: new() for k in NAMES}
    ptr = {k: v.data_ptr() for k, v in planes.items()}
    torch.cuda.synchronize()
    integ.render_device(cam, scene, film.data_ptr())  # warm-up: workspace, code objects, the scene's survival profile
    render_ms = []
    for _ in range(3):
        film.zero_()
        torch.cuda.synchronize()
        t = time.perf_counter()
        integ.render_device(cam, scene, film.data_ptr())
        render_ms.append((time.perf_counter() - t) * 1e3)
    integ.render_aov_device(cam, scene, ptr)
    for k in planes:
        planes[k].zero_()
    torch.cuda.synchronize()
    t = time.perf_counter()
    integ.render_aov_device(cam, scene, ptr)
    aov_ms = (time.perf_counter() - t) * 1e3
    dn = ptrs.Denoiser(W, H)
    call = lambda **kw: dn.denoise_device(film.data_ptr(), ptr, out.data_ptr(), iterations=ITERATIONS, **kw)
    results = {}
    for form in (0, 1):  # warm-up, and the two forms' outputs must be the same bits
        with ptrs.options(denoise_lds=form):
            call()
        results[form] = out.clone()
    assert torch.equal(results[0].view(torch.int32), results[1].view(torch.int32)), "the two forms differ"
    steps = {form: [[] for _ in range(ITERATIONS)] for form in (0, 1)}
    whole = {form: [] for form in (0, 1)}
    for _ in range(rounds):
        for form in (0, 1):
            with ptrs.options(denoise_lds=form):
                per_call = [[] for _ in range(ITERATIONS)]
                for _ in range(calls):
                    st = call(timing=True)
                    for i in range(ITERATIONS):
                        per_call[i].append(st.debug[1 + i] * 1e-6)
                for i in range(ITERATIONS):
                    steps[form][i].append(statistics.median(per_call[i]))
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(calls):
                    call()
                whole[form].append((time.perf_counter() - t) * 1e3 / calls)
    dn.close()
    floor_ms = W * H * FLOOR_BYTES_PER_PIXEL / HBM_BYTES_PER_S * 1e3
    render = statistics.median(render_ms)
    res = dict(workload=label, width=W, height=H, spp=spp, max_depth=depth, render_ms=spread(render_ms), aov_ms=aov_ms, floor_ms_per_iteration=floor_ms, steps=[])
    for i in range(ITERATIONS):
        d, l = spread(steps[0][i]), spread(steps[1][i])
        row = dict(step=1 << i, direct_ms=d, lds_ms=l, direct_over_floor=d["median"] / floor_ms, lds_over_floor=l["median"] / floor_ms,
                   direct_share_of_render=d["median"] / render, lds_share_of_render=l["median"] / render, ships_lds=bool(l["max"] < d["min"]))
        res["steps"].append(row)
        print("%-10s step %2d  direct %.4f ms (%.4f .. %.4f)  lds %.4f ms (%.4f .. %.4f)  floor %.4f ms  lds faster beyond the spread: %s" % (
            label, 1 << i, d["median"], d["min"], d["max"], l["median"], l["min"], l["max"], floor_ms, row["ships_lds"]))
    res["call_ms"] = dict(direct=spread(whole[0]), lds=spread(whole[1]))
    print("%-10s render %.3f ms, aov %.3f ms, denoise call: direct %.4f ms (%.4f .. %.4f), lds %.4f ms (%.4f .. %.4f)" % (
        label, render, aov_ms, res["call_ms"]["direct"]["median"], min(whole[0]), max(whole[0]), res["call_ms"]["lds"]["median"], min(whole[1]), max(whole[1])))
    return res


def main():
    rounds, calls = int(arg("--rounds", 7)), int(arg("--calls", 20))
    path = arg("--out", os.path.join(ROOT, "profiles", "denoise_cost.json"))
    res = dict(build_id=ptrs.build_id(), device=torch.cuda.get_device_name(0), rounds=rounds, calls_per_round=calls, iterations=ITERATIONS, workloads=[])
    cam, scene = ptrs.import_scene(os.path.join(ROOT, "data", "cornell-box.xml"), (1024, 1024))
    res["workloads"].append(measure("cornell", cam, scene, 16, 15, rounds, calls))
    cam, scene = scenes.colonnade()
    res["workloads"].append(measure("colonnade", cam, scene, 4, 15, rounds, calls))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
