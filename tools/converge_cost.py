#!/usr/bin/env python3
"""What the convergence check and the half film cost: python tools/converge_cost.py [--rounds 7] [--calls 20] [--out profiles/converge_cost.json]

One process, two workloads (Cornell 1024^2, scenes.colonnade() 1280x720, depth 15).  After a warm-up of every variant the variants
alternate `rounds` times; a round is `calls` consecutive calls of one variant; per variant the median and the spread (min .. max) of
the rounds' medians.
  error_check     ptrs_film_error_device on the films of a 16-sample render (device films, torch events around the call on its stream,
                  and the host clock: a call returns with its stream drained and the summary on the host) -- beside the floor of a
                  kernel that reads both films once (32 B / pixel at 8 TB/s) and beside the smallest block render_converged renders
                  (the default first block: samples [0, 4) into both films, [4, 8) into the film)
  half_film       ptrs_render_range_device of samples [0, 16) with and without the half film: the price of the second gather
  to_target       informational: render_converged to the ceiling (target 0) with its history, then to a target half-way between the
                  errors of two checks in the middle of that history, beside render() at the count it stopped at and at the ceiling
                  (all four through host films, like for like)
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
FLOOR_BYTES_PER_PIXEL, HBM_BYTES_PER_S = 32, 8e12
RANGE = (0, 16)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v)


def host_ms(fn, calls):
    torch.cuda.synchronize()
    v = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        v.append((time.perf_counter() - t) * 1e3)
    return statistics.median(v)


def measure(label, cam, scene, ceiling, depth, rounds, calls):
    W, H = cam.film.width, cam.film.height
    integ = ptrs.PathIntegrator(ptrs.SamplerBuilder(ceiling, cam.film.get_sample_bounds()), depth)
    new = lambda: torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    film, half = new(), new()
    tiles = torch.zeros((((H + 15) // 16) * ((W + 15) // 16), 2), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()
    torch.cuda.synchronize()
    integ.render_range_device(cam, scene, 0, 8, film.data_ptr(), half.data_ptr())  # warm-up: workspace, code objects, the scene's survival profile
    film.zero_(), half.zero_()
    torch.cuda.synchronize()
    integ.render_range_device(cam, scene, 0, 8, film.data_ptr(), half.data_ptr())
    integ.render_range_device(cam, scene, 8, 16, film.data_ptr())
    check = lambda: ptrs.film_error_device(W, H, film.data_ptr(), half.data_ptr(), tiles.data_ptr(), stream=stream.cuda_stream)
    s = check()

    def check_events():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        check()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def first_block():
        integ.render_range_device(cam, scene, 0, 4, film.data_ptr(), half.data_ptr())
        integ.render_range_device(cam, scene, 4, 8, film.data_ptr())
    with_half = lambda: integ.render_range_device(cam, scene, RANGE[0], RANGE[1], film.data_ptr(), half.data_ptr())
    without = lambda: integ.render_range_device(cam, scene, RANGE[0], RANGE[1], film.data_ptr())
    for fn in (check, first_block, with_half, without):
        fn()
    ev, host, block, r_half, r_plain = [], [], [], [], []
    for _ in range(rounds):
        ev.append(statistics.median([check_events() for _ in range(calls)]))
        host.append(host_ms(check, calls))
        block.append(host_ms(first_block, 3))
        r_plain.append(host_ms(without, 3))
        r_half.append(host_ms(with_half, 3))
    floor_ms = W * H * FLOOR_BYTES_PER_PIXEL / HBM_BYTES_PER_S * 1e3
    res = dict(workload=label, width=W, height=H, ceiling_spp=ceiling, max_depth=depth, floor_ms=floor_ms,
               error_check=dict(events_ms=spread(ev), host_ms=spread(host), first_block_ms=spread(block), max_tile_error=s.max_tile_error, worst_tile=s.worst_tile, valid_pixels=s.valid_pixels),
               half_film=dict(samples=list(RANGE), without_ms=spread(r_plain), with_ms=spread(r_half)))
    e, h, bl = res["error_check"]["events_ms"], res["error_check"]["host_ms"], res["error_check"]["first_block_ms"]
    print("%-10s error check: events %.4f ms (%.4f .. %.4f), host %.4f ms (%.4f .. %.4f), floor %.4f ms, first block %.3f ms (%.3f .. %.3f): the check is %.2f %% of it" % (
        label, e["median"], e["min"], e["max"], h["median"], h["min"], h["max"], floor_ms, bl["median"], bl["min"], bl["max"], 100.0 * h["median"] / bl["median"]))
    a, b = res["half_film"]["without_ms"], res["half_film"]["with_ms"]
    print("%-10s range [%d, %d): %.3f ms (%.3f .. %.3f) without, %.3f ms (%.3f .. %.3f) with the half film: %+.2f %%" % (
        label, RANGE[0], RANGE[1], a["median"], a["min"], a["max"], b["median"], b["min"], b["max"], 100.0 * (b["median"] / a["median"] - 1.0)))
    # to a target (informational)
    def timed(fn):
        cam.film.clear()
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        return out, (time.perf_counter() - t) * 1e3
    timed(lambda: integ.render_converged(cam, scene, 0.0))
    full, full_ms = timed(lambda: integ.render_converged(cam, scene, 0.0))
    hist = full["history"]
    k = len(hist) // 2
    target = 0.5 * (hist[k][1] + hist[k - 1][1]) if k >= 1 and hist[k][1] < hist[k - 1][1] else hist[k][1] * 1.01
    part, part_ms = timed(lambda: integ.render_converged(cam, scene, target))
    _, fixed_full_ms = timed(lambda: integ.render(cam, scene))
    fixed = ptrs.PathIntegrator(ptrs.SamplerBuilder(part["spp_done"], cam.film.get_sample_bounds()), depth)
    timed(lambda: fixed.render(cam, scene))
    _, fixed_part_ms = timed(lambda: fixed.render(cam, scene))
    res["to_target"] = dict(history=hist, to_ceiling_ms=full_ms, fixed_ceiling_ms=fixed_full_ms, target=target, stopped_at=part["spp_done"], converged=part["converged"],
                            to_target_ms=part_ms, fixed_at_stop_ms=fixed_part_ms)
    print("%-10s to the ceiling (%d spp, %d checks): %.2f ms, render(): %.2f ms; to target %.4g: stopped at %d spp in %.2f ms, render() at %d spp: %.2f ms" % (
        label, ceiling, len(hist), full_ms, fixed_full_ms, target, part["spp_done"], part_ms, part["spp_done"], fixed_part_ms))
    print("%-10s history %s" % (label, ", ".join("%d: %.4g" % h_ for h_ in hist)))
    return res


def main():
    rounds, calls = int(arg("--rounds", 7)), int(arg("--calls", 20))
    path = arg("--out", os.path.join(ROOT, "profiles", "converge_cost.json"))
    res = dict(build_id=ptrs.build_id(), device=torch.cuda.get_device_name(0), rounds=rounds, calls_per_round=calls, workloads=[])
    cam, scene = ptrs.import_scene(os.path.join(ROOT, "data", "cornell-box.xml"), (1024, 1024))
    res["workloads"].append(measure("cornell", cam, scene, 256, 15, rounds, calls))
    cam, scene = scenes.colonnade()
    res["workloads"].append(measure("colonnade", cam, scene, 64, 15, rounds, calls))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
