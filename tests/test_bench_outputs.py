"""bench.py's plain run and `--full`: `--dump-outputs DIR` writes what the last timed step computed (float32 / float64 .npy files,
at most 64 MiB in all), `--steps` is the number of timed steps, and the figures beside the headline come only with `--full`."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import CORNELL, ROOT

spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), capture_output=True, text=True, timeout=600, cwd=ROOT)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    return p, lines


def test_dump_outputs_are_seeded_floats_within_the_limit(tmp_path):
    a, b = bench.seeded_sample(1000, 10), bench.seeded_sample(1000, 10)
    assert np.array_equal(a, b) and len(set(a.tolist())) == 10 and np.all(np.diff(a) > 0) and a.max() < 1000
    assert np.array_equal(bench.seeded_sample(7, 10), np.arange(7))
    film = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    bench.dump_outputs(str(tmp_path / "d"), {"film": film, "counts": np.ones(3)})
    assert np.array_equal(np.load(str(tmp_path / "d" / "film.npy")), film) and np.load(str(tmp_path / "d" / "counts.npy")).dtype == np.float64
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "e"), {"big": np.zeros((bench.DUMP_LIMIT // 8) + 1)})
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "f"), {"ints": np.zeros(4, dtype=np.int32)})


def test_steps_must_be_positive():
    p, lines = _bench("--steps", "0")
    assert p.returncode == 2 and not lines and "--steps" in p.stderr


@pytest.mark.gpu
def test_plain_run_dumps_the_film_it_timed(orc, ptrs, tmp_path):
    out = str(tmp_path / "out")
    p, lines = _bench("--gpus", "1", "--res", "64", "--spp", "4", "--steps", "2", "--warmup", "1", "--dump-outputs", out)
    assert p.returncode == 0 and len(lines) == 1, p.stderr[-2000:]
    j = json.loads(lines[0])
    assert j["steps"] == 2 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
    assert (j["unit"], j["higher_is_better"], j["dtype"]) == ("Mray/s", True, "f32") and j["metric"].startswith("Mray/s")
    assert not {"roofline", "film_check", "cpu_baseline", "collective_smoke"} & set(j)
    assert sorted(os.listdir(out)) == ["film.npy", "ray_counts.npy"]
    film, counts = np.load(os.path.join(out, "film.npy")), np.load(os.path.join(out, "ray_counts.npy"))
    assert film.dtype == np.float32 and film.shape == (64, 64, 4) and counts.dtype == np.float64
    cam, scene = ptrs.import_scene(CORNELL, (64, 64))
    fr, _, ost = orc.OracleScene(scene).render(cam, orc.make_params(64, 64, 4, bench.DEPTH), n_threads=8)
    ref = np.concatenate([fr["rgb"], fr["weight"][..., None]], axis=-1).astype(np.float64)
    assert np.sqrt(((film - ref) ** 2).sum() / (ref ** 2).sum()) < 1e-5
    assert counts.tolist() == [ost.rays_extension, ost.rays_shadow, ost.rays_mis, ost.samples]


@pytest.mark.gpu
def test_full_run_keeps_the_figures_beside_the_headline():
    p, lines = _bench("--gpus", "1", "--res", "64", "--spp", "4", "--steps", "1", "--warmup", "0", "--full", "--no-collective-smoke")
    assert p.returncode == 0 and len(lines) == 1, p.stderr[-2000:]
    j = json.loads(lines[0])
    assert j["steps"] == 1 and j["film_check"] == "no fixture for these settings"
    assert set(j["roofline"]["classes"]) == {"traversal", "shade", "tail"} and j["roofline"]["hbm_copy_measured_gbs"] > 0
    assert "single_lane_frame" in j["config"]["launch"]["fused_tail"]
