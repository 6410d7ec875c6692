"""The bench line's contract on one GPU (bench.py): one JSON line with the keys the driver parses, the roofline object and
the numbers that round 6 moved to the top level.  A bounded --full run (MNRF_BENCH_LEGS) of one timed frame; a plain run carries the
headline keys and none of the secondary legs."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_line_schema(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["MNRF_BENCH_LEGS"] = "headline,other,train"
    dump = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline",
                        "--dump-outputs", str(dump)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "one JSON line at N = 1"
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 1 and d["warmup"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 1e5 and abs(d["value"] - d["config"]["rays_per_step_per_gpu"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) <= 1e-9 and 0.05 < rf["frac"] < 0.34
    assert rf["traffic"] is None or rf["traffic"] > 2e8      # (bytes per launch from profiles/traffic.json; >= the 226 MB algorithmic)
    # round 6: what a harness that keeps only top-level values must still see
    assert d["fp32_rays_per_s"] > 1e5 and 0.5 < d["fp32_frac"] < 1.0
    assert len(d["train_ms"]) == 5 and d["train_ms"][0] > 0 and d["train_ms"][0] == d["train_step"]["ms_per_step"]
    assert d["train_route"] == d["train_step"]["route"] == "graph" and 0.05 < d["train_frac"] < 0.3
    assert d["legs_requested"] == ["headline", "other", "train"]
    # --dump-outputs: the result dict of the timed frame, float32 / float64, at most 64 MB, the frame's colour among them
    import numpy as np
    files = sorted(dump.glob("*.npy"))
    assert files and sum(f.stat().st_size for f in files) <= (64 << 20) + 128 * len(files)     # (+ the .npy headers)
    arrs = {f.stem: np.load(f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert arrs["rgb_fine"].ndim == 2 and arrs["rgb_fine"].shape[1] == 3 and np.isfinite(arrs["rgb_fine"]).all()


SECONDARY_KEYS = ("fp32_rays_per_s", "fp32_frac", "split_rays_per_s", "split_frac", "strong_scaling", "with_host_maps", "maps_only_fused",
                  "train_step", "train_ms", "train_route", "train_frac", "hash_grid_variant", "roughness_variant",
                  "trained_weights_variant", "config1", "cpu_baseline", "legs_requested")


def test_plain_bench_runs_the_headline_only(tmp_path):
    """Without --full the run sets up, warms up, times its frames, dumps and prints the line: the headline keys, the roofline of the
    timed frames, no secondary leg, and little time outside the frames."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "MNRF_BENCH_LEGS")}
    dump = tmp_path / "outputs"
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(dump)], env=env, capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "one JSON line at N = 1"
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "dtype", "config",
              "roofline"):
        assert k in d, k
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "rays/s" and d["higher_is_better"] is True
    assert d["value"] > 1e5 and abs(d["value"] - d["config"]["rays_per_step_per_gpu"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert 0.05 < d["roofline"]["frac"] < 0.34 and d["roofline"]["launches"] > 0
    assert not [k for k in SECONDARY_KEYS if k in d], [k for k in SECONDARY_KEYS if k in d]
    assert (dump / "rgb_fine.npy").exists()
    # set-up, first launches, dump and exit (about 3 s measured); the secondary legs, now behind --full, added over a minute
    assert wall - (d["steps"] + d["warmup"]) * d["ms_per_step"] * 1e-3 < 30.0, wall
