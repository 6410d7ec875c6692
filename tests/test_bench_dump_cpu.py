"""bench.py --dump-outputs on host tensors: every key of the result dict as <key>.npy in float32 / float64, large outputs reduced
to the same fixed seeded row sample, the whole dump within the 64 MB budget, and the same dump from the same inputs."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frame(n):
    g = torch.Generator().manual_seed(1)
    return {"rgb_fine": torch.rand(n, 3, generator=g), "depth_fine": torch.rand(n, generator=g),
            "z_vals_fine": torch.rand(n, 900, generator=g), "mirror_mask_fine": torch.rand(n, generator=g) > 0.5,
            "x_surface_fine": torch.rand(n, 3, generator=g, dtype=torch.float64), "count": torch.arange(5)}


def test_dump_samples_rows_within_budget(tmp_path):
    n = 20000
    out = _frame(n)
    total = bench.dump_outputs(out, str(tmp_path / "a"))
    assert total <= bench.DUMP_BYTES
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == sorted(out)
    k = got["rgb_fine"].shape[0]
    assert 0 < k <= bench.DUMP_ROWS and k * 900 * 4 <= bench.DUMP_BYTES
    rows = np.sort(np.random.default_rng(bench.DUMP_SEED).permutation(n)[:k])
    for name in ("rgb_fine", "depth_fine", "z_vals_fine", "x_surface_fine"):
        assert np.array_equal(got[name], out[name].numpy()[rows]), name
    assert got["mirror_mask_fine"].dtype == np.float32 and np.array_equal(got["mirror_mask_fine"], out["mirror_mask_fine"].numpy()[rows])
    assert got["x_surface_fine"].dtype == np.float64 and got["rgb_fine"].dtype == np.float32
    assert got["count"].dtype == np.float64 and np.array_equal(got["count"], np.arange(5))      # small outputs are written whole
    bench.dump_outputs(_frame(n), str(tmp_path / "b"))
    for name, a in got.items():
        assert np.array_equal(np.load(tmp_path / "b" / (name + ".npy")), a), name


def test_dump_halves_the_sample_to_fit_the_budget(tmp_path):
    n = 20000
    out = {"wide": torch.rand(n, 3000)}          # 8192 rows would be 98 MB
    assert bench.dump_outputs(out, str(tmp_path)) <= bench.DUMP_BYTES
    a = np.load(tmp_path / "wide.npy")
    assert a.shape == (bench.DUMP_ROWS // 2, 3000)
    rows = np.sort(np.random.default_rng(bench.DUMP_SEED).permutation(n)[:a.shape[0]])
    assert np.array_equal(a, out["wide"].numpy()[rows])


def test_dump_keeps_small_outputs_whole(tmp_path):
    out = {"rgb_fine": torch.rand(100, 3), "empty": torch.zeros(0, 3), "scalar": torch.tensor(2.5, dtype=torch.float16)}
    bench.dump_outputs(out, str(tmp_path))
    assert np.array_equal(np.load(tmp_path / "rgb_fine.npy"), out["rgb_fine"].numpy())
    assert np.load(tmp_path / "empty.npy").shape == (0, 3)
    s = np.load(tmp_path / "scalar.npy")
    assert s.dtype == np.float32 and s.shape == () and s == 2.5


def test_bench_refuses_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert r.returncode != 0 and "--steps" in r.stderr
