"""bench.py --dump-outputs (bench.dump_outputs), on the CPU: a small output is
written whole, a large one as a fixed sample (both ends, then seeded indices)
within the byte budget all files of a call share — the same elements in every
call, so two builds can be compared file for file."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_small_output_whole(tmp_path):
    t = torch.arange(1000, dtype=torch.bfloat16)
    d = torch.arange(10, dtype=torch.float64) / 3
    bench.dump_outputs(str(tmp_path / "o"), {"a": t, "d": d})
    a = np.load(tmp_path / "o" / "a.npy")
    assert a.dtype == np.float32 and np.array_equal(a, t.float().numpy())
    assert np.load(tmp_path / "o" / "d.npy").dtype == np.float64
    assert np.array_equal(np.load(tmp_path / "o" / "d.npy"), d.numpy())


def test_large_output_fixed_sample_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 << 20)
    n = (3 << 20) + 17  # 12 MiB of f32: over either file's share
    g = torch.Generator().manual_seed(3)
    x, y = torch.arange(n, dtype=torch.float32), torch.rand(n, generator=g)  # x: its own index, exact
    for name in ("r1", "r2"):
        bench.dump_outputs(str(tmp_path / name), {"x": x, "y": y})
    files = [tmp_path / r / f for r in ("r1", "r2") for f in ("x.npy", "y.npy")]
    assert sum(os.path.getsize(f) for f in files[:2]) <= 4 << 20
    x1, y1, x2, y2 = (np.load(f) for f in files)
    assert np.array_equal(x1, x2) and np.array_equal(y1, y2)
    edge = 1 << 16
    assert np.array_equal(x1[:edge], x.numpy()[:edge]) and np.array_equal(x1[-edge:], x.numpy()[-edge:])
    # the sample is in index order, inside the tensor, the same indices for both files
    assert x1.size == y1.size > 2 * edge
    idx = x1.astype(np.int64)
    assert (np.diff(idx) >= 0).all() and idx[0] == 0 and idx[-1] == n - 1
    assert np.array_equal(y1, y.numpy()[idx])
