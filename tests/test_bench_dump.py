"""CPU: bench.py --dump-outputs writes float32/float64 .npy files within its byte budget, whole when they fit and as the
same seeded sample otherwise."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _headline_sized(seed):
    """The arrays a cfg3_headline step returns, at their real shapes (1920x1088, 5e5 points)."""
    g = torch.Generator().manual_seed(seed)
    return {"image": torch.rand(1088, 1920, 3, generator=g), "depth": torch.rand(1088, 1920, generator=g),
            "pixel_valid_point_count": torch.randint(0, 900, (1088, 1920), generator=g, dtype=torch.int32),
            "grad_point_cloud": torch.randn(500_000, 3, generator=g),
            "grad_point_cloud_features": torch.randn(500_000, 56, generator=g)}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_headline_outputs_fit_the_budget_and_sample_the_same_positions(tmp_path):
    arrays = _headline_sized(0)
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == set(arrays)
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BYTES
    for k, v in a.items():
        assert v.dtype == np.float32 and np.array_equal(v, b[k]), k
    # fits its share: written whole, shape kept; integers as float32
    assert a["depth"].shape == (1088, 1920) and np.array_equal(a["pixel_valid_point_count"], arrays["pixel_valid_point_count"].numpy())
    assert a["grad_point_cloud"].shape == (500_000, 3)
    # larger than its share: a sample of the flattened array, in order, at positions that depend only on the shape
    feat = arrays["grad_point_cloud_features"].numpy().reshape(-1)
    s = a["grad_point_cloud_features"]
    assert s.ndim == 1 and s.nbytes <= bench.DUMP_BYTES // len(arrays)
    idx = np.sort(np.random.default_rng(0).choice(feat.size, s.size, replace=False))
    assert np.array_equal(s, feat[idx])
    other = _headline_sized(1)
    bench.dump_outputs(str(tmp_path / "c"), other)
    assert np.array_equal(_load(tmp_path / "c")["grad_point_cloud_features"],
                          other["grad_point_cloud_features"].numpy().reshape(-1)[idx])


def test_float64_is_kept(tmp_path):
    x = torch.arange(12, dtype=torch.float64).reshape(3, 4) / 3
    bench.dump_outputs(str(tmp_path), {"x": x})
    y = np.load(tmp_path / "x.npy")
    assert y.dtype == np.float64 and np.array_equal(y, x.numpy())
