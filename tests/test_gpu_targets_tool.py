"""GPU (-m gpu): tools/bench_targets.py once, end to end, in a fresh child with 1 + 2 calls per leg and without the training
iteration: it exits 0 and writes one JSON document with every leg of every factor, every time finite and positive."""
import json
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("a_cpu_resize_and_copy_pageable_ms", "a_cpu_resize_and_copy_pinned_ms", "b_device_interpolate_from_f32_ms", "c_kernel_from_uint8_ms")


def test_bench_targets_runs_end_to_end(tmp_path):
    out = tmp_path / "result.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_targets.py"), "--skip-iteration", "--steps", "2", "--warmup", "1",
                        "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert [f.name for f in tmp_path.iterdir()] == ["result.json"]
    doc = json.loads(out.read_text())
    assert set(doc) == {"component", "cpu_threads", "resident_bytes_per_image", "per_target_ms"}
    assert doc["resident_bytes_per_image"] == {"uint8_hwc_16_byte_pitch": 1088 * 1920 * 3, "f32_chw": 1088 * 1920 * 12}
    assert list(doc["per_target_ms"]) == ["factor_1", "factor_2", "factor_4"]
    for factor, legs in doc["per_target_ms"].items():
        f = int(factor.split("_")[1])
        assert legs["target"] == [3, 1088 // f, 1920 // f]
        assert all(math.isfinite(legs[name]) and legs[name] > 0 for name in LEGS), legs
        # torch's own device path in f32 against the kernel: the two share the operator, not the weights' precision
        assert 0.0 <= legs["max_abs_difference_b_c"] <= 2e-5
    committed = json.load(open(os.path.join(ROOT, "profiles", "targets_bench.json")))
    assert set(committed) == set(doc) | {"training_iteration_ms_factor_1_cfg3"}
    assert {k: set(v) for k, v in committed["per_target_ms"].items()} == {k: set(v) for k, v in doc["per_target_ms"].items()}
