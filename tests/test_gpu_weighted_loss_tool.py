"""GPU (-m gpu): tools/bench_weighted_loss.py once, end to end, in a fresh child at tiny sizes (64x96 and 48x80 pictures, the
20 000-row rehearsal scene, 2 + 3 calls, 2 rounds), as tests/test_gpu_mixture_tool.py runs its tool: it exits 0, writes one
JSON document with the keys of profiles/weighted_loss_bench.json, and every window time in it is finite and positive.  The
numbers at this size are overheads and are compared with nothing."""
import json
import math
import os
import subprocess
import sys

import pytest

from test_gpu_tools_smoke import WINDOWS, structure

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_LEGS = ("weighted_fused", "unweighted_fused", "weighted_torch_conv2d_autograd")


def test_bench_weighted_loss_runs_end_to_end_at_tiny_sizes(tmp_path):
    out = tmp_path / "result.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_weighted_loss.py"), "--sizes", "64x96,48x80", "--workload",
                        "tiny_rehearsal", "--steps", "3", "--warmup", "2", "--repeats", "2", "--out", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert [f.name for f in tmp_path.iterdir()] == ["result.json"]
    doc = json.loads(out.read_text())
    committed = json.load(open(os.path.join(ROOT, "profiles", "weighted_loss_bench.json")))
    assert set(doc) == set(committed) == {"component", "method", "loss_fwd_bwd_ms", "target_ms", "training_iteration_ms", "loss_kernels_rocprofv3", "notes"}
    assert sorted(doc["loss_fwd_bwd_ms"]) == ["48x80", "64x96"]
    assert sorted(doc["target_ms"]) == ["48x80_factor_1", "48x80_factor_2", "64x96_factor_1", "64x96_factor_2"]
    windows = []
    for key, rec in doc["loss_fwd_bwd_ms"].items():
        assert set(rec) == set(LOSS_LEGS) | {"weighted_over_unweighted", "torch_over_weighted", "abs_difference_fused_torch",
                                              "weighted_share_of_pixels"}
        assert set(rec) == set(next(iter(committed["loss_fwd_bwd_ms"].values())))
        assert rec["abs_difference_fused_torch"] < 1e-4 and 0 < rec["weighted_share_of_pixels"] < 1
        windows += [rec[leg] for leg in LOSS_LEGS]
    for key, rec in doc["target_ms"].items():
        assert set(rec) == {"target_with_weight", "target", "with_weight_over_plain", "output"} and rec["output"][0] == 4
        windows += [rec["target_with_weight"], rec["target"]]
    it = doc["training_iteration_ms"]
    assert set(it) == {"with_weights", "without_weights", "with_over_without", "workload"} and it["workload"] == "tiny_rehearsal"
    windows += [it["with_weights"], it["without_weights"]]
    for w in windows:
        assert structure(w) == WINDOWS and w["calls_per_window"] >= 1 and len(w["windows_ms"]) == 2
        for v in [w["median_ms"], w["min_ms"], w["max_ms"], *w["windows_ms"]]:
            assert math.isfinite(v) and v > 0, w
    assert isinstance(doc["notes"], list) and doc["loss_kernels_rocprofv3"] == "not measured"      # no --rocprof here
