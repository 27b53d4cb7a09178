"""GPU (-m gpu): every bench_* tool once, end to end, at the smallest shape the project has (synthetic.SMALL: 20 000 points,
256 x 160) with 2 + 3 iterations, each in a fresh child.  Checked: it exits 0, writes one JSON document, every time in it
is finite and positive, and the document has the keys of the committed record of that tool (profiles/pose_grad_bench.json
and depth_grad_bench.json without their rocprofv3 leg, density_bench.json, sparse_step_bench.json, r03_g_trainer_step.json,
r02_shard_projection.jsonl; bench_channels.py, which has no committed record yet: of its output before the tools shared
a harness).  The numbers at this size are overheads and are compared with nothing."""
import json
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--workload", "tiny_rehearsal"]


def keys(*names, **nested):
    return {**{n: None for n in names}, **nested}


CALLS = keys("ms_median", "ms_p10", "ms_p90", "steps")
WINDOWS = keys("median_ms", "min_ms", "max_ms", "windows_ms", "calls_per_window")
ITERATIONS = keys("fused_loss_and_adam_image_in_place", "fused_loss_and_adam", "torch_loss_and_adam")
CHANNEL = keys("passes_staged", "channel_chunk", "chunks", "new_fwd_plus_bwd_ms", "staged_fwd_plus_bwd_ms", "speedup", "largest_spread_ms",
               "faster_by_more_than_the_spread", "forward_walks_per_chunk", "backward_walks_per_chunk", "forward_max_diff_to_staged",
               "backward_max_diff_to_staged",
               **{leg: keys("ms_median", "ms_p10", "ms_p90", "spread_ms", "steps") for leg in ("new_fwd", "new_bwd", "old_fwd", "old_bwd")})
CASES = {
    "bench_pose_grad": (TINY, keys("workload", "step", "device", modes={f"{m}@kobj{k}": CALLS for k in (1, 8)
                                                                        for m in ("points", "points+pose", "pose")})),
    "bench_depth_grad": (TINY, keys("workload", "step", "device", modes={m: CALLS for m in ("image", "image+depth", "image+depth+alpha")})),
    "bench_channels": (["--configs", "tiny_rehearsal", "--channels", "3,16"],
                       keys("device", "steps", "warmup", "timing", configs={"tiny_rehearsal": keys(
                           "n_points", "n_points_in_camera", "n_keys", "height", "width", "k_blend_fwd_ms",
                           channels={"3": CHANNEL, "16": CHANNEL})})),
    "bench_sparse_step": (TINY, keys("component", "method", "source_digest", "device", workloads={"tiny_rehearsal": keys(
        "n_points", "image", "n_points_in_camera", "n_touched", "touched_of_in_camera", "touched_of_all", "compaction_workgroups",
        gs_touched_rows_ms=WINDOWS, training_iteration_ms={"dense": WINDOWS, "selective": WINDOWS},
        adam_two_tensors_ms=keys("selective_plus_list_median_ms", dense=WINDOWS, selective=WINDOWS, selective_fixed_grid_2048=WINDOWS))})),
    "bench_trainer_step": (TINY, keys("component", loss_fwd_bwd_ms=keys("fused_gs_loss_l1_ssim", "torch_conv2d_autograd"),
                                      adam_two_tensors_ms=keys("fused_gs_adam_step", "torch_optim_adam"),
                                      training_iteration_ms=ITERATIONS, training_iterations_per_s=ITERATIONS)),
    "bench_densify": (["--rows", "20000", "--in-camera", "8000"],
                      keys("what", "n_rows", "n_valid", "n_in_camera", "reps", "device", "densify_fraction_of_valid", "pruned_fraction_of_valid",
                           "hip_select_apply_ms_median", "hip_select_apply_ms_min", "hip_select_ms_median", "torch_reference_ms_median",
                           "torch_reference_ms_min", "speedup_median",
                           counts=keys("floaters", "transparent", "densify", "fillable", "over", "under", "valid_before", "valid_after",
                                       "single_frame", "single_frame_viewspace"))),
    "bench_shard_projection": (TINY, keys("workload", "steps", "wait_per_view_ms", "begun_back_to_back_ms")),
}


def structure(doc):
    return {k: structure(v) for k, v in doc.items()} if isinstance(doc, dict) else None


def times(doc, path=()):
    """(path, value) of every number stored under a name that says milliseconds (a spread, a difference of two, left out)"""
    if isinstance(doc, dict):
        for k, v in doc.items():
            yield from times(v, path + (k,))
    elif isinstance(doc, list):
        for i, v in enumerate(doc):
            yield from times(v, path + (i,))
    elif isinstance(doc, (int, float)) and not isinstance(doc, bool):
        names = [p for p in path if isinstance(p, str)]
        if any("ms" in p.split("_") for p in names) and "spread" not in names[-1] and names[-1] not in ("steps", "calls_per_window"):
            yield path, doc


@pytest.mark.parametrize("tool", list(CASES))
def test_tool_runs_end_to_end_at_the_smallest_shape(tool, tmp_path):
    args, want = CASES[tool]
    out = tmp_path / "result.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool + ".py"), *args, "--steps", "3", "--warmup", "2", "--out", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert [f.name for f in tmp_path.iterdir()] == ["result.json"]
    doc = json.loads(out.read_text())               # one document: anything behind it is an error
    assert structure(doc) == want
    found = list(times(doc))
    assert found, "no time in the document"
    for path, v in found:
        assert math.isfinite(v) and v > 0, (path, v)
