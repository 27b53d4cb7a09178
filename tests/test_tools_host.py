"""The measurement tools' host side (no GPU): every tool explains itself with --help without touching a GPU and refuses to
run without one; the shared summary, the two rocprofv3 CSV reducers and the one scene-to-input builder give the figures
worked out here."""
import concurrent.futures
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from taichi_3d_gaussian_splatting_amd.synthetic import scene_input, synth, view_pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import harness  # noqa: E402
import pmc_to_json  # noqa: E402

TOOLS = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(ROOT, "tools", "*.py")) if not p.endswith("harness.py"))
HOST_TOOLS = ("asm_diff", "trace_gaps")            # these read files; every other tool measures on the GPU
GPU_TOOLS = [t for t in TOOLS if t not in HOST_TOOLS]
# the tool as __main__ in a child, which then says whether anything initialised the GPU runtime
HELP = ("import runpy, sys, torch\nsys.argv = [sys.argv[1], '--help']\nsys.path.insert(0, {tools!r})\n"
        "try:\n    runpy.run_path(sys.argv[0], run_name='__main__')\nexcept SystemExit as e:\n    code = e.code\n"
        "assert not torch.cuda.is_initialized(), 'GPU runtime initialised by --help'\nsys.exit(code)\n").format(
            tools=os.path.join(ROOT, "tools"))


def _children(argvs):
    """{key: CompletedProcess}, the children run side by side (each is a second or two of imports)"""
    def run(item):
        return item[0], subprocess.run([sys.executable] + item[1], cwd=ROOT, capture_output=True, text=True, timeout=120)
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return dict(pool.map(run, argvs.items()))


@pytest.fixture(scope="module")
def help_runs():
    return _children({t: ["-c", HELP, os.path.join(ROOT, "tools", t + ".py")] for t in TOOLS})


@pytest.fixture(scope="module")
def bare_runs():
    return _children({t: [os.path.join(ROOT, "tools", t + ".py")] for t in GPU_TOOLS})


def test_no_tool_builds_the_input_or_times_with_events_itself():
    """one scene-to-input builder (synthetic.scene_input), one event timer and one library-profiler call site (harness.py;
    bench_densify.py keeps the timer that restores its scene before every repetition)"""
    for t in TOOLS:
        text = open(os.path.join(ROOT, "tools", t + ".py")).read()
        assert "GaussianPointCloudRasterisationInput(" not in text, t
        assert "gs_profile_enable" not in text, t
        assert "Event(enable_timing" not in text or t == "bench_densify", t
    assert not os.path.exists(os.path.join(ROOT, "tools", "r03_batches"))


@pytest.mark.parametrize("tool", TOOLS)
def test_help_exits_zero_without_a_gpu_context(help_runs, tool):
    p = help_runs[tool]
    assert p.returncode == 0, p.stderr[-2000:]
    assert "usage:" in p.stdout, p.stdout[-500:]


@pytest.mark.skipif(torch.cuda.is_available(), reason="this machine has a GPU: the tools would start measuring")
@pytest.mark.parametrize("tool", GPU_TOOLS)
def test_gpu_tool_refuses_to_run_without_a_gpu(bare_runs, tool):
    p = bare_runs[tool]
    assert p.returncode != 0
    assert f"{tool}.py needs the GPU" in p.stderr, p.stderr[-2000:]


def test_summary():
    ms = np.array([4.0, 1.0, 3.0, 2.0, 10.0, 6.0, 5.0, 8.0, 7.0, 9.0])
    # sorted 1..10: the median lies between 5 and 6; numpy's percentile interpolates at rank q (n - 1) = 0.9 and 8.1
    by_hand = dict(ms_median=5.5, ms_p10=1.9, ms_p90=9.1, spread_ms=7.2, steps=10)
    by_numpy = dict(ms_median=np.median(ms), ms_p10=np.percentile(ms, 10), ms_p90=np.percentile(ms, 90),
                    spread_ms=np.percentile(ms, 90) - np.percentile(ms, 10), steps=10)
    got = harness.summary(ms)
    assert list(got) == list(by_hand) and isinstance(got["steps"], int)
    assert all(type(got[k]) is float for k in got if k != "steps")             # plain floats: the result goes to JSON
    for k in by_hand:
        assert got[k] == pytest.approx(by_hand[k], rel=1e-12) and got[k] == pytest.approx(by_numpy[k], rel=1e-12), k


def test_kernel_stats_rows_of_a_committed_record():
    rows = harness.kernel_stats_rows(os.path.join(ROOT, "profiles", "sparse_step_kernel_stats.csv"), ("k_blend_bwd_tile", "k_blend_fwd"))
    assert all("k_blend_bwd_tile" in k or "k_blend_fwd" in k for k in rows) and not any("(" in k for k in rows)
    bwd = [v for k, v in rows.items() if "k_blend_bwd_tile" in k]
    assert len(bwd) == 1 and bwd[0]["calls"] == 520 and bwd[0]["avg_us"] == pytest.approx(230.729844231, rel=1e-12)
    assert any("k_blend_fwd" in k for k in rows)


def test_counter_reducer(tmp_path):
    run = tmp_path / "out" / "host"
    run.mkdir(parents=True)
    (run / "1_counter_collection.csv").write_text(
        '"Dispatch_Id","Kernel_Name","Counter_Name","Counter_Value"\n'
        '1,"void k_blend_fwd<false>(int*, int)","SQ_WAVE_CYCLES",100\n'
        '2,"void k_blend_fwd<true>(int*, int)","SQ_WAVE_CYCLES",300\n'
        '3,"k_filter(float const*)","SQ_WAVE_CYCLES",10\n'
        '4,"k_filter(float const*)","SQ_WAIT_ANY",4\n'
        '5,"k_filter(float const*)","SQ_WAIT_ANY",7\n'
        '6,"at::native::vectorized_elementwise_kernel<4>(int)","SQ_WAVE_CYCLES",999\n')
    got = pmc_to_json.kernel_means(pmc_to_json.run_csvs(str(tmp_path / "out")))
    # template arguments dropped, kernels of other libraries dropped: (100 + 300) / 2, 10, (4 + 7) / 2
    assert got == {"k_blend_fwd": {"SQ_WAVE_CYCLES": 200.0}, "k_filter": {"SQ_WAVE_CYCLES": 10.0, "SQ_WAIT_ANY": 5.5}}


@pytest.mark.parametrize("pose", [False, True])
@pytest.mark.parametrize("requires_grad", [False, True])
def test_scene_input(requires_grad, pose):
    s = synth(37, 48, 32, 0.3, sh_deg=3, seed=5)
    s.point_invalid_mask[3] = 1
    s.point_object_id[5:] = 1
    q, t = (np.repeat(x, 2, 0) for x in view_pose(1, 3))
    inp = scene_input(s, q, t, "cpu", band=2, requires_grad=requires_grad, pose=pose)
    for name, ref, grad in (("point_cloud", s.point_cloud, requires_grad), ("point_cloud_features", s.point_cloud_features, requires_grad),
                            ("point_object_id", s.point_object_id, False), ("point_invalid_mask", s.point_invalid_mask, False),
                            ("q_pointcloud_camera", q, pose), ("t_pointcloud_camera", t, pose)):
        got = getattr(inp, name)
        assert got.device.type == "cpu" and got.requires_grad == grad, name
        a = got.detach().numpy()
        assert a.dtype == ref.dtype and a.shape == ref.shape and a.tobytes() == ref.tobytes(), name
    cam = inp.camera_info
    assert cam.camera_intrinsics.numpy().tobytes() == s.camera_intrinsics.tobytes() and not cam.camera_intrinsics.requires_grad
    assert (cam.camera_height, cam.camera_width, cam.camera_id, inp.color_max_sh_band) == (32, 48, 0, 2)
