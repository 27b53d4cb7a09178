"""GPU (-m gpu): tools/bench_mixture_grad.py once, end to end, in a fresh child at its rehearsal size (the 20 000-row scene,
G = 8 and 12, 2 + 3 calls), as tests/test_gpu_mixture_tool.py runs bench_mixture.py: it exits 0, writes one JSON document with
the keys of profiles/mixture_grad_bench.json (the parity section, which a rehearsal leaves out, aside), every time in it is
finite and positive, and at this size both autograd legs run."""
import json
import math
import os
import subprocess
import sys

import pytest

from test_gpu_tools_smoke import structure, times

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("log_density", "log_density_backward", "log_density_backward_without_x", "fourier", "fourier_backward")


def test_bench_mixture_grad_runs_end_to_end_at_the_rehearsal_size(tmp_path):
    out = tmp_path / "result.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_mixture_grad.py"), "--workload", "tiny_rehearsal", "--rehearsal",
                        "--steps", "3", "--warmup", "2", "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert [f.name for f in tmp_path.iterdir()] == ["result.json"]
    doc = json.loads(out.read_text())
    committed = json.load(open(os.path.join(ROOT, "profiles", "mixture_grad_bench.json")))
    assert set(doc) == set(committed) - {"parity"}
    assert all(r <= 1.0 for call in ("log_density_backward", "fourier_backward") for c in committed["parity"][call].values() for r in c.values())
    scene = doc["scenes"]["tiny_rehearsal"]
    assert scene["n_rows"] == scene["n_rows_taking_part"] == 20000 and sorted(scene["grids"]) == ["G=12", "G=8"]
    headline = committed["scenes"]["cfg3_headline"]["grids"]["G=35"]
    for g, rec in scene["grids"].items():
        assert rec["pairs"] == 20000 * rec["queries"]
        for call in CALLS:
            assert set(structure(rec[call])) >= set(structure(headline[call])) - {"speedup_over_torch_autograd"}
            assert rec[call]["steps"] == 3 and rec[call]["pairs_per_second"] > 0
        for leg in ("torch_autograd_log_density", "torch_autograd_fourier"):
            assert rec[leg]["status"] == "run", (g, rec[leg])
    found = list(times(doc))
    assert found, "no time in the document"
    for path, v in found:
        assert math.isfinite(v) and v > 0, (path, v)
