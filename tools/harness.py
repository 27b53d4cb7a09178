"""What the measurement tools under tools/ share: the import paths, the refusal to run without a GPU, the timers and their
summary, the library's and rocprofv3's per-kernel times, the seeded backward of the parity tools and the JSON writer.
Importing it puts the checkout and tests/ (parity_util, density_ref) on sys.path and touches no GPU."""
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def require_gpu(tool_name):
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool_name} needs the GPU: nothing is measured without one")


def use_library(file_name):
    """GSRAST_LIB defaults to a diagnostic build of the library; call before the package is imported"""
    os.environ.setdefault("GSRAST_LIB", os.path.join(ROOT, "taichi_3d_gaussian_splatting_amd", "lib", file_name))


# ---- timers -----------------------------------------------------------------------------------------------------------
def per_call_ms(fn, steps, warmup):
    """-> array of `steps` per-call milliseconds: a device-event pair around each fn() (its host side included), after
    `warmup` untimed calls and a synchronise; one synchronise after the last call, before the events are read"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in ev])


def summary(ms):
    p10, p90 = float(np.percentile(ms, 10)), float(np.percentile(ms, 90))
    return dict(ms_median=float(np.median(ms)), ms_p10=p10, ms_p90=p90, spread_ms=p90 - p10, steps=int(len(ms)))


def window_ms(fn, n):
    """per-call time of n calls between two device events; the window ends in a synchronise on the second event"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def alternate(variants, n, warm, repeats=5):
    """variants {name: fn or (fn, environment for its calls)}: each called `warm` times untimed, one synchronise, then
    window_ms(fn, n) of each in turn, `repeats` rounds -> {name: {median_ms, min_ms, max_ms, windows_ms, calls_per_window}}"""
    variants = {name: v if isinstance(v, tuple) else (v, {}) for name, v in variants.items()}

    def run(fn, env, count, timed):
        os.environ.update(env)
        try:
            if timed:
                return window_ms(fn, count)
            for _ in range(count):
                fn()
        finally:
            for k in env:
                del os.environ[k]
    for fn, env in variants.values():
        run(fn, env, warm, False)
    torch.cuda.synchronize()
    got = {name: [] for name in variants}
    for _ in range(repeats):
        for name, (fn, env) in variants.items():
            got[name].append(run(fn, env, n, True))
    return {name: dict(median_ms=round(statistics.median(v), 5), min_ms=round(min(v), 5), max_ms=round(max(v), 5),
                       windows_ms=[round(x, 5) for x in v], calls_per_window=n) for name, v in got.items()}


def wall_ms(fn, n, warm):
    """per-call host-clock milliseconds of n calls of fn(): `warm` untimed calls and a synchronise first; the clock stops
    after a synchronise behind the last call"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


# ---- per-kernel times -------------------------------------------------------------------------------------------------
def library_kernel_ms(module, device, kernel_name, fn, warm, reps):
    """mean milliseconds of one kernel over `reps` calls of fn(), by the library's own profiler (gs_profile_enable for that
    kernel alone, after `warm` untimed calls and a synchronise; read after a synchronise behind the last call)"""
    from taichi_3d_gaussian_splatting_amd import _native
    L = _native.lib()
    names = L.gs_kernel_names().decode().split(",")
    kid = names.index(kernel_name)
    ctx = module._ctx_for(device)
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    _native.check(L.gs_profile_enable(ctx, C.c_uint64(1 << kid)), "gs_profile_enable")
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ms, cnt = (C.c_double * len(names))(), (C.c_int64 * len(names))()
    _native.check(L.gs_profile_read(ctx, ms, cnt, len(names), 1), "gs_profile_read")
    _native.check(L.gs_profile_enable(ctx, C.c_uint64(0)), "gs_profile_enable")
    return ms[kid] / max(cnt[kid], 1)


def kernel_stats_rows(csv_path, name_filters):
    """rows of a rocprofv3 kernel_stats.csv whose kernel name holds one of name_filters -> {kernel: {calls, avg_us}}"""
    rows = {}
    with open(csv_path) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Name", "")
            if any(k in name for k in name_filters):
                rows[name.split("(")[0]] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3}
    return rows


def rocprof_kernel_stats(child_argv, name_filters, seconds=900):
    """One `rocprofv3 --kernel-trace --stats` run (no other trace domain, no counters) of `python <child_argv>` under a
    time limit; a child that fails or runs out of time ends the tool -> kernel_stats_rows of its summary"""
    out = tempfile.mkdtemp(prefix="kernel_stats_")
    cmd = ["timeout", "-k", "10", str(seconds), "rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "run",
           "--output-format", "csv", "--", sys.executable] + list(child_argv)
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    return kernel_stats_rows(stats[0], name_filters) if stats else {}


# ---- the parity tools' backward ---------------------------------------------------------------------------------------
def seeded_backward(module, inp, seed=0, **backward_args):
    """forward, then backward against g = 2 (image - target), target ~ U[0,1) from default_rng(seed) (or from the
    generator given as seed) -> (image, g)"""
    image = module(inp)[0]
    rng = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
    target = torch.tensor(rng.uniform(0, 1, image.shape).astype(np.float32), device=image.device)
    g = 2.0 * (image.detach() - target)
    image.backward(g, **backward_args)
    return image, g


def write_json(result, out_path, indent=1):
    """writes the result to out_path (its directory made; nothing written when out_path is None) and prints it"""
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=indent)
            fh.write("\n")
    print(json.dumps(result))
