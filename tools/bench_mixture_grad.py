#!/usr/bin/env python3
"""Time the gradients of the scene-as-mixture calls (mixture_grad.log_density_backward / fourier_backward:
gs_mixture_log_density_backward, gs_mixture_fourier_backward, include/gs_mixture_grad.h) on cuda:0 beside their forward calls,
at G = 35 and G = 96 over the two scenes of bench_mixture.py:

  cfg3_headline   the 500 000-row scene of BASELINE config 3
  rows_1e5        synth() with 100 000 rows, otherwise the same parameters

and put torch autograd through the closed form (tests/mixture_ref.py, f32, on the same device) beside them: the only route to
these gradients without the kernels.  Its graph holds several (queries, rows, 3) tensors, so it runs the queries in slices of
at most 2^27 / (3 rows) and lets torch accumulate the slices' gradients; the leg is first projected from its first slice
(timed alone, after a warm-up) and runs in full only if the projection is within --baseline-seconds (60); otherwise the record
says "not run" and why.

Per call of ours: device events around each call after the warm-up (harness.per_call_ms: host side and the output allocation
included), median / p10 / p90.  The upstream gradients are seeded (magnitudes in (0.5, 1.5), random signs).  The density's
backward is timed with and without the gradient to x; backward_over_forward is the ratio of the medians.

Without --rehearsal the record also holds the parity ratios of tests/test_gpu_mixture_grad.py: measured error / bar of every
group of every (N, P) case of the two size sweeps and of the chunked case.  --rehearsal shrinks the grids to G = 8 and 12 and
drops the parity section (a run of the plumbing); --workload NAME measures that one scene (a name of synthetic.make_scene, or
rows_1e5).

Writes the result (with _native.source_digest()) to --out, default profiles/mixture_grad_bench.json, and prints it."""
import argparse
import os
import sys

import harness as H
import torch

import mixture_grad_ref as GR
import mixture_ref as R
from bench_mixture import scene_tensors
from taichi_3d_gaussian_splatting_amd import _native, mixture, mixture_grad

DEV = "cuda:0"
SLICE_ELEMENTS = 2 ** 27


def autograd_leg(scene, queries, g, fourier, centre, a):
    """torch autograd through the closed form in f32 on the device, the queries in slices -> the record of the leg"""
    pc, feat, mask = scene
    n = int(pc.shape[0])
    rows = max(1, min(int(queries.shape[0]), SLICE_ELEMENTS // (3 * n)))
    slices = list(zip(queries.split(rows), g.split(rows)))
    print(f"bench_mixture_grad: autograd leg of {len(slices)} slices of {rows} queries", file=sys.stderr, flush=True)

    def run(parts):
        pc_, feat_ = pc.clone().requires_grad_(True), feat.clone().requires_grad_(True)
        for q_, g_ in parts:
            if fourier:
                out = torch.view_as_real(R.fourier(pc_, feat_, mask, q_, centre, torch.float32, rows=rows))
            else:
                out = R.log_density(pc_, feat_, mask, q_, torch.float32, rows=rows)
            (out * g_).sum().backward()
        return pc_.grad, feat_.grad

    try:
        run(slices[:1])                                               # untimed: allocator and library warm-up
        one = float(H.wall_ms(lambda: run(slices[:1]), 1, 0))
        projected = one * len(slices) / 1e3
        if projected > a.baseline_seconds:
            return {"status": "not run", "first_slice_ms": one, "slices": len(slices), "queries_per_slice": rows, "projected_seconds": projected,
                    "reason": f"one slice of {len(slices)} took {one:.0f} ms: {projected:.0f} s projected (limit {a.baseline_seconds} s)"}
        return {"status": "run", "first_slice_ms": one, "slices": len(slices), "queries_per_slice": rows,
                "all_slices_ms": float(H.wall_ms(lambda: run(slices), 1, 0))}
    except torch.cuda.OutOfMemoryError as e:
        torch.cuda.empty_cache()
        return {"status": "not run", "reason": "out of device memory: " + str(e).split("\n")[0][:160]}


def measure_scene(name, grids, a):
    scene = scene_tensors(name)
    n_part = int(mixture.takes_part(scene).sum())
    bbox = mixture.bounding_box(scene)
    centre = (bbox[0] + bbox[1]) / 2.0
    out = {"n_rows": int(scene[0].shape[0]), "n_rows_taking_part": n_part, "grids": {}}
    for G in grids:
        print(f"bench_mixture_grad: {name}, G = {G}", file=sys.stderr, flush=True)
        x = mixture.sample_grid(bbox, G).reshape(-1, 3).contiguous()
        k = mixture.frequency_grid(bbox, G).reshape(-1, 3).contiguous()
        g1 = GR.upstream(G ** 3, 1, seed=G).reshape(-1).to(DEV)
        g2 = GR.upstream(G ** 3, 2, seed=G + 1).to(DEV)
        log_p = mixture.log_density(scene, x)
        rec = {"queries": G ** 3, "pairs": n_part * G ** 3, "query_chunks": mixture_grad.query_chunks(int(scene[0].shape[0]), G ** 3)[0]}
        calls = (("log_density", lambda: mixture.log_density(scene, x)),
                 ("log_density_backward", lambda: mixture_grad.log_density_backward(scene, x, log_p, g1)),
                 ("log_density_backward_without_x", lambda: mixture_grad.log_density_backward(scene, x, log_p, g1, want_x=False)),
                 ("fourier", lambda: mixture.fourier(scene, k, centre)),
                 ("fourier_backward", lambda: mixture_grad.fourier_backward(scene, k, centre, g2)))
        for call, fn in calls:
            t = H.summary(H.per_call_ms(fn, a.steps, a.warmup))
            rec[call] = dict(t, pairs_per_second=rec["pairs"] / (t["ms_median"] * 1e-3))
        for call, forward in (("log_density_backward", "log_density"), ("log_density_backward_without_x", "log_density"),
                              ("fourier_backward", "fourier")):
            rec[call]["backward_over_forward"] = round(rec[call]["ms_median"] / rec[forward]["ms_median"], 2)
        rec["torch_autograd_log_density"] = autograd_leg(scene, x, g1, False, centre, a)
        rec["torch_autograd_fourier"] = autograd_leg(scene, k, g2, True, centre, a)
        for call, leg in (("log_density_backward", "torch_autograd_log_density"), ("fourier_backward", "torch_autograd_fourier")):
            if rec[leg]["status"] == "run":
                rec[call]["speedup_over_torch_autograd"] = round(rec[leg]["all_slices_ms"] / rec[call]["ms_median"], 1)
        out["grids"][f"G={G}"] = rec
        torch.cuda.empty_cache()
    return out


def parity_ratios():
    """measured error / bar of every group of every case of tests/test_gpu_mixture_grad.py's sweeps (its assertions included)"""
    import test_gpu_mixture_grad as T
    out = {"log_density_backward": {}, "fourier_backward": {}}
    for kind, call in (("density", "log_density_backward"), ("fourier", "fourier_backward")):
        for n in T.N_SIZES:
            total = len(T.case(kind, n)[0])
            for p in T.P_SIZES:
                if kind == "density" and (n, p) == (1, 1):
                    continue
                out[call][f"N={n},P={T.count(p, total)}"] = T.sweep_case(kind, n, p)
        n = T.CB + 1
        p = T.chunked_size(n)
        scene = T.T.scene(n)
        q, g = T.T.query_list(scene[0], scene[1], kind)[:p], T.upstream(kind, n, p)
        out[call][f"N={n},P={p} (three query chunks)"] = T.check_case(kind, n, p, scene, q, g, T.closed(kind, scene, q, g),
                                                                     T.autograd(kind, scene, q, g, torch.float32))
    for call in list(out):
        out[call + "_largest_ratio"] = max(r for c in out[call].values() for r in c.values())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(H.ROOT, "profiles", "mixture_grad_bench.json"))
    ap.add_argument("--workload", help="one scene instead of cfg3_headline and rows_1e5: a name of synthetic.make_scene, or rows_1e5")
    ap.add_argument("--steps", type=int, default=5, help="timed calls of each entry point per scene and grid")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rehearsal", action="store_true", help="G = 8 and 12 instead of 35 and 96, no parity section")
    ap.add_argument("--baseline-seconds", type=float, default=60.0, help="an autograd leg runs in full only if projected within this")
    a = ap.parse_args()
    H.require_gpu("bench_mixture_grad.py")
    grids = (8, 12) if a.rehearsal else (35, 96)
    names = [a.workload] if a.workload else ["cfg3_headline", "rows_1e5"]
    out = {"component": "gradients of the scene as a Gaussian mixture: the backward of the log-density and of the closed-form Fourier transform on a "
                        "G^3 grid (gs_mixture_log_density_backward, gs_mixture_fourier_backward) beside their forward calls and beside torch "
                        "autograd through the closed form in slices, one GPU (see device)",
           "method": "ours: device events around each call after the warm-up, median / p10 / p90 of the per-call milliseconds; autograd legs: "
                     "host clock around one run ending in a synchronise, first projected from the first slice and run in full only within "
                     "the limit given; pairs = rows taking part x queries; backward_over_forward = ratio of the medians",
           "source_digest": _native.source_digest(), "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "components_per_workgroup": mixture_grad.COMPONENTS_PER_WORKGROUP, "queries_per_chunk": mixture_grad.QUERIES_PER_CHUNK,
           "run_length": mixture_grad.RUN_LENGTH, "baseline_limits": {"seconds": a.baseline_seconds, "slice_elements": SLICE_ELEMENTS},
           "scenes": {name: measure_scene(name, grids, a) for name in names}}
    if not a.rehearsal:
        out["parity"] = parity_ratios()
    H.write_json(out, a.out)


if __name__ == "__main__":
    main()
