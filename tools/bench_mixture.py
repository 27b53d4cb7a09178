#!/usr/bin/env python3
"""Time the scene-as-mixture calls (mixture.log_density / mixture.fourier: gs_mixture_log_density, gs_mixture_fourier,
include/gs_mixture.h) on cuda:0 at G = 35 and G = 96 -- the two grid sizes of the reference's FTGMM.py -- over two scenes:

  cfg3_headline   the 500 000-row scene of BASELINE config 3
  rows_1e5        synth() with 100 000 rows, otherwise the same parameters

and put the reference's way of doing the same beside them, restated here in torch on the same device (not imported, not
copied): the density as MixtureSameFamily(Categorical, MultivariateNormal(scale_tril = cholesky(R S^2 R^T))).log_prob one grid
slice at a time, the transform as sum w exp(-i k.(mu - c) - 1/2 k^T Sigma k) over covariance matrices in batches of 500
frequencies.  A baseline leg is first projected from its first slice or batch (timed alone, after the set-up); it runs in
full only if the projection is within --baseline-seconds (60), its largest tensor within --baseline-gib (48) and below 2^31
elements (the transform leg at 500 000 rows, whose (500, N, 3, 3) tensor has 2.25e9, ended in a memory-access fault of the
device when it was tried as two batched matmul; the leg is written with broadcast products now and is not started at that
size); otherwise the record says "not run" and why.

Per call of ours: device events around each call after the warm-up (harness.per_call_ms: host side and the output
allocation included), median / p10 / p90; pairs per second = rows that take part x queries / median; and the share of the
157.3 TFLOP/s f32 vector peak that the builder's own count of f32 operations per pair amounts to -- a fused
multiply-add counted as 2, an exponential as 1:
  density   27 = 3 (x - mu) + 15 (3 x 3 whitening: 3 mul, 6 fma) + 5 (sum of squares) + 1 (c - .) + 1 max + 1 sub + 1 exp
                 + 1 add, and 3/4 for the running maximum's rescale once per four records
  transform 66 = 5 (phase) + 15 + 5 (|S R^T k|^2) + 2 (exp, weight) + 35 (range reduction, two polynomials, quadrant) + 4

Without --rehearsal the record also holds the parity ratios of tests/test_gpu_mixture.py: measured error / bar for every (N, P)
case of the two size sweeps.  --rehearsal shrinks the grids to G = 8 and 12 and drops the parity section (a run of the
plumbing); --workload NAME measures that one scene (a name of synthetic.make_scene, or rows_1e5).

Writes the result (with _native.source_digest()) to --out, default profiles/mixture_bench.json, and prints it."""
import argparse
import os
import sys

import harness as H
import torch

from taichi_3d_gaussian_splatting_amd import _native, mixture
from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, synth

DEV = "cuda:0"
PEAK_TFLOPS = 157.3
FLOPS_PER_PAIR = {"log_density": 27, "fourier": 66}
BATCH = 500
ELEMENT_LIMIT = 2 ** 31


def scene_tensors(name):
    s = synth(100_000, 1920, 1088, 0.02, sh_deg=3, seed=0) if name == "rows_1e5" else make_scene(name)
    return tuple(torch.tensor(a, device=DEV) for a in (s.point_cloud, s.point_cloud_features, s.point_invalid_mask))


# ---- the reference's way, restated ---------------------------------------------------------------------------------------------
def reference_mixture(scene):
    """-> (MixtureSameFamily, weights, means, covariances) as define_gmm builds them (f32; the f64 fallback of the Cholesky
    factor for the rows where f32 fails)"""
    from torch.distributions.categorical import Categorical
    from torch.distributions.mixture_same_family import MixtureSameFamily
    from torch.distributions.multivariate_normal import MultivariateNormal
    pc, feat, mask = scene
    valid = mask == 0
    mu, f = pc[valid], feat[valid]
    x, y, z, w = f[:, :4].unbind(-1)
    two_s = 2.0 / (f[:, :4] * f[:, :4]).sum(-1)
    R = torch.stack((1 - two_s * (y * y + z * z), two_s * (x * y - z * w), two_s * (x * z + y * w),
                     two_s * (x * y + z * w), 1 - two_s * (x * x + z * z), two_s * (y * z - x * w),
                     two_s * (x * z - y * w), two_s * (y * z + x * w), 1 - two_s * (x * x + y * y)), -1).reshape(-1, 3, 3)
    S = R * torch.exp(f[:, 4:7]).unsqueeze(-2)
    cov = torch.bmm(S, S.transpose(-2, -1))
    tril, info = torch.linalg.cholesky_ex(cov)
    bad = info > 0
    tril = torch.where(bad[:, None, None], torch.linalg.cholesky_ex(cov.double())[0].float(), tril)
    alphas = torch.sigmoid(f[:, 7])
    gmm = MixtureSameFamily(Categorical(alphas), MultivariateNormal(mu, scale_tril=tril, validate_args=False))
    return gmm, alphas / alphas.sum(), mu, cov


def reference_density_slice(gmm, coords, i):
    return gmm.log_prob(coords[i])


def reference_fourier_batch(weights, mu, cov, centre, k):
    """one batch of frequencies through the reference's formula, with its (batch, N, 3, 3) intermediate: Sigma k and k^T (Sigma k)
    as broadcast products and sums (the reference writes them as two torch.matmul over batch x N matrices of 3 x 3)"""
    shifted = mu - centre
    k_e = k.unsqueeze(-2)                                             # (B, 1, 3)
    ik_dot_mu = -1j * torch.sum(k_e * shifted, dim=-1)                # (B, N)
    sigma_k = (cov.unsqueeze(0) * k_e.unsqueeze(-2)).sum(-1)          # (B, N, 3, 3) -> (B, N, 3)
    k_sigma_k = (k_e * sigma_k).sum(-1)                               # (B, N)
    return (weights.unsqueeze(0) * torch.exp(ik_dot_mu - 0.5 * k_sigma_k)).sum(dim=-1)


def baseline_leg(first, rest, n_parts, largest_elements, a):
    """first(): the first slice / batch; rest(): all of them; largest_elements: the f32 elements of the leg's largest tensor.
    -> the record of the leg"""
    print(f"bench_mixture: reference leg of {n_parts} parts", file=sys.stderr, flush=True)
    largest_gib = largest_elements * 4 / 2 ** 30
    if largest_elements >= ELEMENT_LIMIT:
        return {"status": "not run", "reason": f"its largest tensor alone has {largest_elements:.3g} elements ({largest_gib:.1f} GiB); no leg with "
                "2^31 elements or more in one tensor is started: the transform leg at 500 000 rows (500 x N x 3 x 3 = 2.25e9) ended in a "
                "memory-access fault of the device when it was tried"}
    if largest_gib > a.baseline_gib:
        return {"status": "not run", "reason": f"its largest tensor alone is {largest_gib:.1f} GiB (limit {a.baseline_gib} GiB)"}
    try:
        first()                                                       # untimed: allocator and library warm-up
        one = float(H.wall_ms(first, 1, 0))
        projected = one * n_parts / 1e3
        if projected > a.baseline_seconds:
            return {"status": "not run", "first_part_ms": one, "parts": n_parts, "projected_seconds": projected,
                    "reason": f"one part of {n_parts} took {one:.0f} ms: {projected:.0f} s projected (limit {a.baseline_seconds} s)"}
        return {"status": "run", "first_part_ms": one, "parts": n_parts, "all_parts_ms": float(H.wall_ms(rest, 1, 0))}
    except torch.cuda.OutOfMemoryError as e:
        torch.cuda.empty_cache()
        return {"status": "not run", "reason": "out of device memory: " + str(e).split("\n")[0][:160]}


def measure_scene(name, grids, a):
    scene = scene_tensors(name)
    n_part = int(mixture.takes_part(scene).sum())
    bbox = mixture.bounding_box(scene)
    centre = (bbox[0] + bbox[1]) / 2.0
    out = {"n_rows": int(scene[0].shape[0]), "n_rows_taking_part": n_part, "grids": {}}
    gmm, weights, mu, cov = reference_mixture(scene)
    n_valid = int(mu.shape[0])
    for G in grids:
        print(f"bench_mixture: {name}, G = {G}", file=sys.stderr, flush=True)
        coords = mixture.sample_grid(bbox, G)
        x, k = coords.reshape(-1, 3).contiguous(), mixture.frequency_grid(bbox, G).reshape(-1, 3).contiguous()
        rec = {"queries": G ** 3, "pairs": n_part * G ** 3}
        for call, fn in (("log_density", lambda: mixture.log_density(scene, x)), ("fourier", lambda: mixture.fourier(scene, k, centre))):
            t = H.summary(H.per_call_ms(fn, a.steps, a.warmup))
            rate = rec["pairs"] / (t["ms_median"] * 1e-3)
            rec[call] = dict(t, pairs_per_second=rate, f32_operations_per_pair=FLOPS_PER_PAIR[call],
                             fraction_of_vector_peak=rate * FLOPS_PER_PAIR[call] / (PEAK_TFLOPS * 1e12))
        rec["reference_log_prob_by_slices"] = baseline_leg(
            lambda: reference_density_slice(gmm, coords, 0),
            lambda: [reference_density_slice(gmm, coords, i) for i in range(G)], G, G * G * n_valid * 3, a)
        batches = list(k.split(BATCH))
        rec["reference_transform_by_batches_of_500"] = baseline_leg(
            lambda: reference_fourier_batch(weights, mu, cov, centre, batches[0]),
            lambda: [reference_fourier_batch(weights, mu, cov, centre, b) for b in batches], len(batches),
            min(BATCH, G ** 3) * n_valid * 9, a)
        for call, leg in (("log_density", "reference_log_prob_by_slices"), ("fourier", "reference_transform_by_batches_of_500")):
            if rec[leg]["status"] == "run":
                rec[call]["speedup_over_reference"] = round(rec[leg]["all_parts_ms"] / rec[call]["ms_median"], 1)
        out["grids"][f"G={G}"] = rec
        torch.cuda.empty_cache()
    return out


def parity_ratios():
    """measured error / bar of every (N, P) case of tests/test_gpu_mixture.py's two size sweeps"""
    import test_gpu_mixture as T
    out = {"log_density": {}, "fourier": {}}
    for n in T.N_SIZES:
        x, ref, f32, drop = T.density_case(n)
        k, fref, phase, fdrop = T.fourier_case(n)
        for p in T.P_SIZES:
            px, pk = T.count(p, len(x)), T.count(p, len(k))
            bar = T.density_bar(ref[:px], f32[:px], drop[:px])
            err = float((T.gpu_log_density(*T.scene(n), x[:px]).double() - ref[:px]).abs().max())
            out["log_density"][f"N={n},P={px}"] = dict(error=err, bar=bar, ratio=err / bar)
            bar = T.fourier_bar(fref[:pk], phase[:pk], fdrop[:pk])
            err = float((T.gpu_fourier(*T.scene(n), k[:pk]).to(torch.complex128) - fref[:pk]).abs().max())
            out["fourier"][f"N={n},P={pk}"] = dict(error=err, bar=bar, ratio=err / bar)
    for call in list(out):
        out[call + "_largest_ratio"] = max(c["ratio"] for c in out[call].values())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(H.ROOT, "profiles", "mixture_bench.json"))
    ap.add_argument("--workload", help="one scene instead of cfg3_headline and rows_1e5: a name of synthetic.make_scene, or rows_1e5")
    ap.add_argument("--steps", type=int, default=5, help="timed calls of each of the two entry points per scene and grid")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rehearsal", action="store_true", help="G = 8 and 12 instead of 35 and 96, no parity section")
    ap.add_argument("--baseline-seconds", type=float, default=60.0, help="a baseline leg runs in full only if projected within this")
    ap.add_argument("--baseline-gib", type=float, default=48.0, help="... and if its largest tensor is within this")
    a = ap.parse_args()
    H.require_gpu("bench_mixture.py")
    grids = (8, 12) if a.rehearsal else (35, 96)
    names = [a.workload] if a.workload else ["cfg3_headline", "rows_1e5"]
    out = {"component": "the scene as a Gaussian mixture: log-density and closed-form Fourier transform on a G^3 grid (gs_mixture_log_density, "
                        "gs_mixture_fourier) beside the reference's slice-by-slice log_prob and its transform in batches of 500, one GPU (see device)",
           "method": "ours: device events around each call after the warm-up, median / p10 / p90 of the per-call milliseconds; reference legs: "
                     "host clock around one run ending in a synchronise, first projected from the first slice / batch and run in full only "
                     "within the limits given; pairs = rows taking part x queries; fraction_of_vector_peak = pairs/s x f32 operations per "
                     f"pair (fma = 2) / {PEAK_TFLOPS} TFLOP/s",
           "source_digest": _native.source_digest(), "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "points_per_workgroup": mixture.POINTS_PER_WORKGROUP, "components_per_chunk": mixture.COMPONENTS_PER_CHUNK,
           "baseline_limits": {"seconds": a.baseline_seconds, "largest_tensor_gib": a.baseline_gib},
           "scenes": {name: measure_scene(name, grids, a) for name in names}}
    if not a.rehearsal:
        out["parity"] = parity_ratios()
    H.write_json(out, a.out)


if __name__ == "__main__":
    main()
