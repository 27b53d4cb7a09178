#!/usr/bin/env python3
"""Measure vector quantisation (include/gs_vq.h, vq.py) and compressed scene files (compression.py), on cuda:0:
  sizes      at every --rows x --codes: gs_vq_assign, gs_vq_update and one k-means iteration (both) on the 45 higher-band SH
             coefficients of a synthetic scene, beside the same iteration in torch operations on the same device: torch.cdist +
             argmin over chunks of rows (the N x K distance matrix does not fit in one piece; the chunk is stated, and a leg whose
             chunk's matrix would pass 2^31 elements is "not run"), then index_add_ and a division.  The assignment's FLOP rate
             is 2 N K Dp over its median time, against the 157.3 TFLOP/s f32 peak of the chip.
  compress   compression.compress() end to end at every --rows (the largest --codes, 10 iterations), the time to write the
             file, and its size beside the parquet of the same scene.
The synthetic scenes' SH coefficients are independent draws: incompressible by construction.  They serve for timing, which does
not depend on the data; the sizes of the files do not depend on it either (36 bytes per Gaussian before deflate), the picture
quality after compression does and is not measured here.
Each comparison alternates its legs in one process (harness.alternate: every leg warmed, then `repeats` rounds of one timed
window per leg, a window being `--steps` calls between two device events).  No ratio is asserted.

    python tools/bench_vq.py [--out profiles/vq_bench.json] [--rows 500000,2000000] [--codes 256,4096] [--steps N] [--warmup N]
                             [--repeats N] [--skip-compress]
"""
import argparse
import os
import tempfile
import time

import harness as H
import torch

from taichi_3d_gaussian_splatting_amd import compression, scene_io, vq
from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, synth

DEV = "cuda:0"
ROWS, CODES = "500000,2000000", "256,4096"
WORKLOADS = {500_000: "cfg3_headline", 2_000_000: "cfg5_infer2e6"}
PEAK_TFLOPS_F32 = 157.3
CHUNK_ELEMENTS = 2 ** 28                                            # of a chunk's distance matrix: 1 GiB of float32
KEYS = ("component", "method", "data", "peak_tflops_f32", "sizes", "compress", "notes")


def scene_of(n):
    return make_scene(WORKLOADS[n]) if n in WORKLOADS else synth(n, 256, 160, 0.05)


def torch_assign(x, codebook, labels, chunk):
    for lo in range(0, x.shape[0], chunk):
        labels[lo:lo + chunk] = torch.cdist(x[lo:lo + chunk], codebook).argmin(1)


def torch_update(x, labels, codebook):
    sums = torch.zeros_like(codebook).index_add_(0, labels, x)
    counts = torch.bincount(labels, minlength=codebook.shape[0])
    codebook.copy_(torch.where(counts[:, None] > 0, sums / counts.clamp_min(1)[:, None], codebook))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--rows", default=ROWS, help="rows of the scenes, comma separated")
    ap.add_argument("--codes", default=CODES, help="codebook sizes, comma separated")
    ap.add_argument("--steps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=2, help="untimed calls of every leg")
    ap.add_argument("--repeats", type=int, default=5, help="alternating rounds")
    ap.add_argument("--skip-compress", action="store_true")
    a = ap.parse_args()
    H.require_gpu("bench_vq.py")
    rows, codes = [int(v) for v in a.rows.split(",")], [int(v) for v in a.codes.split(",")]
    out = {"component": "vector quantisation: assignment (matrix cores), update and k-means iteration; compressed scene files, 1x MI355X",
           "method": f"harness.alternate: {a.warmup} warm calls per leg, {a.repeats} rounds of one {a.steps}-call window per leg between device events",
           "data": "the 45 higher-band SH coefficients of synthetic scenes (independent draws: timing only)",
           "peak_tflops_f32": PEAK_TFLOPS_F32, "sizes": {}, "compress": {}, "notes": []}
    for n in rows:
        s = scene_of(n)
        x = torch.tensor(s.point_cloud_features[:, list(compression.REST_COLUMNS)], device=DEV)
        xp = vq.padded(x)[0][:, :45]                                # rows of 48 floats, made once: the calls take it as it is
        out["sizes"][str(n)] = {}
        for k in codes:
            start = xp[vq.initial_rows(n, k).to(DEV)]
            k = start.shape[0]
            codebook = torch.zeros(k, 48, device=DEV)[:, :45]
            codebook.copy_(start)
            labels, _ = vq.assign(xp, codebook)
            labels64 = labels.long()
            torch_labels = torch.empty(n, dtype=torch.int64, device=DEV)
            torch_codebook = start.clone()
            chunk = max(min(CHUNK_ELEMENTS // k, n), 1)
            rec = {"rows": n, "codes": k, "dim": 45, "torch_chunk_rows": chunk}
            legs = {"assign": {"hip": lambda: vq.assign(xp, codebook)}, "update": {"hip": lambda: vq.update(xp, labels, codebook)},
                    "iteration": {"hip": lambda: vq.update(xp, vq.assign(xp, codebook)[0], codebook)}}
            if chunk * k < 2 ** 31:
                legs["assign"]["torch"] = lambda: torch_assign(x, torch_codebook, torch_labels, chunk)
                legs["update"]["torch"] = lambda: torch_update(x, labels64, torch_codebook)
                legs["iteration"]["torch"] = lambda: (torch_assign(x, torch_codebook, torch_labels, chunk),
                                                      torch_update(x, torch_labels, torch_codebook))
            for name, variants in legs.items():
                rec[name] = H.alternate(variants, a.steps, a.warmup, a.repeats)
                if "torch" in variants:
                    rec[name]["torch_over_hip"] = round(rec[name]["torch"]["median_ms"] / rec[name]["hip"]["median_ms"], 3)
                else:
                    rec[name]["torch"], rec[name]["torch_over_hip"] = "not run", "not run"
            flop = 2.0 * n * k * 48
            rec["assign_tflops"] = round(flop / (rec["assign"]["hip"]["median_ms"] * 1e-3) / 1e12, 3)
            rec["assign_share_of_f32_peak"] = round(rec["assign_tflops"] / PEAK_TFLOPS_F32, 4)
            out["sizes"][str(n)][str(k)] = rec
            del codebook, torch_codebook, torch_labels, labels, labels64
            torch.cuda.empty_cache()
        if not a.skip_compress:
            scene = torch.tensor(s.point_cloud, device=DEV), torch.tensor(s.point_cloud_features, device=DEV)
            from types import SimpleNamespace
            holder = SimpleNamespace(point_cloud=scene[0], point_cloud_features=scene[1])
            compression.compress(holder, codes=min(max(codes), n), iters=1)             # warm
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            compressed = compression.compress(holder, codes=max(codes), iters=10)
            t1 = time.perf_counter()
            with tempfile.TemporaryDirectory() as tmp:
                npz, parquet = os.path.join(tmp, "scene.npz"), os.path.join(tmp, "scene.parquet")
                compressed.save(npz)
                t2 = time.perf_counter()
                scene_io.save_parquet(parquet, s.point_cloud, s.point_cloud_features)
                sizes = os.path.getsize(npz), os.path.getsize(parquet)
            out["compress"][str(n)] = {"rows": n, "codes": int(compressed.codebook.shape[0]), "iters": 10,
                                       "compress_ms": round((t1 - t0) * 1e3, 3), "save_ms": round((t2 - t1) * 1e3, 3),
                                       "npz_bytes": sizes[0], "bytes_before_deflate": compressed.nbytes(), "parquet_bytes": sizes[1],
                                       "parquet_over_npz": round(sizes[1] / sizes[0], 3)}
            del scene, holder, compressed
        del x, xp
        torch.cuda.empty_cache()
    if a.skip_compress:
        out["compress"] = "not measured"

    def legs_of(doc, path=()):
        if isinstance(doc, dict) and "windows_ms" in doc:
            yield "/".join(path), doc
        elif isinstance(doc, dict):
            for key, v in doc.items():
                yield from legs_of(v, path + (key,))
    for name, leg in legs_of(out):
        if leg["max_ms"] > 1.5 * leg["min_ms"]:
            out["notes"].append(f"{name}: its windows span {leg['min_ms']} to {leg['max_ms']} ms ({leg['windows_ms']}): more than one "
                                "regime in one leg, so its median and the ratios made from it are not a steady-state figure")
    assert set(out) == set(KEYS)
    H.write_json(out, a.out)


if __name__ == "__main__":
    main()
