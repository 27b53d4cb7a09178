#!/usr/bin/env python3
"""The trainer's smoke run of tests/test_gpu_trainer.py (tests/trainer_util.smoke_run: a 400-point synthetic scene, 6 + 2 views
of 64x96, positions and SH DC perturbed, 120 iterations) -> the validation means before and after, as one JSON.

    python tools/trainer_smoke.py [--out profiles/trainer_smoke.json]
"""
import argparse
import tempfile
import time

import harness as H

import trainer_util


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    H.require_gpu("trainer_smoke.py")
    with tempfile.TemporaryDirectory(prefix="trainer_smoke_") as root:
        t0 = time.perf_counter()
        trainer, before, after = trainer_util.smoke_run(root)
        seconds = time.perf_counter() - t0
    H.write_json({"component": "GaussianPointCloudTrainer smoke run, 1x MI355X", "settings": trainer_util.SMOKE,
                  "points": trainer_util.N_POINTS, "image": [trainer_util.H, trainer_util.W],
                  "views": {"train": len(trainer_util.TRAIN_VIEWS), "val": len(trainer_util.VAL_VIEWS)},
                  "validation_before": before, "validation_after": after,
                  "psnr_gain_db": after["psnr"] - before["psnr"], "wall_seconds_with_setup": round(seconds, 2)}, a.out)


if __name__ == "__main__":
    main()
