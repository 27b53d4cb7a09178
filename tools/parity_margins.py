"""Per-element parity margins of the two returned gradients (GPU): for BASELINE configs 2 and 3 (and any soak seeds
given), the worst and 99.9th-percentile per-element errors of the HIP operator against the CPU oracle under the bar of
tests/parity_util.py (|a - ref| <= 1e-4 |ref| + 1e-5 S, S = magnitude summed to produce the element), the error relative
to |ref| over well-conditioned elements, and the tensor-level figure (max |a - ref| / max |ref|: the margin to the 1e-4
bar); under `extras`, the tensor-level figures of the three view-space products of the backward and whether the
affected-pixel counts are equal.  The upstream gradient is 2 (image - target), target ~ U[0,1) seeded with 0.  Writes JSON
to the path given (default parity_margins.json in the current directory); the judged copy lives under profiles/.

    python tools/parity_margins.py [out.json] [--workload NAME ...]
"""
import argparse
import json
import os

import harness as H
import numpy as np

import parity_util as P
from oracle import oracle
from taichi_3d_gaussian_splatting_amd.synthetic import make_scene, view_pose


def run(name, scene, q, t, band=3, partial=False):
    module = P.module(partial, hook=lambda x: None)
    inp = P.make_input(scene, q, t, band)
    ocfg = oracle.default_config(allow_partial_tiles=int(partial))
    f, feat_after = P.run_oracle(scene, q, t, ocfg)
    image, g = H.seeded_backward(module, inp)
    b = oracle.backward(f, g.cpu().numpy(), band, ocfg, want_summed=True)
    gp, gf = inp.point_cloud.grad.cpu().numpy(), inp.point_cloud_features.grad.cpu().numpy()
    m = P.backward_margins(gp, gf, b)
    m["xyz"]["tensor_level"] = P.rel_err(gp, b["grad_pointcloud"])
    for lo, hi, gname in P.GROUPS:
        m[gname]["tensor_level"] = P.rel_err(gf[:, lo:hi], b["grad_pointcloud_features"][:, lo:hi])
    img_ref = f.rasterized_image
    img = image.detach().cpu().numpy()
    nz = img_ref > 1e-3
    m["image"] = {"tensor_level": P.rel_err(img, img_ref),
                  "rel_max_where_ref_gt_1e-3": float((np.abs(img - img_ref)[nz] / img_ref[nz]).max())}
    ex = module.last_backward_extras
    extras = {key: P.rel_err(ex[key].cpu().numpy(), b[key])
              for key in ("grad_viewspace", "magnitude_grad_viewspace", "magnitude_grad_viewspace_on_image")}
    extras["n_affected_equal"] = bool(np.array_equal(ex["num_affected_pixels"].cpu().numpy(), b["num_affected_pixels"]))
    return {"workload": name, "N": int(f.N), "M": int(f.M), "K": int(f.K), "groups": m, "extras": extras}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default="parity_margins.json")
    ap.add_argument("--workload", action="append", help="default: cfg2_truck7k and cfg3_headline")
    a = ap.parse_args()
    H.require_gpu("parity_margins.py")
    res = {"bar": f"|a - ref| <= {P.ELEM_RTOL} |ref| + {P.ELEM_FLOOR} S  (tests/parity_util.py); bar_use = error / bar",
           "cases": []}
    q, t = view_pose()
    for name in a.workload or ("cfg2_truck7k", "cfg3_headline"):
        res["cases"].append(run(name, make_scene(name), q, t))
        print(json.dumps(res["cases"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
