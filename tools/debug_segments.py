"""One soak scene (tools/parity_soak.py, by seed) through the blend backward with unit grad factors, against the oracle:
tile-list lengths and heavy tiles of the frame, per gradient group the worst use of the per-element bar and the
tensor-level error, the six worst elements of the position gradient with the tiles that hold the worst point, and .npy
dumps of the position gradient and the view-space magnitude image (named by GS_BWD_SEGMENTS) for comparing two runs.

    [GS_BWD_SEGMENTS=0|1] python tools/debug_segments.py [seed] [dump_dir]        (GPU; dump_dir defaults to the current directory)
"""
import argparse
import os

import harness as H
import numpy as np

import parity_util as P
from oracle import oracle


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("seed", nargs="?", type=int, default=60163)
    ap.add_argument("dump_dir", nargs="?", default=".")
    a = ap.parse_args()
    H.require_gpu("debug_segments.py")
    c = P.soak_case(a.seed)
    s, q, t, partial = c["scene"], c["q"], c["t"], c["partial"]
    ocfg = oracle.default_config(allow_partial_tiles=int(partial), **P.UNIT_FACTORS)
    f, feat_after = P.run_oracle(s, q, t, ocfg)
    module = P.module(partial, hook=lambda x: None, **P.UNIT_FACTORS)
    inp = P.make_input(s, q, t, 3)
    image, g = H.seeded_backward(module, inp, c["rng"])
    fr = module.last_frame
    lens = f.tile_points_end - f.tile_points_start
    segments = os.environ.get("GS_BWD_SEGMENTS")
    print("W,H", c["W"], c["H"], "T", lens.size, "lens max", lens.max(), "heavy", fr.heavy_tiles(), "items", fr.heavy_tiles(items=True),
          "segments env", segments)
    b = oracle.backward(f, g.cpu().numpy(), 3, ocfg, want_summed=True)
    gp, gf = inp.point_cloud.grad.cpu().numpy(), inp.point_cloud_features.grad.cpu().numpy()
    m = P.backward_margins(gp, gf, b)
    row = {"xyz": (round(m["xyz"]["bar_use_max"], 2), "%.1e" % P.rel_err(gp, b["grad_pointcloud"]))}
    for lo, hi, name in P.GROUPS:
        row[name] = (round(m[name]["bar_use_max"], 2), "%.1e" % P.rel_err(gf[:, lo:hi], b["grad_pointcloud_features"][:, lo:hi]))
    print(row)
    mi = module.last_backward_extras["magnitude_grad_viewspace_on_image"].cpu().numpy()
    print("mag image rel err", P.rel_err(mi, b["magnitude_grad_viewspace_on_image"]))
    os.makedirs(a.dump_dir, exist_ok=True)
    np.save(os.path.join(a.dump_dir, f"dbg_gp_{segments or '1'}.npy"), gp)
    np.save(os.path.join(a.dump_dir, f"dbg_mag_{segments or '1'}.npy"), mi)
    np.save(os.path.join(a.dump_dir, "dbg_mag_ref.npy"), b["magnitude_grad_viewspace_on_image"])
    # the worst elements against the per-element bar: which point, which tiles hold it and how long their lists are
    err = np.abs(gp - b["grad_pointcloud"])
    summed = b["summed_pointcloud"]
    use = err / np.maximum(summed, 1e-30)
    flat = np.argsort(use.ravel())[::-1][:6]
    ids = np.asarray(f.point_id_in_camera_list)
    cam_of = {int(p): i for i, p in enumerate(ids)}
    for fl in flat:
        p, comp = divmod(int(fl), 3)
        print("point", p, "component", comp, "got %.6e ref %.6e err %.2e summed %.3e err/summed %.2e"
              % (gp[p, comp], b["grad_pointcloud"][p, comp], err[p, comp], summed[p, comp], use[p, comp]),
              "tiles covered", int(np.asarray(f.num_overlap_tiles)[cam_of[p]]) if p in cam_of else None)
    m_idx = cam_of.get(int(flat[0]) // 3)
    if m_idx is not None:            # tiles holding the worst point: from the sorted values
        pos = np.nonzero(np.asarray(f.point_offset_with_sort_key) == m_idx)[0]
        ts, te = np.asarray(f.tile_points_start), np.asarray(f.tile_points_end)
        for ps in pos[:12]:
            tl = int(np.nonzero((ts <= ps) & (te > ps))[0][0])
            print("   in tile", tl, "list", int(ts[tl]), int(te[tl]), "len", int(te[tl] - ts[tl]), "position in list", int(ps - ts[tl]))


if __name__ == "__main__":
    main()
