"""trainer_util's 64x96 dataset with normal priors, for tests/test_gpu_trainer_geometry.py and tools/bench_geometry.py: the
normals of the ground-truth scene's depth (depth_trainer_util.ground_truth_depth) by the float64 restatement
tests/geometry_ref.py, written as 8-bit PNGs (n + 1) / 2 with (0,0,0) where there is none; the mean angle between the normals of
a trainer's validation renders and those; and the two seeded short runs whose angles are compared."""
import json
import os

import numpy as np
import torch

import depth_trainer_util as DU
import geometry_ref as R
import trainer_util as TU

MAX_REL_JUMP = 0.1              # of the ground-truth normals: none across a depth edge of the scene
# The weights of the 120-iteration runs.  At iteration 0 of these runs (measured on an MI355X) the colour loss is 0.018, the normal
# loss 0.049 and the inverse-depth smoothness 0.028: with these weights the two terms together weigh about as much as the colour
# term.
SHORT_RUN = dict(smooth_weight=0.5, normal_weight=0.1)


def intrinsics():
    """(fx, fy, cx, cy) of the dataset's camera"""
    k = np.asarray(TU.ground_truth_scene().camera_intrinsics, dtype=np.float64)
    return float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])


def encode(normals):
    """(3,H,W) float64 unit normals, 0 where none -> (H,W,3) uint8 (n + 1) / 2, (0,0,0) where none"""
    has = (normals != 0).any(axis=0)
    coded = np.clip(np.round((normals + 1.0) * 127.5), 0, 255).astype(np.uint8)
    return np.where(has[None], coded, 0).transpose(1, 2, 0).copy()


def add_normals(base, root, device, name="normal"):
    """base: what trainer_util.write_dataset returned.  Writes root/<name>/view_<v>.png for every view and the JSONs
    root/train_<name>.json, root/val_<name>.json with a normal_path column.
    -> dict(paths, images, normals={view: float64 (3,H,W), 0 where none}, stored={view: uint8 (H,W,3)})"""
    import PIL.Image
    root = str(root)
    os.makedirs(os.path.join(root, name), exist_ok=True)
    K = intrinsics()
    normals, stored, files = {}, {}, {}
    for view, z in DU.ground_truth_depth(device).items():
        normals[view] = R.depth_normals(z, K, MAX_REL_JUMP)[0]
        stored[view] = encode(normals[view])
        files[view] = os.path.join(root, name, f"view_{view}.png")
        PIL.Image.fromarray(stored[view]).save(files[view])
    paths = dict(base["paths"])
    for split, views in (("train", TU.TRAIN_VIEWS), ("val", TU.VAL_VIEWS)):
        records = json.load(open(base["paths"][split]))
        assert len(records) == len(views)
        for r, view in zip(records, views):
            r["normal_path"] = files[view]
        paths[split] = os.path.join(root, f"{split}_{name}.json")
        with open(paths[split], "w") as fh:
            json.dump(records, fh)
    return dict(paths=paths, images=base["images"], normals=normals, stored=stored)


def validation_normal_angle(trainer, data):
    """the mean over the validation views of the mean angle, in degrees, between geometry.depth_normals of the depth rendered
    from the trainer's scene at full resolution and the ground-truth normals, over the pixels where both exist"""
    from taichi_3d_gaussian_splatting_amd import geometry
    angles = []
    with torch.no_grad():
        for i, view in enumerate(TU.VAL_VIEWS):
            _, q, t, info = trainer.val_targets.target(i, 1)[:4]
            _, rendered, _ = trainer.rasterisation(trainer._rasterisation_input(info, q, t, color_max_sh_band=3))
            n = geometry.depth_normals(rendered, info.camera_intrinsics, MAX_REL_JUMP).double().cpu().numpy()
            truth = data["normals"][view]
            both = (n != 0).any(axis=0) & (truth != 0).any(axis=0)
            assert both.sum() > 100
            cos = np.clip((n * truth).sum(axis=0)[both], -1.0, 1.0)
            angles.append(float(np.degrees(np.arccos(cos)).mean()))
    return float(np.mean(angles))


def regularised_and_plain_runs(data, out_dir, device="cuda:0", geometry_config=None):
    """The same seeded short run (trainer_util.SMOKE, from the perturbed scene the dataset's cloud holds) with the geometry terms
    and without.  -> {"geometry" | "none": dict(angle, psnr, means, trainer)}.  geometry_config None: SHORT_RUN."""
    from taichi_3d_gaussian_splatting_amd.geometry import GeometryConfig
    from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer, JsonlSummaryWriter
    geometry_config = geometry_config or GeometryConfig(**SHORT_RUN)
    out = {}
    for name in ("none", "geometry"):
        config = TU.train_config(data["paths"], os.path.join(str(out_dir), name), seed=0, log_loss_interval=10, **TU.SMOKE)
        config.loss_function_config.enable_regularization = False
        kwargs = dict(geometry=geometry_config) if name == "geometry" else {}
        trainer = GaussianPointCloudTrainer(config, device=device, writer=JsonlSummaryWriter(config.summary_writer_log_dir), **kwargs)
        trainer.train()
        iteration, means = trainer.last_validation
        assert iteration == TU.SMOKE["val_interval"]
        out[name] = dict(angle=validation_normal_angle(trainer, data), psnr=float(means["psnr"]), means=means, trainer=trainer)
    return out
