"""trainer_util's 64x96 dataset with depth files, for tests/test_gpu_trainer_depth.py and tools/bench_depth_loss.py: depth and
accumulated alpha of the ground-truth scene rendered per view, the depth zeroed where alpha < 0.5 (no surface: a hole), written
as 16-bit PNGs with a depth_scale under which the largest depth fits; and the two seeded short runs whose depth error is
compared."""
import json
import os

import numpy as np
import torch

import trainer_util as TU

ALPHA_MIN = 0.5
# The depth term's weight in the 120-iteration runs: constant.  The default schedule anneals it to a hundredth over the run --
# meant for tens of thousands of iterations -- which here leaves the last third of the run to the colour term alone.
SHORT_RUN = dict(weight_init=1.0, weight_final=1.0)
U16_TOP = 65000                 # the largest depth of the dataset maps to this value


def ground_truth_depth(device):
    """-> {view: float32 (H,W) depth of the ground-truth scene, 0 where the accumulated alpha is below ALPHA_MIN}"""
    from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast
    from taichi_3d_gaussian_splatting_amd.synthetic import scene_input, view_pose
    scene = TU.ground_truth_scene()
    module = Rast(Rast.GaussianPointCloudRasterisationConfig())
    n_views = len(TU.TRAIN_VIEWS) + len(TU.VAL_VIEWS)
    out = {}
    with torch.no_grad():
        for view in range(n_views):
            q, t = view_pose(view, n_views)
            _, depth, _, alpha = module(scene_input(scene, q, t, device, band=3), return_accumulated_alpha=True)
            out[view] = torch.where(alpha >= ALPHA_MIN, depth, torch.zeros_like(depth)).cpu().numpy().astype(np.float32)
    return out


def add_depth(base, root, device, transform=None, name="depth"):
    """base: what trainer_util.write_dataset returned.  Writes root/<name>/view_<v>.png (uint16) for every view and the JSONs
    root/train_<name>.json, root/val_<name>.json with depth_path and depth_scale columns.  transform(view, z) -> the values to
    store for the valid samples (default: the depth itself); holes stay 0.
    -> dict(paths, images, depth={view: the float32 ground-truth depth, holes 0}, depth_scale, stored={view: uint16 array})"""
    import PIL.Image
    root = str(root)
    os.makedirs(os.path.join(root, name), exist_ok=True)
    depth = ground_truth_depth(device)
    values = {}
    for view, z in depth.items():
        v = z.astype(np.float64) if transform is None else np.asarray(transform(view, z.astype(np.float64)), np.float64)
        values[view] = np.where(z > 0, v, 0.0)
    top = max(float(v.max()) for v in values.values())
    assert top > 0
    depth_scale = top / U16_TOP
    stored, files = {}, {}
    for view, v in values.items():
        u16 = np.round(v / depth_scale).astype(np.uint16)
        u16[(depth[view] > 0) & (u16 == 0)] = 1             # a valid sample stays valid
        files[view] = os.path.join(root, name, f"view_{view}.png")
        PIL.Image.fromarray(u16).save(files[view])
        stored[view] = u16
    paths = dict(base["paths"])
    for split, views in (("train", TU.TRAIN_VIEWS), ("val", TU.VAL_VIEWS)):
        records = json.load(open(base["paths"][split]))
        assert len(records) == len(views)
        for r, view in zip(records, views):
            r["depth_path"], r["depth_scale"] = files[view], depth_scale
        paths[split] = os.path.join(root, f"{split}_{name}.json")
        with open(paths[split], "w") as fh:
            json.dump(records, fh)
    return dict(paths=paths, images=base["images"], depth=depth, depth_scale=depth_scale, stored=stored)


def validation_depth_error(trainer, data):
    """the mean over the validation views of the mean |D - Z| over the pixels with a ground-truth depth, D rendered from the
    trainer's scene at full resolution"""
    errors = []
    with torch.no_grad():
        for i, view in enumerate(TU.VAL_VIEWS):
            _, q, t, info = trainer.val_targets.target(i, 1)[:4]
            _, rendered, _ = trainer.rasterisation(trainer._rasterisation_input(info, q, t, color_max_sh_band=3))
            z = torch.from_numpy(data["depth"][view]).to(rendered.device)
            valid = z > 0
            errors.append(float((rendered - z).abs()[valid].mean().item()))
    return float(np.mean(errors))


def supervised_and_plain_runs(data, out_dir, device="cuda:0", depth_config=None):
    """The same seeded short run (trainer_util.SMOKE, from the perturbed scene the dataset's cloud holds) with depth="metric"
    and without.  -> {"metric" | "none": dict(depth_error, psnr, means, trainer)}.  depth_config None: SHORT_RUN."""
    from taichi_3d_gaussian_splatting_amd.depth import DepthConfig
    depth_config = depth_config or DepthConfig(**SHORT_RUN)
    from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer, JsonlSummaryWriter
    out = {}
    for name in ("none", "metric"):
        config = TU.train_config(data["paths"], os.path.join(str(out_dir), name), seed=0, log_loss_interval=10, **TU.SMOKE)
        config.loss_function_config.enable_regularization = False
        kwargs = dict(depth="metric", depth_config=depth_config) if name == "metric" else {}
        trainer = GaussianPointCloudTrainer(config, device=device, writer=JsonlSummaryWriter(config.summary_writer_log_dir), **kwargs)
        trainer.train()
        iteration, means = trainer.last_validation
        assert iteration == TU.SMOKE["val_interval"]
        out[name] = dict(depth_error=validation_depth_error(trainer, data), psnr=float(means["psnr"]), means=means, trainer=trainer)
    return out
