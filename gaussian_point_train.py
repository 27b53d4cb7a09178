"""Train a scene from images: python gaussian_point_train.py --train_config PATH (the reference's script and YAML format).
--pixel_weights alpha|file [--mask_erode K] trains with per-pixel weights (INTEGRATION.md "Masked and weighted training");
--density mcmc [--mcmc_cap N] trains with a fixed budget of Gaussians (INTEGRATION.md "Fixed-budget densification");
--appearance affine trains a colour transform per training image with the scene (INTEGRATION.md "Exposure compensation");
--bilateral_grid [--bilateral_shape X Y L --bilateral_tv W --bilateral_lr LR] trains a bilateral grid of colour transforms per
training image instead (INTEGRATION.md "Bilateral grids");
--depth metric|relative [--depth_weight W --depth_space depth|inverse --depth_norm l1|l2] adds a depth term from the dataset's
depth_path maps (INTEGRATION.md "Depth supervision in the trainer");
--depth_smooth W [--smooth_order 1|2 --smooth_space depth|inverse --smooth_edge_lambda L] adds an edge-aware smoothness of the
rendered depth, and --normal_prior W [--normal_convention opencv|opengl] a normal loss against the dataset's normal_path priors
(INTEGRATION.md "Geometry regularisers");
--normal_consistency W [--consistency_min_length L --consistency_start N] adds the consistency of the rendered Gaussian normals
with the normal of the rendered depth, which needs no data (INTEGRATION.md "Normal consistency");
--background colour|random|sky [--background_colour R G B --background_bands B --background_lr LR --composite_targets] puts a
solid colour, a random colour per step or a learnable spherical-harmonics sky behind the splats, and composites RGBA pictures
over the same background (INTEGRATION.md "Backgrounds");
--filter3d [--filter3d_variance V --filter3d_interval N] trains under the 3D smoothing filter of Mip-Splatting and writes
filter3d_<iteration>.pt beside every scene file (INTEGRATION.md "3D smoothing filter");
--pose_refinement [--pose_lr LR --pose_lr_final LR --pose_reg W --pose_start N --val_pose_steps N] trains a pose correction per
training image with the scene and writes poses_<iteration>.pt beside every scene file (INTEGRATION.md "Pose refinement")."""
import argparse

from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer

if __name__ == "__main__":
    parser = argparse.ArgumentParser("Train a Gaussian Point Cloud Scene")
    parser.add_argument("--train_config", type=str, required=True)
    parser.add_argument("--gen_template_only", action="store_true", default=False)
    parser.add_argument("--pixel_weights", choices=("none", "alpha", "file"), default="none",
                        help="the loss's per-pixel weights: the RGBA images' alpha, or the dataset's mask_path images")
    parser.add_argument("--mask_erode", type=int, default=0, help="shrink the mask by this many pixels at load")
    parser.add_argument("--density", choices=("adaptive", "mcmc"), default="adaptive",
                        help="how the scene grows: the adaptive controller's clone / split, or relocation under a fixed budget")
    parser.add_argument("--mcmc_cap", type=int, default=None, help="with --density mcmc: the number of Gaussians to reach and keep "
                        "(default: every row the scene allocates, max_num_points_ratio)")
    parser.add_argument("--appearance", choices=("none", "affine"), default="none",
                        help="exposure compensation: a learnable 3x4 affine colour transform per training image")
    parser.add_argument("--bilateral_grid", action="store_true", default=False,
                        help="a learnable bilateral grid of 3x4 colour transforms per training image: spatially varying colour correction")
    parser.add_argument("--bilateral_shape", type=int, nargs=3, default=None, metavar=("X", "Y", "L"),
                        help="with --bilateral_grid: vertices across, down and along the luminance (default 16 16 8)")
    parser.add_argument("--bilateral_tv", type=float, default=None, metavar="W", help="with --bilateral_grid: weight of the grid's total variation")
    parser.add_argument("--bilateral_lr", type=float, default=None, metavar="LR", help="with --bilateral_grid: the grids' learning rate at "
                        "iteration 0 (it falls to a hundredth of it over the run)")
    parser.add_argument("--depth", choices=("none", "metric", "relative"), default="none",
                        help="depth supervision from the dataset's depth_path maps: metres, or a monocular network's relative "
                        "inverse depth aligned per view by scale and shift")
    parser.add_argument("--depth_weight", type=float, default=None, help="with --depth: the term's weight at iteration 0 (it falls to "
                        "a hundredth of it over the run)")
    parser.add_argument("--depth_space", choices=("depth", "inverse"), default=None, help="with --depth: the space of the residual")
    parser.add_argument("--depth_norm", choices=("l1", "l2"), default=None, help="with --depth: the norm of the residual")
    parser.add_argument("--depth_smooth", type=float, default=None, metavar="W", help="weight of the edge-aware smoothness of the rendered depth")
    parser.add_argument("--smooth_order", type=int, choices=(1, 2), default=None, help="with --depth_smooth: first or second differences")
    parser.add_argument("--smooth_space", choices=("depth", "inverse"), default=None, help="with --depth_smooth: the space of the differences")
    parser.add_argument("--smooth_edge_lambda", type=float, default=None, help="with --depth_smooth: how fast an edge of the picture relaxes it")
    parser.add_argument("--normal_prior", type=float, default=None, metavar="W", help="weight of the normal loss against the dataset's "
                        "normal_path priors")
    parser.add_argument("--normal_convention", choices=("opencv", "opengl"), default=None, help="with --normal_prior: the priors' camera frame")
    parser.add_argument("--normal_consistency", type=float, default=None, metavar="W", help="weight of the consistency between the rendered "
                        "Gaussian normals and the normal of the rendered depth (needs no data)")
    parser.add_argument("--consistency_min_length", type=float, default=None, help="with --normal_consistency: a pixel whose blended normal "
                        "is shorter than this is left out")
    parser.add_argument("--consistency_start", type=int, default=None, metavar="N", help="with --normal_consistency: the first iteration of the "
                        "geometry terms (GeometryConfig.start_iteration)")
    parser.add_argument("--background", choices=("none", "colour", "random", "sky"), default="none",
                        help="what lies behind the splats: a solid colour, a random colour per step, or a learnable sky")
    parser.add_argument("--background_colour", type=float, nargs=3, default=None, metavar=("R", "G", "B"),
                        help="with --background: the colour, the validation colour of random, the sky's start (default 0 0 0)")
    parser.add_argument("--background_bands", type=int, choices=(0, 1, 2, 3), default=None, help="with --background sky: its spherical-harmonics bands")
    parser.add_argument("--background_lr", type=float, default=None, metavar="LR", help="with --background sky: its learning rate at "
                        "iteration 0 (it falls to a tenth of it over the run)")
    parser.add_argument("--composite_targets", action="store_true", default=False,
                        help="with --background: composite the RGBA pictures over the step's background")
    parser.add_argument("--filter3d", action="store_true", default=False, help="train under the 3D smoothing filter of Mip-Splatting")
    parser.add_argument("--filter3d_variance", type=float, default=None, metavar="V", help="with --filter3d: the filter's variance in "
                        "square pixels (default 0.2)")
    parser.add_argument("--filter3d_interval", type=int, default=None, metavar="N", help="with --filter3d: iterations between two "
                        "refreshes of the sampling rates (default 100)")
    parser.add_argument("--pose_refinement", action="store_true", default=False, help="train a camera pose correction per training image")
    parser.add_argument("--pose_lr", type=float, default=None, metavar="LR", help="with --pose_refinement: the corrections' learning rate "
                        "at its first iteration (default 1e-3)")
    parser.add_argument("--pose_lr_final", type=float, default=None, metavar="LR", help="with --pose_refinement: their learning rate at the "
                        "last iteration (default 1e-4)")
    parser.add_argument("--pose_reg", type=float, default=None, metavar="W", help="with --pose_refinement: weight of the L2 pull to the "
                        "dataset's pose (default 1e-6)")
    parser.add_argument("--pose_start", type=int, default=None, metavar="N", help="with --pose_refinement: the first refined iteration")
    parser.add_argument("--val_pose_steps", type=int, default=0, metavar="N", help="align every validation view against the frozen scene "
                        "by N pose steps and log val/psnr_aligned, val/ssim_aligned and val/loss_aligned as well")
    args = parser.parse_args()
    if not args.pose_refinement and any(v is not None for v in (args.pose_lr, args.pose_lr_final, args.pose_reg, args.pose_start)):
        parser.error("--pose_lr, --pose_lr_final, --pose_reg and --pose_start need --pose_refinement")
    if not args.filter3d and (args.filter3d_variance is not None or args.filter3d_interval is not None):
        parser.error("--filter3d_variance and --filter3d_interval need --filter3d")
    if args.background == "none" and (args.background_colour is not None or args.background_bands is not None or
                                      args.background_lr is not None or args.composite_targets):
        parser.error("--background_colour, --background_bands, --background_lr and --composite_targets need --background")
    if args.normal_consistency is None and (args.consistency_min_length is not None or args.consistency_start is not None):
        parser.error("--consistency_min_length and --consistency_start need --normal_consistency")
    if args.depth_smooth is None and (args.smooth_order is not None or args.smooth_space is not None or args.smooth_edge_lambda is not None):
        parser.error("--smooth_order, --smooth_space and --smooth_edge_lambda need --depth_smooth")
    if args.normal_prior is None and args.normal_convention is not None:
        parser.error("--normal_convention needs --normal_prior")
    if args.depth == "none" and (args.depth_weight is not None or args.depth_space is not None or args.depth_norm is not None):
        parser.error("--depth_weight, --depth_space and --depth_norm need --depth metric or relative")
    if not args.bilateral_grid and (args.bilateral_shape is not None or args.bilateral_tv is not None or args.bilateral_lr is not None):
        parser.error("--bilateral_shape, --bilateral_tv and --bilateral_lr need --bilateral_grid")
    if args.bilateral_grid and args.appearance == "affine":
        parser.error("--bilateral_grid and --appearance affine are alternatives: a grid contains the affine transform")
    if args.mcmc_cap is not None and args.density != "mcmc":
        parser.error("--mcmc_cap needs --density mcmc")
    if args.gen_template_only:
        import dataclasses

        import yaml
        with open(args.train_config, "w") as fh:
            yaml.safe_dump(dataclasses.asdict(GaussianPointCloudTrainer.TrainConfig()), fh)
        raise SystemExit(0)
    config = GaussianPointCloudTrainer.TrainConfig.from_yaml_file(args.train_config)
    if config.unknown_keys:
        print("ignored keys of the config:", ", ".join(config.unknown_keys))
    mcmc_config = None
    if args.density == "mcmc":
        from taichi_3d_gaussian_splatting_amd.mcmc import MCMCConfig
        mcmc_config = MCMCConfig(cap_max=args.mcmc_cap, seed=int(config.seed))
    depth_config = None
    if args.depth != "none":
        from taichi_3d_gaussian_splatting_amd.depth import DepthConfig
        depth_config = DepthConfig()
        if args.depth_weight is not None:
            depth_config.weight_init, depth_config.weight_final = args.depth_weight, args.depth_weight / 100.0
        if args.depth_space is not None:
            depth_config.space = args.depth_space
        if args.depth_norm is not None:
            depth_config.norm = args.depth_norm
    bilateral_config = None
    if args.bilateral_grid:
        from taichi_3d_gaussian_splatting_amd.bilateral import BilateralGridConfig
        bilateral_config = BilateralGridConfig()
        if args.bilateral_shape is not None:
            bilateral_config.grid_x, bilateral_config.grid_y, bilateral_config.grid_l = args.bilateral_shape
        if args.bilateral_tv is not None:
            bilateral_config.tv_weight = args.bilateral_tv
        if args.bilateral_lr is not None:
            bilateral_config.lr, bilateral_config.lr_final = args.bilateral_lr, args.bilateral_lr / 100.0
    geometry_config = None
    if args.depth_smooth is not None or args.normal_prior is not None or args.normal_consistency is not None:
        from taichi_3d_gaussian_splatting_amd.geometry import GeometryConfig
        chosen = dict(smooth_weight=args.depth_smooth, smooth_order=args.smooth_order, smooth_space=args.smooth_space,
                      smooth_edge_lambda=args.smooth_edge_lambda, normal_weight=args.normal_prior, normal_convention=args.normal_convention,
                      consistency_weight=args.normal_consistency, consistency_min_length=args.consistency_min_length,
                      start_iteration=args.consistency_start)
        geometry_config = GeometryConfig(**{name: value for name, value in chosen.items() if value is not None})
    background_config = None
    if args.background != "none":
        from taichi_3d_gaussian_splatting_amd.background import BackgroundConfig
        background_config = BackgroundConfig()
        if args.background_colour is not None:
            background_config.colour = tuple(args.background_colour)
        if args.background_bands is not None:
            background_config.bands = args.background_bands
        if args.background_lr is not None:
            background_config.lr, background_config.lr_final = args.background_lr, args.background_lr / 10.0
    filter3d_config = None
    if args.filter3d:
        from taichi_3d_gaussian_splatting_amd.filter3d import Filter3DConfig
        chosen = dict(variance=args.filter3d_variance, interval=args.filter3d_interval)
        filter3d_config = Filter3DConfig(**{name: value for name, value in chosen.items() if value is not None})
    pose_config = None
    if args.pose_refinement:
        from taichi_3d_gaussian_splatting_amd.pose_table import PoseRefinementConfig
        chosen = dict(lr=args.pose_lr, lr_final=args.pose_lr_final, reg=args.pose_reg, start_iteration=args.pose_start)
        pose_config = PoseRefinementConfig(**{name: value for name, value in chosen.items() if value is not None})
    trainer = GaussianPointCloudTrainer(config, pixel_weights=args.pixel_weights, mask_erode=args.mask_erode, density=args.density,
                                        mcmc_config=mcmc_config, appearance=args.appearance, depth=args.depth, depth_config=depth_config,
                                        geometry=geometry_config, bilateral_grid=bilateral_config, background=args.background,
                                        background_config=background_config, composite_targets=args.composite_targets,
                                        filter3d=filter3d_config, pose_refinement=pose_config, validation_pose_steps=args.val_pose_steps)
    trainer.train()
