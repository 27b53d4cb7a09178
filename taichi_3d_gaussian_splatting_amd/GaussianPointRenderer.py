"""GaussianPointRenderer -- the reference's renderer class (gaussian_point_render.py:20-122) on this package: trained scenes
(one parquet, or a list of them as the visualiser's --parquet_path_list) held as a compose.SceneComposition, rendered under a
list of camera poses by the rasteriser's rgb_only path under no_grad, the frames leaving the device through frames.FrameSink.

Same nested GaussianPointRendererConfig fields and defaults, set_portrait_mode, ExtraSceneInfo, crop of the image size to
multiples of 16, near_plane=0.8, far_plane=1000., depth_to_sort_key_scale=100. and run(output_prefix).  What differs:
  - all poses are converted once, batched (SE3_to_quaternion_and_translation_torch on (F,4,4)), and become the K pose rows of
    every frame in one call (SceneComposition.camera_rows), instead of one conversion per frame;
  - a frame is converted to 8 bits on the device (gs_frame_to_u8, bit for bit the reference's clamp(image * 255, 0, 255).byte())
    and a quarter of the bytes crosses to pinned memory on a side stream while the next frame renders; files are encoded by
    the sink's writer threads;
  - run() can also write the colour-mapped depth, and with a targets.TargetStore it renders the store's views with their own
    cameras and returns per-view metrics: the 8-bit PSNR from the exact sum of squared differences, and the float PSNR and
    SSIM the trainer's validation() logs, from the same LossFunction kernels -- all read from the device once, at the end;
  - run(appearance=...) corrects the frames of the views a trained appearance table knows (appearance.py: the per-view affine
    colour transform of exposure compensation) before they are converted to 8 bits, and adds psnr_cc per view: the PSNR after
    the best affine fit of the rendering to its ground truth; an entry that is a (Gy,Gx,L,12) bilateral grid (bilateral.py) is
    sliced over its frame instead;
  - render(background=...) and run(background=...) composite every frame over a background.BackgroundModel (a solid colour,
    or the sky a trainer saved) before it is converted to 8 bits.  This takes the depth rasteriser for the accumulated alpha,
    which is slower than the rgb_only path.  The sky's frame is that of the composition's first scene;
  - GaussianPointRenderer(config, filter3d=FILE or a filter3d.Filter3D) renders the scene under the 3D smoothing filter a
    trainer saved beside it (filter3d_<iteration>.pt): the features the rasteriser is given are the filtered ones for a frame
    at factor filter3d_factor (1: the filter of a run's last, full-resolution iterations; the factor a run was trained at:
    that run's own filter, for frames finer than it ever saw), made once.  A single scene only; None, the default, is the loop
    as it was;
  - fuse() renders the poses with depth and accumulated alpha and integrates them into a fusion.TSDFVolume on the device, from
    which a triangle mesh is extracted (fusion.py).
"""
import os
from dataclasses import dataclass, field
from typing import List, Optional, Union

import numpy as np
import torch

from . import appearance as _appearance
from . import background as _background
from . import bilateral as _bilateral
from . import frames, fusion
from .Camera import CameraInfo
from .compose import SceneComposition
from .GaussianPointCloudRasterisation import GaussianPointCloudRasterisation
from .LossFunction import LossFunction
from .utils import SE3_to_quaternion_and_translation_torch


class GaussianPointRenderer:
    @dataclass
    class GaussianPointRendererConfig:
        parquet_path: Union[str, List[str]]
        cameras: torch.Tensor
        device: str = "cuda"
        image_height: int = 544
        image_width: int = 976
        camera_intrinsics: torch.Tensor = field(default_factory=lambda: torch.tensor(
            [[581.743, 0.0, 488.0], [0.0, 581.743, 272.0], [0.0, 0.0, 1.0]]))

        def set_portrait_mode(self):
            self.image_height = 976
            self.image_width = 544
            self.camera_intrinsics = torch.tensor(
                [[1163.486, 0.0, 272.0], [0.0, 1163.486, 488.0], [0.0, 0.0, 1.0]])

    ExtraSceneInfo = SceneComposition.ExtraSceneInfo

    def __init__(self, config: "GaussianPointRenderer.GaussianPointRendererConfig", frame_format: str = "png", slots: int = 4,
                 filter3d=None, filter3d_factor=1) -> None:
        self.config = config
        self.config.image_height = self.config.image_height - self.config.image_height % 16
        self.config.image_width = self.config.image_width - self.config.image_width % 16
        paths = [config.parquet_path] if isinstance(config.parquet_path, (str, bytes, os.PathLike)) else list(config.parquet_path)
        self.composition = SceneComposition(paths, device=config.device)
        self.scene = self.composition.scene
        self.extra_scene_info_dict = self.composition.extra_scene_info_dict
        self.device = self.composition.device
        self.cameras = self.config.cameras.to(device=self.device, dtype=torch.float32)
        self.camera_info = CameraInfo(
            camera_intrinsics=self.config.camera_intrinsics.to(device=self.device, dtype=torch.float32),
            camera_width=self.config.image_width,
            camera_height=self.config.image_height,
            camera_id=0,
        )
        Rast = GaussianPointCloudRasterisation
        self.rasteriser = Rast(config=Rast.GaussianPointCloudRasterisationConfig(
            near_plane=0.8, far_plane=1000., depth_to_sort_key_scale=100., rgb_only=True))
        self._rasteriser_with_depth = None
        self.frame_format, self.slots = frame_format, slots
        self.loss_function = LossFunction(LossFunction.LossFunctionConfig(enable_regularization=False))
        self.filter3d = None
        self._filtered = None
        if filter3d is not None:
            from .filter3d import Filter3D
            if len(paths) != 1:
                raise ValueError("filter3d needs a single scene: a saved table belongs to the rows of one scene file")
            self.filter3d = Filter3D.load(str(filter3d), self.scene) if isinstance(filter3d, (str, bytes, os.PathLike)) else filter3d
            with torch.no_grad():           # the scene does not change between frames: filtered once
                self._filtered = self.filter3d.features(filter3d_factor).detach()

    def _with_depth(self):
        if self._rasteriser_with_depth is None:
            Rast = GaussianPointCloudRasterisation
            self._rasteriser_with_depth = Rast(config=Rast.GaussianPointCloudRasterisationConfig(
                near_plane=0.8, far_plane=1000., depth_to_sort_key_scale=100.))
        return self._rasteriser_with_depth

    def pose_rows(self, cameras: Optional[torch.Tensor] = None):
        """(F,4,4) T_pointcloud_camera (default: the config's cameras) -> (F,K,4), (F,K,3): the pose rows of every frame for
        the composition's current placements, converted once"""
        cameras = self.cameras if cameras is None else cameras.to(device=self.device, dtype=torch.float32)
        q, t = SE3_to_quaternion_and_translation_torch(cameras)
        K = len(self.composition)
        q_rows, t_rows = self.composition.camera_rows(q, t)
        return q_rows.reshape(-1, K, 4), t_rows.reshape(-1, K, 3)

    def render(self, q_rows: torch.Tensor, t_rows: torch.Tensor, camera_info: Optional[CameraInfo] = None, depth: bool = False,
               alpha: bool = False, keep_frame: bool = False, background=None):
        """one frame under the (K,4), (K,3) pose rows -> (image (H,W,3) f32, depth (H,W) or None), band 3, no gradient; with
        alpha=True (which takes the depth rasteriser) a third value, the accumulated alpha (H,W).  keep_frame (with depth or
        alpha): the depth rasteriser keeps the frame for render_channels.  background (a background.BackgroundModel): the image
        is composited over it, which takes the depth rasteriser too; the view direction of a sky is that of pose row 0"""
        Rast = GaussianPointCloudRasterisation
        wanted_alpha, alpha = alpha, alpha or background is not None
        with torch.no_grad():
            outputs = (self._with_depth() if depth or alpha else self.rasteriser)(Rast.GaussianPointCloudRasterisationInput(
                point_cloud=self.scene.point_cloud,
                point_cloud_features=self.scene.point_cloud_features if self._filtered is None else self._filtered,
                point_invalid_mask=self.scene.point_invalid_mask,
                point_object_id=self.scene.point_object_id,
                camera_info=self.camera_info if camera_info is None else camera_info,
                q_pointcloud_camera=q_rows,
                t_pointcloud_camera=t_rows,
                color_max_sh_band=3,
            ), **({"return_accumulated_alpha": True} if alpha else {}), **({"keep_frame": True} if keep_frame else {}))
        image, image_depth = outputs[0], outputs[1]
        if background is not None:
            info = self.camera_info if camera_info is None else camera_info
            with torch.no_grad():       # in the rasteriser's layout, so the composited frame is again a contiguous (H,W,3)
                image = _background.composite_forward(image.permute(2, 0, 1), outputs[3], background.coef, background.bands,
                                                      q_rows[:1].contiguous(), info.camera_intrinsics.contiguous()).permute(1, 2, 0)
        if wanted_alpha:
            return image, (image_depth if depth else None), outputs[3]
        return image, (image_depth if depth else None)

    def fuse(self, volume: fusion.TSDFVolume, cameras: Optional[torch.Tensor] = None) -> fusion.TSDFVolume:
        """Render every pose ((F,4,4) T_pointcloud_camera, default: the config's cameras) with depth and accumulated alpha
        through the depth rasteriser under no_grad and integrate the frames into `volume`, fusion.VIEWS_PER_LAUNCH views per
        library call.  The poses and the intrinsics are taken from their host copies; no frame is copied to the host and
        nothing here waits for the device.  -> volume"""
        cameras = self.config.cameras if cameras is None else cameras
        q_rows, t_rows = self.pose_rows(cameras)
        q_world, t_world = SE3_to_quaternion_and_translation_torch(cameras.detach().to(device="cpu", dtype=torch.float32))
        q_world, t_world = q_world.numpy(), t_world.numpy()
        host_info = CameraInfo(camera_intrinsics=self.config.camera_intrinsics.detach().to(device="cpu", dtype=torch.float32),
                               camera_width=self.config.image_width, camera_height=self.config.image_height, camera_id=0)
        for first in range(0, q_rows.shape[0], fusion.VIEWS_PER_LAUNCH):
            batch = range(first, min(first + fusion.VIEWS_PER_LAUNCH, q_rows.shape[0]))
            rendered = [self.render(q_rows[i], t_rows[i], depth=True, alpha=True) for i in batch]
            volume.integrate([r[1] for r in rendered], [q_world[i] for i in batch], [t_world[i] for i in batch], host_info,
                             alpha=[r[2] for r in rendered], image=[r[0] for r in rendered])
        return volume

    def write_normals(self, directory, targets=None, max_rel_jump: float = 0.1, source: str = "depth", min_length: float = 0.5):
        """Render every camera of the config (or every view of `targets`, a targets.TargetStore, under its own pose and camera)
        with depth and write the depth-derived camera-space normal map (geometry.depth_normals: x right, y down, z forward)
        to <directory>/normal_<i:03>.png as the 8-bit RGB image (n + 1) / 2, (0,0,0) where there is no normal -- the encoding
        ImagePoseDataset.load_normal reads.  The intrinsics are read by the host once per camera.  -> the number of files
        source="gaussians": the rendered per-Gaussian normals instead (normals.rendered_normals over the kept frame), normalised
        per pixel where the blend is at least min_length long, (0,0,0) elsewhere; same encoder."""
        import PIL.Image
        from . import geometry
        from . import normals as _normals
        if source not in ("depth", "gaussians"):
            raise ValueError(f'source must be "depth" or "gaussians", got {source!r}')
        min_length = _normals._positive(min_length, "min_length")
        os.makedirs(str(directory), exist_ok=True)
        if targets is None:
            q_rows, t_rows = self.pose_rows()
            infos = [self.camera_info] * q_rows.shape[0]
        else:
            K = len(self.composition)
            q_rows, t_rows = self.composition.camera_rows(targets.q, targets.t)
            q_rows, t_rows = q_rows.reshape(len(targets), K, 4), t_rows.reshape(len(targets), K, 3)
            infos = [targets.target(i, 1)[3] for i in range(len(targets))]
        intrinsics = {}
        for i, info in enumerate(infos):
            if source == "gaussians":
                rast = self._with_depth()
                self.render(q_rows[i], t_rows[i], camera_info=info, depth=True, keep_frame=True)
                with torch.no_grad():
                    rendered = _normals.rendered_normals(rast, self.scene, (q_rows[i].contiguous(), t_rows[i].contiguous()))
                    coded = geometry.normals_to_uint8(_normals.unit_normals(rendered, min_length))
                PIL.Image.fromarray(coded.cpu().numpy()).save(os.path.join(str(directory), f"normal_{i:03d}.png"))
                continue
            if id(info.camera_intrinsics) not in intrinsics:
                intrinsics[id(info.camera_intrinsics)] = geometry.intrinsics_tuple(info.camera_intrinsics)
            _, image_depth = self.render(q_rows[i], t_rows[i], camera_info=info, depth=True)
            normals = geometry.depth_normals(image_depth.contiguous(), intrinsics[id(info.camera_intrinsics)], max_rel_jump)
            PIL.Image.fromarray(geometry.normals_to_uint8(normals).cpu().numpy()).save(os.path.join(str(directory), f"normal_{i:03d}.png"))
        return len(infos)

    def run(self, output_prefix, depth: bool = False, targets=None, gt_prefix=None, appearance=None, image_paths=None, background=None):
        """Render every camera of the config to <output_prefix>/frame_<i:03>.<format> (and depth_<i:03> with depth=True).
        output_prefix None: the frames still cross to the host, nothing is written.

        targets (a targets.TargetStore): its views are rendered instead, each under its own pose and camera, and compared with
        its image; gt_prefix then receives the ground-truth frames -- the stored bytes where the store holds the decoded
        image, RGB_ROUND of the resized f32 image otherwise.  -> None without targets, else a dict with `views` (per view:
        psnr_8bit from the exact SSE, psnr and ssim as the trainer's validation() computes them) and their `mean`.

        appearance ({image path: (12,) transform on the device}, AppearanceTable.by_image_path) with image_paths (the path of
        every view of `targets`, in order): a view whose path is in the dict is corrected by its transform before it is
        converted to 8 bits and measured; every other frame is rendered as without it.  A value may also be the view's
        (Gy,Gx,L,12) bilateral grid (BilateralGridTable.by_image_path), which is sliced over the frame.  Every view then also gets psnr_cc:
        the float PSNR after appearance.fit_affine(rendering, ground truth), which reads 23 numbers to the host per view.

        background (a background.BackgroundModel): every frame is composited over it before anything else is done with it."""
        if appearance is not None:
            if targets is None or image_paths is None or len(image_paths) != len(targets):
                raise ValueError("appearance needs targets and the image path of every one of its views")
        directory = None if output_prefix is None else str(output_prefix)
        sink = frames.FrameSink(directory, fmt=self.frame_format, slots=self.slots, device=self.device)
        gt_sink = None
        if targets is not None and gt_prefix is not None:
            gt_sink = frames.FrameSink(str(gt_prefix), fmt=self.frame_format, slots=self.slots, device=self.device)
        if targets is None:
            q_rows, t_rows = self.pose_rows()
            for i in range(q_rows.shape[0]):
                image, image_depth = self.render(q_rows[i], t_rows[i], depth=depth, background=background)
                sink.submit(image, depth=image_depth)
            sink.close()
            return None
        n = len(targets)
        K = len(self.composition)
        q_rows, t_rows = self.composition.camera_rows(targets.q, targets.t)
        q_rows, t_rows = q_rows.reshape(n, K, 4), t_rows.reshape(n, K, 3)
        float_metrics = torch.zeros((n, 3), dtype=torch.float32, device=self.device)      # psnr, ssim, psnr_cc
        sizes = []
        for i in range(n):
            image_gt, _, _, info = targets.target(i, 1)
            h, w = info.camera_height, info.camera_width
            image, image_depth = self.render(q_rows[i], t_rows[i], camera_info=info, depth=depth, background=background)
            if appearance is not None and str(image_paths[i]) in appearance:
                # in the rasteriser's layout, so the corrected frame is again a contiguous (H,W,3)
                correction = appearance[str(image_paths[i])]
                correct = _bilateral.slice_forward if correction.dim() == 4 else _appearance.apply_forward
                image = correct(image.permute(2, 0, 1), correction).permute(1, 2, 0)
            stored = targets.images[i]
            if stored.dtype == torch.uint8:
                gt_bytes = stored
            else:                           # an autoscaled view: its f32 image, rounded to the bytes it is compared as
                gt_bytes = frames.frame_to_u8(image_gt.permute(1, 2, 0).contiguous(), frames.RGB_ROUND)
            sink.submit(image, depth=image_depth, gt=gt_bytes)
            if gt_sink is not None:
                gt_sink.submit(gt_bytes[:h, :w])
            with torch.no_grad():           # GaussianPointTrainer.validation(): clamp, then the loss kernels and the mse
                image_pred = torch.clamp(image, 0, 1).permute(2, 0, 1)
                _, _, ssim_loss = self.loss_function(image_pred, image_gt)
                float_metrics[i, 0] = 10 * torch.log10(1.0 / torch.mean((image_pred - image_gt) ** 2))
                float_metrics[i, 1] = 1.0 - ssim_loss
                if appearance is not None:
                    image_cc = torch.clamp(_appearance.apply_forward(image_pred, _appearance.fit_affine(image_pred, image_gt)), 0, 1)
                    float_metrics[i, 2] = 10 * torch.log10(1.0 / torch.mean((image_cc - image_gt) ** 2))
            sizes.append(h * w * 3)
        sse = sink.close().numpy()
        if gt_sink is not None:
            gt_sink.close()
        float_metrics = float_metrics.cpu().numpy().astype(np.float64)
        psnr_8bit = [float(frames.psnr_from_sse(s, size)) for s, size in zip(sse, sizes)]
        views = [dict(index=i, sse_8bit=int(sse[i]), psnr_8bit=psnr_8bit[i], psnr=float(float_metrics[i, 0]), ssim=float(float_metrics[i, 1]))
                 for i in range(n)]
        names = ("psnr_8bit", "psnr", "ssim")
        if appearance is not None:
            names += ("psnr_cc",)
            for i, v in enumerate(views):
                v["psnr_cc"] = float(float_metrics[i, 2])
        mean = {name: float(np.mean([v[name] for v in views])) if views else float("nan") for name in names}
        return dict(views=views, mean=mean)
