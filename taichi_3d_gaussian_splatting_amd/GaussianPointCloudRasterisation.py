"""GaussianPointCloudRasterisation -- drop-in for the reference operator
(taichi_3d_gaussian_splatting/GaussianPointCloudRasterisation.py:775-1204) backed by
libgsrast.so (hand-written HIP for MI355X / gfx950) through its C ABI.

Same class, nested dataclass names, field order, forward() contract and backward-hook
payload as the reference.  The Python side only validates arguments, allocates the output
tensors, keeps the opaque frame handle alive between forward and backward and dispatches
the hook; all arithmetic happens in the library (called through _native.call()).  There is no fallback path.
"""
from dataclasses import dataclass
from typing import Callable, Optional

import torch

from . import _native, channels, sparse
from ._host import _ConfigBase, _Contexts, _Frame, _marshal
from .Camera import CameraInfo
from .controller_stats import ControllerAccumulators

TILE_WIDTH = 16
TILE_HEIGHT = 16


class GaussianPointCloudRasterisation(torch.nn.Module):
    @dataclass
    class GaussianPointCloudRasterisationConfig(_ConfigBase):
        near_plane: float = 0.8
        far_plane: float = 1000.
        depth_to_sort_key_scale: float = 100.
        rgb_only: bool = False
        # un-annotated on purpose, as in the reference (RAST:782-786): class attributes, not fields
        grad_color_factor = 5.
        grad_high_order_color_factor = 1.
        grad_s_factor = 0.5
        grad_q_factor = 1.
        grad_alpha_factor = 20.
        # extension over the reference: True lifts the W,H % 16 == 0 requirement (e.g. a true 1920x1080 frame)
        allow_partial_tiles = False
        # extension: True runs the backward's per-contribution Gaussian gradient (utils.py:331-348) in the reference's own f32
        # operation order instead of the faster, algebraically equal form (gs_config.bwd_reference_order)
        backward_reference_order = False
        # extension: True makes rasterized_depth differentiable (the reference drops its gradient, RAST:1157-1163): a loss on
        # the depth map then reaches the point and pose gradients (gs_backward_ex).  Read at forward time; no effect with rgb_only
        differentiable_depth = False

    @dataclass
    class GaussianPointCloudRasterisationInput:
        point_cloud: torch.Tensor  # Nx3
        point_cloud_features: torch.Tensor  # Nx56
        point_object_id: torch.Tensor  # N, int32, index into the pose rows
        point_invalid_mask: torch.Tensor  # N, int8
        camera_info: CameraInfo
        q_pointcloud_camera: torch.Tensor  # Kx4, xyzw
        t_pointcloud_camera: torch.Tensor  # Kx3
        color_max_sh_band: int = 2

    @dataclass
    class BackwardValidPointHookInput:
        point_id_in_camera_list: torch.Tensor  # M
        grad_point_in_camera: torch.Tensor  # Mx3
        grad_pointfeatures_in_camera: torch.Tensor  # Mx56
        grad_viewspace: torch.Tensor  # Mx2
        magnitude_grad_viewspace: torch.Tensor  # M
        magnitude_grad_viewspace_on_image: torch.Tensor  # HxWx2
        num_overlap_tiles: torch.Tensor  # M
        num_affected_pixels: torch.Tensor  # M
        point_depth: torch.Tensor  # M
        point_uv_in_camera: torch.Tensor  # Mx2

    # extension (a plain attribute, not a config field: the config's field order mirrors the reference): True makes every
    # backward leave the rows it touched in last_touched_rows (sparse.TouchedRows, for FusedAdam.step(rows=...)); None
    # after a backward that computed no point gradients
    track_touched_rows = False

    def __init__(self, config: "GaussianPointCloudRasterisation.GaussianPointCloudRasterisationConfig",
                 backward_valid_point_hook: Optional[Callable[["GaussianPointCloudRasterisation.BackwardValidPointHookInput"], None]] = None,
                 controller_accumulators: Optional[ControllerAccumulators] = None):
        """`controller_accumulators` is an extension over the reference signature (RAST:819-824): when given, every
        backward adds this view's densification statistics to them on the device (controller_stats.py)."""
        super().__init__()
        _native.lib()                       # fail now, loudly, if libgsrast.so is absent
        self.config = config
        self._hook = backward_valid_point_hook
        self.controller_accumulators = controller_accumulators
        self._ctxs = _Contexts()            # device index -> _native.Context (owner of the gs_ctx)
        self.last_frame: Optional[_Frame] = None   # inspection aid (tests / profiling); replaced every call
        self.last_forward_outputs = {}
        self.last_touched_rows: Optional[sparse.TouchedRows] = None
        module = self

        class _module_function(torch.autograd.Function):
            @staticmethod
            def forward(ctx, pointcloud, pointcloud_features, point_invalid_mask, point_object_id,
                        q_pointcloud_camera, t_pointcloud_camera, camera_info, color_max_sh_band, grad_mode, return_alpha,
                        keep_frame):
                # ctx.needs_input_grad says whether the inputs require grad, not whether a graph is being recorded (it is True
                # under torch.no_grad() too, and grad mode is always off inside forward): the caller passes the grad mode in
                needs_grad = bool(grad_mode and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1] or
                                                 ctx.needs_input_grad[4] or ctx.needs_input_grad[5]))
                outs, frame = module._run_forward(pointcloud, pointcloud_features, point_invalid_mask, point_object_id,
                                                  q_pointcloud_camera, t_pointcloud_camera, camera_info,
                                                  keep=needs_grad or keep_frame)
                image, depth, acc_alpha, last, count = outs
                ctx.frame = frame if needs_grad else None
                ctx.camera_info = camera_info
                ctx.color_max_sh_band = color_max_sh_band
                # extension: the depth gradient flows only with config.differentiable_depth (as of this forward)
                ctx.differentiable_depth = bool(getattr(module.config, "differentiable_depth", False)) and not module.config.rgb_only
                ctx.save_for_backward(pointcloud, pointcloud_features, point_invalid_mask, point_object_id,
                                      q_pointcloud_camera, t_pointcloud_camera, acc_alpha, last,
                                      depth if ctx.differentiable_depth else None)
                ctx.mark_non_differentiable(count)
                # an output nothing downstream used gets None, not an image-sized zero tensor (a fill launch each): the count
                # (no gradient), the depth unless differentiable_depth (ignored then, RAST:1157-1163) and the alpha.  backward
                # therefore takes gs_backward_ex only for a depth or alpha gradient that actually arrives
                ctx.set_materialize_grads(False)
                if return_alpha:                            # extension: pixel_accumulated_alpha as a differentiable output
                    return image, depth, count, acc_alpha
                return image, depth, count

            @staticmethod
            def backward(ctx, grad_rasterized_image, grad_rasterized_depth, grad_pixel_valid_point_count, *grad_alpha):
                grad_pointcloud = grad_pointcloud_features = grad_q = grad_t = None
                want_points = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]      # RAST:1028
                want_pose = ctx.needs_input_grad[4] or ctx.needs_input_grad[5]        # extension: the reference returns None for the pose
                if want_points or want_pose:
                    if ctx.frame is None:
                        raise RuntimeError("backward through a forward that ran without gradient tracking")
                    (pointcloud, pointcloud_features, point_invalid_mask, point_object_id, q_pointcloud_camera,
                     t_pointcloud_camera, acc_alpha, last, depth) = ctx.saved_tensors
                    if not ctx.differentiable_depth:        # the reference's behaviour: the depth gradient does not flow (RAST:1157-1163)
                        grad_rasterized_depth = None
                    grad_acc_alpha = grad_alpha[0] if grad_alpha else None
                    if grad_rasterized_image is None:       # only the depth (or alpha) was used downstream
                        grad_rasterized_image = torch.zeros(ctx.camera_info.camera_height, ctx.camera_info.camera_width, 3,
                                                            dtype=torch.float32, device=pointcloud.device)
                    grad_pointcloud, grad_pointcloud_features, grad_q, grad_t = module._run_backward(
                        ctx.frame, pointcloud, pointcloud_features, point_invalid_mask, point_object_id,
                        q_pointcloud_camera, t_pointcloud_camera, ctx.camera_info, acc_alpha, last,
                        grad_rasterized_image.contiguous(), ctx.color_max_sh_band, want_points=want_points, want_pose=want_pose,
                        grad_depth=grad_rasterized_depth, depth=depth, grad_alpha=grad_acc_alpha)
                    # the frame is NOT released here: like the reference's saved tensors it lives as long as the graph
                    # node does, so backward(retain_graph=True) followed by another backward works; it goes back to the
                    # pool when autograd drops the node (_Frame.__del__)
                return (grad_pointcloud, grad_pointcloud_features, None, None,
                        grad_q if ctx.needs_input_grad[4] else None, grad_t if ctx.needs_input_grad[5] else None, None, None, None, None, None)

        self._module_function = _module_function

    # ------------------------------------------------------------------ helpers
    def _ctx_for(self, device: torch.device):
        """The raw gs_ctx* of this module on `device` (profiling / diagnostics)."""
        return self._ctxs.of(device).handle

    def _run_forward(self, pointcloud, features, mask, obj, q, t, camera_info, keep):
        scene, cam, cfg, Kmat = _marshal(self.config, pointcloud, features, mask, obj, q, t, camera_info)
        dev = pointcloud.device
        H, W = camera_info.camera_height, camera_info.camera_width
        image = torch.empty(H, W, 3, dtype=torch.float32, device=dev)                   # RAST:967-976
        depth = torch.empty(H, W, dtype=torch.float32, device=dev)
        acc_alpha = torch.empty(H, W, dtype=torch.float32, device=dev)
        last = torch.empty(H, W, dtype=torch.int32, device=dev)
        count = torch.empty(H, W, dtype=torch.int32, device=dev)
        out = _native.GsForwardOut.of(image, depth, acc_alpha, last, count)
        frame = _Frame.of_call("gs_forward", self._ctxs.of(dev), dev, scene, cam, cfg, out, keep=keep)
        if keep:
            frame.marshalled = (scene, cam, cfg)       # the backward of this frame reads the same tensors (Kmat is kept alive below)
            frame._keepalive = Kmat
        frame.last = None if self.config.rgb_only else last      # what render_channels walks the frame with
        self.last_frame = frame
        self.last_forward_outputs = {"pixel_accumulated_alpha": acc_alpha, "pixel_offset_of_last_effective_point": last}
        return (image, depth, acc_alpha, last, count), frame

    def _run_backward(self, frame, pointcloud, features, mask, obj, q, t, camera_info, acc_alpha, last, grad_image, sh_band,
                      want_points=True, want_pose=False, grad_depth=None, depth=None, grad_alpha=None):
        """-> (grad_pointcloud, grad_pointcloud_features, grad_q, grad_t); the first two are None when not want_points (no hook
        call and no controller statistics then, as in the reference, RAST:1028), the last two None when not want_pose.
        grad_depth (with the forward's depth) and grad_alpha, (H,W) or None: gs_backward_ex when either is given."""
        dev = pointcloud.device
        N, M = pointcloud.shape[0], frame.n_points_in_camera
        H, W = camera_info.camera_height, camera_info.camera_width
        # The host part of a backward sits on the step's critical path (the GPU has about one forward blend of queued work
        # when autograd gets here), so it is kept short: the inputs were validated and marshalled by the forward of this
        # frame (same tensors: autograd's saved tensors), and everything the hook receives comes out of ONE allocation.
        ms = frame.marshalled
        if ms is None or (ms[0].point_cloud, ms[0].point_cloud_features, ms[0].point_invalid_mask, ms[0].point_object_id, ms[0].n_points,
                          ms[1].q_pointcloud_camera, ms[1].t_pointcloud_camera) != (
                pointcloud.data_ptr() or None, features.data_ptr() or None, mask.data_ptr() or None, obj.data_ptr() or None, pointcloud.shape[0],
                q.data_ptr() or None, t.data_ptr() or None):
            ms = _marshal(self.config, pointcloud, features, mask, obj, q, t, camera_info)   # storage was swapped since the forward (p.data = ...)
        scene, cam = ms[0], ms[1]       # (a re-marshalled ms[3], the intrinsics, lives in `ms` until this call returns)
        cfg = _native.GsConfig.of(self.config)     # read again: the grad factors (and bwd_reference_order) may have changed since the forward
        if grad_image.dtype != torch.float32 or tuple(grad_image.shape) != (H, W, 3):
            raise ValueError("grad of rasterized_image must be float32 (H,W,3)")
        # one allocation for both gradients so that data-parallel training all-reduces ONE buffer; the 56-float rows
        # come first: 224*N bytes keep them 16-byte aligned for any N (the kernels store them as float4)
        grad_pc = grad_feat = grad_q = grad_t = None
        if want_points:
            flat = torch.empty(N * 59, dtype=torch.float32, device=dev)
            grad_feat = flat[:N * 56].view(N, 56)
            grad_pc = flat[N * 56:].view(N, 3)
        if want_pose:
            # (n_objects,4) and (n_objects,3) float32, one allocation; every row is written
            pose_flat = torch.empty(q.shape[0] * 7, dtype=torch.float32, device=dev)
            grad_q = pose_flat[:q.shape[0] * 4].view(q.shape[0], 4)
            grad_t = pose_flat[q.shape[0] * 4:].view(q.shape[0], 3)
        want_hook = self._hook is not None and want_points
        grad_uv = mag = mag_img = n_aff = h_pc = h_feat = h_uv = h_mag = h_ids = h_ntiles = h_depth = h_puv = None
        if want_hook:
            # twelve arrays, one buffer and one split (the 56-float rows first: the kernel stores them as float4 and the buffer
            # is aligned); a Python-level tensor op costs 1-2 us, so fewer of them is what shortens this path
            sizes = (M * 56, M * 3, M * 2, M, M, M * 2, N * 2, N, H * W * 2, M, M, M)
            parts = torch.empty(sum(sizes), dtype=torch.float32, device=dev).split(sizes)
            h_feat, h_pc, h_uv, h_mag, h_depth, h_puv = parts[0].view(M, 56), parts[1].view(M, 3), parts[2].view(M, 2), parts[3], parts[4], parts[5].view(M, 2)
            grad_uv, mag, mag_img = parts[6].view(N, 2), parts[7], parts[8].view(H, W, 2)
            n_aff, h_ids, h_ntiles = parts[9].view(torch.int32), parts[10].view(torch.int32), parts[11].view(torch.int32)
        ctrl = None
        if self.controller_accumulators is not None and want_points:
            self.controller_accumulators.validate(N, dev)
            if N > 0:
                ctrl = _native.GsControllerAccumulators.of(self.controller_accumulators)
        out = _native.GsBackwardOut.of(
            controller=ctrl, grad_pointcloud=grad_pc, grad_pointcloud_features=grad_feat, grad_viewspace=grad_uv,
            magnitude_grad_viewspace=mag, magnitude_grad_viewspace_on_image=mag_img, num_affected_pixels=n_aff,
            hook_grad_point_in_camera=h_pc, hook_grad_pointfeatures_in_camera=h_feat, hook_grad_viewspace=h_uv,
            hook_magnitude_grad_viewspace=h_mag, hook_point_id_in_camera_list=h_ids, hook_num_overlap_tiles=h_ntiles,
            hook_point_depth=h_depth, hook_point_uv_in_camera=h_puv, grad_q_pointcloud_camera=grad_q, grad_t_pointcloud_camera=grad_t)
        ptr, ctxh = _native.ptr, self._ctx_for(dev)
        if grad_depth is None and grad_alpha is None:
            _native.call("gs_backward", dev, ctxh, frame.handle, scene, cam, cfg, ptr(grad_image), ptr(acc_alpha), ptr(last),
                         int(sh_band), out)
        else:
            if grad_depth is not None and depth is None:
                raise ValueError("a depth gradient needs the forward's rasterized_depth")
            for g, name in ((grad_depth, "rasterized_depth"), (grad_alpha, "accumulated_alpha")):
                if g is not None and (g.dtype != torch.float32 or tuple(g.shape) != (H, W)):
                    raise ValueError(f"grad of {name} must be float32 (H,W)")
            grad_depth = grad_depth.contiguous() if grad_depth is not None else None
            grad_alpha = grad_alpha.contiguous() if grad_alpha is not None else None
            extra = _native.GsBackwardExtra(grad_rasterized_depth=ptr(grad_depth), rasterized_depth=ptr(depth) if grad_depth is not None else None,
                                            grad_pixel_accumulated_alpha=ptr(grad_alpha))
            _native.call("gs_backward_ex", dev, ctxh, frame.handle, scene, cam, cfg, ptr(grad_image), extra, ptr(acc_alpha), ptr(last),
                         int(sh_band), out)
        if self.track_touched_rows:             # same stream, directly behind the backward whose tags it reads; one allocation
            self.last_touched_rows = sparse.touched_rows(frame) if want_points else None
        self.last_backward_extras = dict(grad_viewspace=grad_uv, magnitude_grad_viewspace=mag,
                                         magnitude_grad_viewspace_on_image=mag_img, num_affected_pixels=n_aff)
        if want_hook:                                                                   # RAST:1127-1142
            self._hook(GaussianPointCloudRasterisation.BackwardValidPointHookInput(
                point_id_in_camera_list=h_ids,
                grad_point_in_camera=h_pc, grad_pointfeatures_in_camera=h_feat, grad_viewspace=h_uv,
                magnitude_grad_viewspace=h_mag, magnitude_grad_viewspace_on_image=mag_img,
                num_overlap_tiles=h_ntiles, num_affected_pixels=n_aff,
                point_depth=h_depth, point_uv_in_camera=h_puv))
        return grad_pc, grad_feat, grad_q, grad_t

    # ------------------------------------------------------------------ nn.Module
    def forward(self, input_data: "GaussianPointCloudRasterisation.GaussianPointCloudRasterisationInput",
                return_accumulated_alpha: bool = False, keep_frame: bool = False):
        """-> (rasterized_image, rasterized_depth, pixel_valid_point_count), as the reference; with return_accumulated_alpha
        (extension) a fourth output, pixel_accumulated_alpha (H,W) = 1 - final transmittance, which is differentiable.
        keep_frame (extension): keep the frame (self.last_frame) even when no input requires grad or under torch.no_grad(),
        so that render_channels can be differentiated on it with the geometry frozen."""
        camera_info = input_data.camera_info
        if not getattr(self.config, "allow_partial_tiles", False):
            assert camera_info.camera_width % TILE_WIDTH == 0        # RAST:1193-1194
            assert camera_info.camera_height % TILE_HEIGHT == 0
        if return_accumulated_alpha and self.config.rgb_only:
            raise ValueError("return_accumulated_alpha needs the full forward: rgb_only computes no accumulated alpha")
        if keep_frame and self.config.rgb_only:
            raise ValueError("keep_frame needs the full forward: an rgb_only frame cannot be kept")
        return self._module_function.apply(
            input_data.point_cloud, input_data.point_cloud_features, input_data.point_invalid_mask,
            input_data.point_object_id, input_data.q_pointcloud_camera, input_data.t_pointcloud_camera,
            camera_info, input_data.color_max_sh_band, torch.is_grad_enabled(), bool(return_accumulated_alpha), bool(keep_frame))

    def render_channels(self, values: torch.Tensor, frame: Optional[_Frame] = None) -> torch.Tensor:
        """values (N,C) float32, C <= 64 -> (H,W,C): the per-Gaussian channels blended over `frame` (default: the frame of
        the last forward) with the colour's own weights alpha_i T_i; differentiable in `values` only (channels.py)."""
        return channels.render_channels(values, self.last_frame if frame is None else frame)
