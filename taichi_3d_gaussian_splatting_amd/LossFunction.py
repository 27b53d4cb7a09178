"""LossFunction -- same class, config and return triple as the reference's LossFunction.py:8-51,
   L = (1 - lambda) L1 + lambda (1 - SSIM) [+ regularization_weight * mean ||exp(s)||],
with the L1 + SSIM part (value and gradient) computed by libgsrast in three HIP launches
(gs_loss_l1_ssim_forward / _backward) instead of pytorch_msssim's conv2d chain + autograd.  SSIM follows
pytorch_msssim.ssim(data_range=1, size_average=True): 11-tap Gaussian window (sigma 1.5), valid filtering,
K1 = 0.01, K2 = 0.03.  The scale regulariser is fused as well (gs_scale_regulariser[_grad]): in torch its
boolean-mask indexing and the sort-based index_put of its backward cost more than the rasteriser's backward.
The library calls go through _native.call().

With pixel_weight the same three launches compute the weighted loss of include/gs_loss_weighted.h
(gs_loss_l1_ssim_weighted_forward / _backward): masked training."""
import ctypes as C
from dataclasses import dataclass

import torch
import torch.nn as nn

from . import _native
from ._host import _ConfigBase
from ._native import ptr as _ptr


def check_loss_images(predicted, ground_truth):
    """Raise unless both images are float32 (3,H,W) tensors on the same GPU with H, W >= 11 (the SSIM window).  Reads no
    data and launches nothing: the kernels take raw pointers, and a host pointer handed to them faults the device."""
    if predicted.dim() != 3 or predicted.shape[0] != 3 or predicted.shape != ground_truth.shape:
        raise ValueError("predicted_image and ground_truth_image must both be (3,H,W)")
    if predicted.dtype != torch.float32 or ground_truth.dtype != torch.float32 or not predicted.is_cuda:
        raise TypeError("images must be float32 tensors on the GPU")
    if ground_truth.device != predicted.device:
        raise ValueError(f"ground_truth_image is on {ground_truth.device}, predicted_image on {predicted.device}")
    if predicted.shape[1] < 11 or predicted.shape[2] < 11:
        raise ValueError(f"images of {predicted.shape[1]}x{predicted.shape[2]} are smaller than the 11x11 SSIM window")


_VP, _I32, _F32, _IMG = C.c_void_p, C.c_int32, C.c_float, C.POINTER(_native.GsLossImage)
ARGTYPES = {
    # (ctx, predicted, ground_truth, pixel_weight, H, W, clamp_predicted, lambda, maps, loss_terms[5], stream)
    "gs_loss_l1_ssim_weighted_forward": [_VP, _IMG, _IMG, _VP, _I32, _I32, _I32, _F32, _VP, _VP, _VP],
    # (ctx, predicted, ground_truth, pixel_weight, H, W, clamp_predicted, lambda, maps, loss_terms, upstream, grad_predicted, stream)
    "gs_loss_l1_ssim_weighted_backward": [_VP, _IMG, _IMG, _VP, _I32, _I32, _I32, _F32, _VP, _VP, _VP, _IMG, _VP],
}
_bound = False


def _bind():
    """argtypes of the weighted entry points, set once on the loaded library (they are not part of _native.SYMBOLS)"""
    global _bound
    if not _bound:
        L = _native.lib()
        for name, argtypes in ARGTYPES.items():
            if not hasattr(L, name):
                raise _native.NativeLibraryError(f"{_native.LIB_PATH} does not export {name}")
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
        _bound = True


def check_pixel_weight(pixel_weight, predicted):
    """Raise unless pixel_weight is a contiguous float32 (H,W) tensor on the device of the (3,H,W) predicted image.  Reads no
    data and launches nothing."""
    if not isinstance(pixel_weight, torch.Tensor):
        raise TypeError("pixel_weight must be a tensor")
    H, W = int(predicted.shape[-2]), int(predicted.shape[-1])
    if tuple(pixel_weight.shape) != (H, W):
        raise ValueError(f"pixel_weight must be ({H},{W}), got {tuple(pixel_weight.shape)}")
    if pixel_weight.dtype != torch.float32:
        raise TypeError(f"pixel_weight must be float32, got {pixel_weight.dtype}")
    if pixel_weight.device != predicted.device:
        raise ValueError(f"pixel_weight is on {pixel_weight.device}, predicted_image on {predicted.device}")
    if not pixel_weight.is_contiguous():
        raise ValueError("pixel_weight must be contiguous")


def check_regulariser_inputs(features, invalid_mask):
    """Raise unless features is a contiguous float32 (N,56) GPU tensor and invalid_mask an (N,) bool or integer tensor on
    the same device.  Returns the mask as the contiguous int8 (N,) tensor the kernels read (the input itself when it
    already is one; a copy otherwise).  Reads no data and launches nothing."""
    if features.dtype != torch.float32 or not features.is_cuda or not features.is_contiguous() or features.dim() != 2 \
            or features.shape[1] != 56:
        raise TypeError("pointcloud_features must be a contiguous float32 (N,56) GPU tensor")
    if invalid_mask.device != features.device:
        raise ValueError(f"point_invalid_mask is on {invalid_mask.device}, pointcloud_features on {features.device}")
    if invalid_mask.dim() != 1 or invalid_mask.shape[0] != features.shape[0]:
        raise ValueError(f"point_invalid_mask must be ({features.shape[0]},), got {tuple(invalid_mask.shape)}")
    if invalid_mask.dtype == torch.int8:
        mask = invalid_mask
    elif invalid_mask.dtype == torch.bool or not (invalid_mask.is_floating_point() or invalid_mask.is_complex()):
        mask = (invalid_mask != 0).to(torch.int8)               # (a plain .to(int8) would wrap 256 to 0)
    else:
        raise TypeError(f"point_invalid_mask must be bool or integer, got {invalid_mask.dtype}")
    return mask.contiguous()


class _L1SSIM(torch.autograd.Function):
    """Forward: gs_loss_l1_ssim_forward (value; the derivative maps stay in a tensor this node owns).  Backward:
    gs_loss_l1_ssim_backward, scaled by the incoming gradient on the device.  The predicted image is read through its strides:
    the rasteriser's (H,W,3) output viewed as (3,H,W) by permute(2,0,1) needs no copy, and its gradient is written in the
    same layout."""

    @staticmethod
    def forward(ctx, predicted, ground_truth, lambda_value, clamp_predicted):
        check_loss_images(predicted, ground_truth)
        dev = predicted.device
        H, W = int(predicted.shape[1]), int(predicted.shape[2])
        terms = torch.empty(3, dtype=torch.float32, device=dev)
        maps = torch.empty(_native.lib().gs_loss_maps_floats(H, W), dtype=torch.float32, device=dev)
        _native.call("gs_loss_l1_ssim_forward", dev, _native.shared_ctx(dev),
                     _native.GsLossImage.of(predicted), _native.GsLossImage.of(ground_truth), H, W, int(bool(clamp_predicted)),
                     float(lambda_value), _ptr(maps), _ptr(terms))
        ctx.save_for_backward(predicted, ground_truth, maps)
        ctx.lambda_value, ctx.clamp_predicted = float(lambda_value), int(bool(clamp_predicted))
        ctx.mark_non_differentiable(terms)
        return terms[0], terms

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        predicted, ground_truth, maps = ctx.saved_tensors
        dev = predicted.device
        H, W = int(predicted.shape[1]), int(predicted.shape[2])
        # the gradient in the memory layout of the image it belongs to (a permuted view of an (H,W,3) buffer for a permuted input)
        # (preserve_format: the input's strides when it is dense and non-overlapping, contiguous otherwise)
        grad = torch.empty_like(predicted, memory_format=torch.preserve_format)
        up = grad_loss.reshape(1).to(torch.float32).contiguous()
        _native.call("gs_loss_l1_ssim_backward", dev, _native.shared_ctx(dev),
                     _native.GsLossImage.of(predicted), _native.GsLossImage.of(ground_truth), H, W, ctx.clamp_predicted,
                     ctx.lambda_value, _ptr(maps), _ptr(up), _native.GsLossImage.of(grad))
        return grad, None, None, None


class _L1SSIMWeighted(torch.autograd.Function):
    """_L1SSIM with a weight per pixel: gs_loss_l1_ssim_weighted_forward / _backward.  terms is {L, L1_w, 1 - SSIM_w, S_w, V};
    the backward reads S_w and V from it on the device.  The gradient goes to the predicted image only."""

    @staticmethod
    def forward(ctx, predicted, ground_truth, pixel_weight, lambda_value, clamp_predicted):
        check_loss_images(predicted, ground_truth)
        check_pixel_weight(pixel_weight, predicted)
        _bind()
        dev = predicted.device
        H, W = int(predicted.shape[1]), int(predicted.shape[2])
        terms = torch.empty(5, dtype=torch.float32, device=dev)
        maps = torch.empty(_native.lib().gs_loss_maps_floats(H, W), dtype=torch.float32, device=dev)
        _native.call("gs_loss_l1_ssim_weighted_forward", dev, _native.shared_ctx(dev),
                     _native.GsLossImage.of(predicted), _native.GsLossImage.of(ground_truth), _ptr(pixel_weight), H, W,
                     int(bool(clamp_predicted)), float(lambda_value), _ptr(maps), _ptr(terms))
        ctx.save_for_backward(predicted, ground_truth, pixel_weight, maps, terms)
        ctx.lambda_value, ctx.clamp_predicted = float(lambda_value), int(bool(clamp_predicted))
        ctx.mark_non_differentiable(terms)
        return terms[0], terms

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        predicted, ground_truth, pixel_weight, maps, terms = ctx.saved_tensors
        dev = predicted.device
        H, W = int(predicted.shape[1]), int(predicted.shape[2])
        grad = torch.empty_like(predicted, memory_format=torch.preserve_format)
        up = grad_loss.reshape(1).to(torch.float32).contiguous()
        _native.call("gs_loss_l1_ssim_weighted_backward", dev, _native.shared_ctx(dev),
                     _native.GsLossImage.of(predicted), _native.GsLossImage.of(ground_truth), _ptr(pixel_weight), H, W,
                     ctx.clamp_predicted, ctx.lambda_value, _ptr(maps), _ptr(terms), _ptr(up), _native.GsLossImage.of(grad))
        return grad, None, None, None, None


class _ScaleRegulariser(torch.autograd.Function):
    """mean over valid points of ||exp(s)||_2 (LossFunction.py:40-51) without boolean-mask indexing."""

    @staticmethod
    def forward(ctx, features, invalid_mask):
        mask = check_regulariser_inputs(features, invalid_mask)
        dev = features.device
        out = torch.empty(2, dtype=torch.float32, device=dev)
        _native.call("gs_scale_regulariser", dev, _native.shared_ctx(dev), _ptr(features), _ptr(mask),
                     features.shape[0], _ptr(out))
        ctx.save_for_backward(features, mask, out)
        return out[0]

    @staticmethod
    def backward(ctx, upstream):
        features, mask, out = ctx.saved_tensors
        dev = features.device
        grad = torch.empty_like(features)
        up = upstream.reshape(1).to(torch.float32).contiguous()
        _native.call("gs_scale_regulariser_grad", dev, _native.shared_ctx(dev), _ptr(features), _ptr(mask),
                     features.shape[0], _ptr(out), _ptr(up), _ptr(grad))
        return grad, None


class LossFunction(nn.Module):
    @dataclass
    class LossFunctionConfig(_ConfigBase):
        lambda_value: float = 0.2
        enable_regularization: bool = True
        regularization_weight: float = 2

    def __init__(self, config: "LossFunction.LossFunctionConfig"):
        super().__init__()
        self.config = config

    def forward(self, predicted_image, ground_truth_image, point_invalid_mask=None, pointcloud_features=None, clamp_predicted=False,
                pixel_weight=None):
        """predicted_image / ground_truth_image: (B, C, H, W) or (C, H, W), C = 3, any strides (the rasteriser's (H,W,3)
        output under permute(2,0,1) is read in place).  Returns (L, L1, LD_SSIM).
        clamp_predicted=True (not in the reference's signature) applies the trainer's torch.clamp(image, 0, 1)
        (GaussianPointTrainer.py:173) inside the kernels: loss_function(image_pred.permute(2, 0, 1), image_gt, ...,
        clamp_predicted=True) equals loss_function(torch.clamp(image_pred, 0, 1).permute(2, 0, 1), image_gt, ...) in value and
        gradient, without the clamp's kernels and copies.
        With B > 1 (LossFunction.py:21-33 accepts it; the reference trainer uses batch_size=None) the images are
        equally sized, so the batch means of L1 and of size_average=True SSIM are the means of the per-image values:
        the fused kernel runs once per image.
        pixel_weight (not in the reference's signature): a contiguous float32 (H,W) tensor on the images' device, or (B,H,W)
        for a batch (a single (H,W) is shared by the batch; the (1,H,W) weight of a batch of one is squeezed with it).  L1 and LD_SSIM then are the weighted terms of
        include/gs_loss_weighted.h: a pixel counts with its weight (anything not > 0 as 0), an SSIM window with the weight of
        its centre pixel; the weights get no gradient.  None is the unweighted loss."""
        # (no unsqueeze / [b] round trip for a single image: the select's backward is a zero fill and a copy of the whole image)
        if predicted_image.dim() == 4 and predicted_image.shape[0] == 1:
            predicted_image = predicted_image.squeeze(0)
        if ground_truth_image.dim() == 4 and ground_truth_image.shape[0] == 1:
            ground_truth_image = ground_truth_image.squeeze(0)
        if predicted_image.shape != ground_truth_image.shape:
            raise ValueError("predicted_image and ground_truth_image must have the same shape")
        if isinstance(pixel_weight, torch.Tensor) and predicted_image.dim() == 3 and pixel_weight.dim() == 3 \
                and pixel_weight.shape[0] == 1:
            pixel_weight = pixel_weight.squeeze(0)              # the (1,H,W) weight of a (1,3,H,W) batch, like the images
        if pixel_weight is not None:
            L, terms = self._weighted(predicted_image, ground_truth_image, pixel_weight, clamp_predicted)
        elif predicted_image.dim() == 3:
            L, terms = _L1SSIM.apply(predicted_image, ground_truth_image, self.config.lambda_value, clamp_predicted)
        else:
            per_image = [_L1SSIM.apply(p, g, self.config.lambda_value, clamp_predicted)
                         for p, g in zip(predicted_image.unbind(0), ground_truth_image.unbind(0))]
            L = torch.stack([p[0] for p in per_image]).mean()
            terms = torch.stack([p[1] for p in per_image]).mean(dim=0)
        L1, LD_SSIM = terms[1], terms[2]
        if pointcloud_features is not None and self.config.enable_regularization:
            L = L + self.config.regularization_weight * self._regularization_loss(point_invalid_mask, pointcloud_features)
        return L, L1, LD_SSIM

    def _weighted(self, predicted_image, ground_truth_image, pixel_weight, clamp_predicted):
        """-> (L, terms) of the weighted kernels; every weight is validated before the first launch"""
        if not isinstance(pixel_weight, torch.Tensor):
            raise TypeError("pixel_weight must be a tensor")
        if predicted_image.dim() == 3:
            check_loss_images(predicted_image, ground_truth_image)
            check_pixel_weight(pixel_weight, predicted_image)
            return _L1SSIMWeighted.apply(predicted_image, ground_truth_image, pixel_weight, self.config.lambda_value, clamp_predicted)
        B = predicted_image.shape[0]
        if pixel_weight.dim() == 3 and pixel_weight.shape[0] != B:
            raise ValueError(f"pixel_weight holds {pixel_weight.shape[0]} planes for a batch of {B}")
        if pixel_weight.dim() not in (2, 3):
            raise ValueError(f"pixel_weight must be (H,W) or (B,H,W), got {tuple(pixel_weight.shape)}")
        weights = [pixel_weight] * B if pixel_weight.dim() == 2 else list(pixel_weight.unbind(0))
        for p, g, w in zip(predicted_image.unbind(0), ground_truth_image.unbind(0), weights):
            check_loss_images(p, g)
            check_pixel_weight(w, p)
        per_image = [_L1SSIMWeighted.apply(p, g, w, self.config.lambda_value, clamp_predicted)
                     for p, g, w in zip(predicted_image.unbind(0), ground_truth_image.unbind(0), weights)]
        return torch.stack([p[0] for p in per_image]).mean(), torch.stack([p[1] for p in per_image]).mean(dim=0)

    def _regularization_loss(self, point_invalid_mask, pointcloud_features):
        if pointcloud_features.is_cuda and pointcloud_features.dtype == torch.float32 and pointcloud_features.is_contiguous() \
                and pointcloud_features.dim() == 2 and pointcloud_features.shape[1] == 56:
            return _ScaleRegulariser.apply(pointcloud_features, point_invalid_mask)
        s = pointcloud_features[point_invalid_mask == 0, 4:7]           # LossFunction.py:48-50
        return torch.norm(torch.exp(s), dim=1).mean()
