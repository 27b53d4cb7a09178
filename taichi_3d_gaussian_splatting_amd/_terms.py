"""What the scalar loss terms on the rendered depth share (depth.py, geometry.py): the check of a plane, the one autograd node
behind depth_loss, normal_loss and depth_smoothness, and the shape of a term the trainer sums (TrainerTerm).  A new term on the
rendered depth needs its two library calls, a *_flags() wrapper that ends in depth_term(), and a TrainerTerm beside them."""
import torch

MAX_PIXELS = 2 ** 31 - 2048                     # GS_APPEARANCE_MAX_PIXELS: a pixel index and its block's end fit int32


def check_plane(plane, what="depth", like=None, device=True):
    """Raise unless `plane` is a contiguous float32 (H,W) tensor on a GPU (of like's shape and device, when given).
    device=False: dtype, shape and strides only"""
    if not isinstance(plane, torch.Tensor):
        raise TypeError(f"{what} must be a tensor")
    if plane.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {plane.dtype}")
    if plane.dim() != 2 or plane.shape[0] < 1 or plane.shape[1] < 1:
        raise ValueError(f"{what} must be (H,W) with H, W >= 1, got {tuple(plane.shape)}")
    if plane.shape[0] * plane.shape[1] > MAX_PIXELS:
        raise ValueError(f"{what} has more than {MAX_PIXELS} pixels")
    if like is not None and plane.shape != like.shape:
        raise ValueError(f"{what} must have the depth's shape {tuple(like.shape)}, got {tuple(plane.shape)}")
    if not plane.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    if not device:
        return
    if not plane.is_cuda:
        raise ValueError(f"depth supervision runs on the GPU: {what} must be on a cuda/hip device (there is no CPU path)")
    if like is not None and plane.device != like.device:
        raise ValueError(f"{what} is on {plane.device}, the depth on {like.device}")


def upstream_of(grad_loss):
    """the gradient of a scalar loss as the backward calls take it: one float32 on the device"""
    return grad_loss.detach().to(torch.float32).reshape(1).contiguous()


def check_upstream(upstream, depth):
    if upstream is not None and (upstream.dtype != torch.float32 or upstream.numel() != 1 or upstream.device != depth.device):
        raise ValueError("upstream must be one float32 on the depth's device")


class _DepthTerm(torch.autograd.Function):
    """terms = forward(depth, **kwargs) and grad_depth = backward(depth, **kwargs, terms=, upstream=): differentiable in the depth
    only.  `tensors` are the tensors among kwargs (a None is an absent optional plane), saved as autograd wants its inputs saved"""

    @staticmethod
    def forward(ctx, depth, call, *tensors):
        forward, backward, kwargs = ctx.call = call
        terms = forward(depth.detach(), **kwargs)
        ctx.save_for_backward(depth, terms, *tensors)
        ctx.mark_non_differentiable(terms)
        return terms[0], terms

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms):
        saved = ctx.saved_tensors
        depth, terms = saved[:2]
        nothing = (None,) * len(saved)                      # (as many as forward() has inputs: depth, call, the tensors)
        if not ctx.needs_input_grad[0] or grad_loss is None:
            return nothing
        _, backward, kwargs = ctx.call
        return (backward(depth.detach(), **kwargs, terms=terms, upstream=upstream_of(grad_loss)),) + nothing[1:]


def depth_term(depth, forward, backward, tensors: dict, scalars: dict):
    """-> the scalar terms[0] of forward(depth, **tensors, **scalars), differentiable in `depth` through backward(); its `.terms`
    is the whole tensor the forward wrote.  The caller has checked the arguments."""
    loss, terms = _DepthTerm.apply(depth, (forward, backward, {**tensors, **scalars}), *tensors.values())
    loss.terms = terms
    return loss


def check_depth_is_rendered(config, who: str, why: str):
    """what every term on the rendered depth needs of a TrainConfig"""
    if not config.targets_on_device:
        raise ValueError(f"{who} needs targets_on_device=True: {why}")
    if config.rasterisation_config.rgb_only:
        raise ValueError(f"{who} cannot be combined with rasterisation_config.rgb_only=True: no depth is rendered")


class TrainerTerm:
    """An extra loss term of GaussianPointCloudTrainer on the rendered depth: the trainer adds weight_at(iteration) * value(...)
    to the loss from start_iteration on, logs "train/<name> loss" and, over the validation views that have one,
    "val/<name>_loss".  weight_at(iteration) -> float is the term's own.  A term that reads the dataset keeps its resident stores in
    `stores`."""
    name = ""
    start_iteration = 0

    def __init__(self):
        self.stores = dict(train=None, val=None)

    def load(self, train_dataset, val_dataset, device):
        """make resident what the term reads of the two datasets; called once, after every argument has been checked"""

    def load_stores(self, store, train_dataset, val_dataset, device, who: str, **kwargs):
        """`stores` of a targets.ResidentStore class: every training record must have an entry, a validation record may"""
        try:
            self.stores["train"] = store.from_dataset(train_dataset, device, **kwargs)
        except ValueError as e:
            raise ValueError(f"{who}: every training record needs a {store.column} ({e})") from e
        self.stores["val"] = store.from_dataset(val_dataset, device, require_all=False, **kwargs)

    def value(self, split: str, view: int, downsample_factor: int, image_depth, image_gt, camera_info, pixel_weight):
        """-> the term of one view of the split ("train" | "val") as depth_term() returns it, or None where the view has none"""
        raise NotImplementedError

    def train_scalars(self, terms):
        """-> [(tag, value)] to log of the `.terms` of a value, read by the host once"""
        return [(f"train/{self.name} loss", terms[0])]
