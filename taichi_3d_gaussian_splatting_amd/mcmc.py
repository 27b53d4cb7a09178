"""Fixed-budget densification (include/gs_mcmc.h, csrc/k_mcmc.hip) after 3DGS-MCMC (Kheradmand et al., "3D Gaussian Splatting
as Markov Chain Monte Carlo"): train a scene with exactly as many Gaussians as asked for.

  strategy = MCMCStrategy(MCMCConfig(cap_max=1_000_000), scene, optimizer, position_optimizer)
  loss.backward()
  strategy.before_step(iteration)                        # the two L1 regularisers' gradient, added to the features' .grad
  optimizer.step(); position_optimizer.step()
  strategy.after_step(iteration, position_optimizer.lr)  # position noise; every refine_every steps the relocation

There are no clone / split thresholds.  Dead Gaussians (opacity <= min_opacity) are moved onto live ones drawn by opacity, the
set grows by grow_factor per refinement up to cap_max into the scene's free rows (max_num_points_ratio), and the opacity and
scale of a source and its copies are set so that the rendered image does not change.  Every step adds position noise shaped by
each Gaussian's covariance and gated by its opacity; the regularisers make unused Gaussians die.  The rules, to the
parenthesis, are the header's.  Two deviations from the paper: all destinations of a refinement draw their sources in one
round (the paper relocates, then draws again for the added ones), and the Adam moments of the destinations are zeroed like
the sources' (the paper's code zeroes the sources' only).

The three calls -- inject_noise, add_regulariser_grad, relocate -- take anything with the scene's four tensors (point_cloud,
point_cloud_features, point_invalid_mask, point_object_id) and never wait for the host: what they count stays on the device.
There is no fallback path: every call goes through _native.call(), and a CPU tensor is refused.
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _native
from ._native import GsScene

BLOCK = 256                                     # GS_MCMC_BLOCK
N_MAX = 51                                      # GS_MCMC_N_MAX
WEIGHT_ONE = 2 ** 24                            # GS_MCMC_WEIGHT_ONE
STREAM_NOISE, STREAM_RELOCATE = 2, 3            # GS_MCMC_STREAM_*
GATE_K, GATE_X0 = 100.0, 0.995                  # the paper's opacity gate of the noise
COUNTS = ("valid_before", "dead", "alive", "free", "new", "destinations", "sources", "valid_after")      # gs_mcmc_count

_VP, _I32, _I64, _F32, _U32, _U64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_uint32, C.c_uint64


class GsMcmcConfig(C.Structure):
    _fields_ = [("min_opacity_logit", _F32), ("n_max", _I32), ("grow_permille", _I32), ("reserved", _I32), ("cap_max", _I64)]


class GsMcmcPlan(C.Structure):
    _fields_ = [("source_of", _VP), ("dest_row", _VP), ("multiplicity", _VP), ("scratch", _VP), ("counts", _VP), ("n_points", _I64)]

    @classmethod
    def of(cls, plan):
        """plan: an MCMCPlan, whose tensors carry the names of the fields"""
        return cls(n_points=plan.n_points, **{name: _native.ptr(getattr(plan, name)) for name, kind in cls._fields_ if kind is _VP})


ARGTYPES = {
    # (ctx, point_cloud, features, mask, n_points, noise_scale, gate_k, gate_x0, seed, step_index, stream)
    "gs_mcmc_noise": [_VP, _VP, _VP, _VP, _I64, _F32, _F32, _F32, _U64, _U32, _VP],
    # (ctx, features, mask, n_points, lambda_opacity, lambda_scale, upstream, grad_features, value_and_count, stream)
    "gs_mcmc_regulariser": [_VP, _VP, _VP, _I64, _F32, _F32, _VP, _VP, _VP, _VP],
    # (ctx, scene, features_exp_avg, features_exp_avg_sq, point_cloud_exp_avg, point_cloud_exp_avg_sq, config, plan, seed, call_index, stream)
    "gs_mcmc_relocate": [_VP, C.POINTER(GsScene), _VP, _VP, _VP, _VP, C.POINTER(GsMcmcConfig), C.POINTER(GsMcmcPlan), _U64, _U32, _VP],
}
_bound = False


def _bind():
    """argtypes of the entry points, set once on the loaded library (they are not part of _native.SYMBOLS)"""
    global _bound
    if not _bound:
        L = _native.lib()
        for name in list(ARGTYPES) + ["gs_mcmc_scratch_bytes"]:
            if not hasattr(L, name):
                raise _native.NativeLibraryError(f"{_native.LIB_PATH} does not export {name}")
        for name, argtypes in ARGTYPES.items():
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
        L.gs_mcmc_scratch_bytes.argtypes, L.gs_mcmc_scratch_bytes.restype = [_I64], _I64
        _bound = True


def scratch_bytes(n_points: int) -> int:
    _bind()
    return int(_native.lib().gs_mcmc_scratch_bytes(int(n_points)))


def min_opacity_logit(min_opacity: float) -> float:
    """the f32 logit of the smallest opacity that lives, as the library compares it"""
    return float(np.float32(math.log(min_opacity / (1.0 - min_opacity))))


@dataclass
class MCMCConfig:
    """The paper's defaults.  cap_max None: every allocated row of the scene."""
    cap_max: Optional[int] = None
    refine_start: int = 500             # a refinement runs at the iterations i with refine_start < i < refine_stop and
    refine_stop: int = 25_000           # i % refine_every == 0
    refine_every: int = 100
    grow_factor: float = 1.05           # held as per-mille of growth: grow_permille
    min_opacity: float = 0.005
    n_max: int = 51
    noise_lr: float = 5e5
    opacity_reg: float = 0.01
    scale_reg: float = 0.01
    seed: int = 0

    @property
    def grow_permille(self) -> int:
        return int(round((self.grow_factor - 1.0) * 1000.0))

    def check(self):
        if not 1 <= self.n_max <= N_MAX:
            raise ValueError(f"n_max must be in [1, {N_MAX}]")
        if self.grow_permille < 0 or (self.cap_max is not None and self.cap_max < 0):
            raise ValueError("grow_factor must be >= 1 and cap_max >= 0")
        if not 0.0 < self.min_opacity < 1.0:
            raise ValueError("min_opacity must be in (0, 1)")
        if self.refine_every < 1:
            raise ValueError("refine_every must be >= 1")
        if not all(math.isfinite(v) for v in (self.noise_lr, self.opacity_reg, self.scale_reg)):
            raise ValueError("noise_lr, opacity_reg and scale_reg must be finite")

    def is_refinement(self, iteration: int) -> bool:
        return self.refine_start < iteration < self.refine_stop and iteration % self.refine_every == 0


class MCMCPlan:
    """The caller-owned device memory of relocate() for a scene of n_points rows (gs_mcmc_plan)"""

    def __init__(self, n_points: int, device):
        self.n_points = int(n_points)
        for name in ("source_of", "dest_row", "multiplicity"):
            setattr(self, name, torch.zeros(self.n_points, dtype=torch.int32, device=device))
        self.scratch = torch.zeros((scratch_bytes(self.n_points) + 7) // 8, dtype=torch.int64, device=device)
        self.counts = torch.zeros(len(COUNTS), dtype=torch.int32, device=device)


def _scene_tensors(scene):
    pc, ft, mask, obj = scene.point_cloud, scene.point_cloud_features, scene.point_invalid_mask, scene.point_object_id
    for t, what in ((pc, "point_cloud"), (ft, "point_cloud_features"), (mask, "point_invalid_mask"), (obj, "point_object_id")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"fixed-budget densification runs on the GPU: {what} must be a tensor on a cuda/hip device (there is no CPU path)")
    n = pc.shape[0]
    ok = (pc.dtype == torch.float32 and tuple(pc.shape) == (n, 3) and ft.dtype == torch.float32 and tuple(ft.shape) == (n, 56)
          and mask.dtype == torch.int8 and tuple(mask.shape) == (n,) and obj.dtype == torch.int32 and tuple(obj.shape) == (n,)
          and all(t.is_contiguous() and t.device == pc.device for t in (pc, ft, mask, obj)))
    if not ok:
        raise ValueError("a scene is point_cloud (N,3) f32, point_cloud_features (N,56) f32, point_invalid_mask (N) int8 and "
                         "point_object_id (N) int32, contiguous, on one device")
    return pc.detach(), ft.detach(), mask, obj


def _like(t, ref, what):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"fixed-budget densification runs on the GPU: {what} must be a tensor on a cuda/hip device (there is no CPU path)")
    if t.device != ref.device or t.dtype != torch.float32 or t.shape != ref.shape or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 tensor of shape {tuple(ref.shape)} on {ref.device}")
    return t.detach()


def inject_noise(scene, noise_scale: float, step: int, seed: int = 0, gate_k: float = GATE_K, gate_x0: float = GATE_X0):
    """gs_mcmc_noise: x += Sigma z * (gate(opacity) * noise_scale) on every valid row, z ~ N(0, I) from the Philox counter
    (row, step, 2, 0) keyed by seed.  noise_scale = noise_lr * the current position learning rate.  In place, on the current
    stream."""
    _bind()
    pc, ft, mask, _ = _scene_tensors(scene)
    _native.call("gs_mcmc_noise", pc.device, _native.shared_ctx(pc.device), _native.ptr(pc), _native.ptr(ft), _native.ptr(mask), pc.shape[0],
                 float(noise_scale), float(gate_k), float(gate_x0), int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF)


def add_regulariser_grad(scene, opacity_reg: float, scale_reg: float, grad=None, upstream=None, with_grad: bool = True):
    """gs_mcmc_regulariser: opacity_reg * mean sigmoid(logit) + scale_reg * mean exp(log s) over the valid rows; its gradient
    times upstream (a device scalar; None = 1) is ADDED to grad (default: point_cloud_features.grad, which must exist) in
    columns 4..7 of the valid rows.  -> a device tensor of three floats: the opacity term, the scale term, the valid count.
    with_grad=False: the value alone."""
    _bind()
    _, ft, mask, _ = _scene_tensors(scene)
    if with_grad:
        grad = scene.point_cloud_features.grad if grad is None else grad
        if grad is None:
            raise ValueError("point_cloud_features has no .grad to add to: call this after loss.backward(), or pass grad=")
        grad = _like(grad, ft, "grad")
    else:
        grad = None
    if upstream is not None:
        upstream = _like(upstream.reshape(()), torch.empty((), device=ft.device), "upstream")
    out = torch.empty(3, dtype=torch.float32, device=ft.device)
    _native.call("gs_mcmc_regulariser", ft.device, _native.shared_ctx(ft.device), _native.ptr(ft), _native.ptr(mask), ft.shape[0],
                 float(opacity_reg), float(scale_reg), None if upstream is None else upstream.data_ptr(), _native.ptr(grad), out.data_ptr())
    return out


def _moments(optimizer, param, what):
    """(exp_avg, exp_avg_sq) of `param` in a FusedAdam (or anything with .params and .state of that form); (None, None) without"""
    if optimizer is None:
        return None, None
    for p, st in zip(optimizer.params, optimizer.state):
        if p is param:
            return _like(st["exp_avg"], param, f"{what} exp_avg"), _like(st["exp_avg_sq"], param, f"{what} exp_avg_sq")
    raise ValueError(f"the optimizer given for {what} does not hold it")


def relocate(scene, config: MCMCConfig = None, optimizers=(None, None), call_index: int = 0, plan: MCMCPlan = None):
    """gs_mcmc_relocate: dead rows and up to grow_factor's share of free rows become copies of live rows drawn by opacity; the
    opacity and scale of every group are reset so that the image stays, and the Adam moments of its rows are zeroed in
    optimizers = (the features' FusedAdam, the positions' FusedAdam), either of which may be None.  In place, on the current
    stream.  -> plan.counts, int32[8] on the device (COUNTS names them); plan.dest_row / source_of / multiplicity say who went
    where."""
    _bind()
    config = MCMCConfig() if config is None else config
    config.check()
    pc, ft, mask, obj = _scene_tensors(scene)
    n = pc.shape[0]
    if plan is None:
        plan = MCMCPlan(n, pc.device)
    if plan.n_points < n or plan.counts.device != pc.device:
        raise ValueError("the plan is smaller than the scene, or on another device")
    m_f, v_f = _moments(optimizers[0], scene.point_cloud_features, "point_cloud_features")
    m_x, v_x = _moments(optimizers[1], scene.point_cloud, "point_cloud")
    cfg = GsMcmcConfig(min_opacity_logit=min_opacity_logit(config.min_opacity), n_max=config.n_max, grow_permille=config.grow_permille,
                       reserved=0, cap_max=n if config.cap_max is None else int(config.cap_max))
    _native.call("gs_mcmc_relocate", pc.device, _native.shared_ctx(pc.device), GsScene.of(pc, ft, mask, obj), _native.ptr(m_f), _native.ptr(v_f),
                 _native.ptr(m_x), _native.ptr(v_x), cfg, GsMcmcPlan.of(plan), int(config.seed) & (2 ** 64 - 1), int(call_index) & 0xFFFFFFFF)
    return plan.counts


class MCMCStrategy:
    """The strategy around a training step: before_step() between loss.backward() and the optimiser steps, after_step() behind
    them.  history holds (iteration, counts) of every refinement, the counts a clone of the device tensor: nothing here reads
    them on the host."""

    def __init__(self, config: MCMCConfig, scene, optimizer, position_optimizer):
        config.check()
        self.config, self.scene = config, scene
        self.optimizer, self.position_optimizer = optimizer, position_optimizer
        _scene_tensors(scene)
        self.plan = MCMCPlan(scene.point_cloud.shape[0], scene.point_cloud.device)
        self.refinement_calls = 0
        self.last_regulariser = None            # the three floats of the last before_step, on the device
        self.history = []

    def before_step(self, iteration: int):
        self.last_regulariser = add_regulariser_grad(self.scene, self.config.opacity_reg, self.config.scale_reg)

    def after_step(self, iteration: int, position_lr: float):
        inject_noise(self.scene, self.config.noise_lr * float(position_lr), iteration, seed=self.config.seed)
        if self.config.is_refinement(iteration):
            counts = relocate(self.scene, self.config, (self.optimizer, self.position_optimizer), self.refinement_calls, self.plan)
            self.refinement_calls += 1
            self.history.append((iteration, counts.clone()))
