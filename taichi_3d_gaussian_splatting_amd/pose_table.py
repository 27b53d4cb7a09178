"""Per-view camera pose corrections (include/gs_pose_table.h, csrc/k_posetable.hip): six learnable floats per training view
-- a rotation vector and a translation in the camera's own frame -- composed on the right of the dataset's pose in front of the
rasteriser and trained with the scene from the rasteriser's pose gradients: the "pose_opt" of gsplat, the camera optimiser of
BARF and nerfstudio.  Three launches per step and no host synchronisation: compose, its backward, one Adam step.

  table = PoseTable(len(train_dataset), device, PoseRefinementConfig(num_iterations=30_000))
  q, t = compose(q_base, t_base, table.row(view))                        # (K,4), (K,3): all object rows take the view's row
  image, _, _ = rasteriser(input with q, t); loss.backward()              # row.grad lands in row `view` of table.grad
  optimizer.step(); position_optimizer.step(); table.step(view, iteration)

  q, t, delta = refine_pose(rasteriser, input, target, steps=50)          # localisation of one view against a frozen scene

A correction is delta = (w, u): q' = q (x) dq(w), t' = t + R(q) u, i.e. T' = T * D(delta).  Scene and poses are determined only
up to a common rigid motion: what a trained table means is the relative pose between views, not a row on
its own.

There is no fallback path: every call goes through _native.call(), and a CPU tensor is refused.
"""
import ctypes as C
import json
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native

DELTA_FLOATS = 6                                # GS_POSE_DELTA_FLOATS
THREADS = 256                                   # GS_POSE_THREADS
SERIES_S = 1e-8                                 # GS_POSE_SERIES_S
MAX_VIEWS = 2 ** 24                             # GS_POSE_MAX_VIEWS
MAX_OBJECTS = 64                                # GS_POSE_MAX_OBJECTS

_VP, _I32, _F32 = C.c_void_p, C.c_int32, C.c_float
ARGTYPES = {
    # (ctx, delta, q_base, t_base, V, K, q_out, t_out, stream)
    "gs_pose_compose": [_VP, _VP, _VP, _VP, _I32, _I32, _VP, _VP, _VP],
    # (ctx, delta, q_base, grad_q, grad_t, V, K, reg, grad_delta, stream)
    "gs_pose_compose_backward": [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _F32, _VP, _VP],
}
_bound = False


def _bind():
    """argtypes of the entry points, set once on the loaded library (they are not part of _native.SYMBOLS)"""
    global _bound
    if not _bound:
        L = _native.lib()
        for name, argtypes in ARGTYPES.items():
            if not hasattr(L, name):
                raise _native.NativeLibraryError(f"{_native.LIB_PATH} does not export {name}")
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
        _bound = True


# ---- validation: reads no data, launches nothing ----------------------------------------------------------------------------
def _check_tensor(t, what, shape, like=None):
    """type, dtype, shape (a tuple, or a function of the tensor that raises), device, contiguity: in this order"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a tensor")
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {t.dtype}")
    if callable(shape):
        shape(t)
    elif tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be ({','.join(str(n) for n in shape)}), got {tuple(t.shape)}")
    if like is None:
        if not t.is_cuda:
            raise ValueError(f"pose corrections run on the GPU: {what} must be on a cuda/hip device (there is no CPU path)")
    elif t.device != like.device:
        raise ValueError(f"{what} is on {t.device}, q_base on {like.device}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def check_poses(q_base, t_base) -> Tuple[int, int]:
    """Raise unless q_base is a contiguous float32 (V,K,4) tensor on a GPU and t_base the (V,K,3) one beside it.  -> (V, K)"""
    V, K = _check_q(q_base)
    _check_tensor(t_base, "t_base", (V, K, 3), q_base)
    return V, K


def _check_q(q_base) -> Tuple[int, int]:
    def shape(q):
        if q.dim() != 3 or q.shape[2] != 4:
            raise ValueError(f"q_base must be (V,K,4), xyzw, got {tuple(q.shape)}")
        if q.shape[0] > MAX_VIEWS or q.shape[1] > MAX_OBJECTS:
            raise ValueError(f"q_base has more than {MAX_VIEWS} views or {MAX_OBJECTS} object rows")
    _check_tensor(q_base, "q_base", shape)
    return int(q_base.shape[0]), int(q_base.shape[1])


def check_delta(delta, q_base, what="delta"):
    """Raise unless `delta` is a contiguous float32 (V,6) tensor, (rotation vector | translation) per view, on q_base's device"""
    _check_tensor(delta, what, (int(q_base.shape[0]), DELTA_FLOATS), q_base)


# ---- the two calls ------------------------------------------------------------------------------------------------------
def compose_forward(q_base, t_base, delta, q_out=None, t_out=None):
    """gs_pose_compose, no autograd: (V,K,4), (V,K,3) base poses and (V,6) corrections -> the corrected (q, t), same shapes.
    q_out, t_out: where to write instead (q_base and t_base themselves for in place)."""
    V, K = check_poses(q_base, t_base)
    check_delta(delta, q_base)
    if q_out is None:
        q_out = torch.empty_like(q_base)
    if t_out is None:
        t_out = torch.empty_like(t_base)
    check_poses(q_out, t_out)
    if q_out.shape != q_base.shape or q_out.device != q_base.device:
        raise ValueError("q_out and t_out must have the shapes and the device of q_base and t_base")
    _bind()
    _native.call("gs_pose_compose", q_base.device, _native.shared_ctx(q_base.device), delta.data_ptr(), q_base.data_ptr(), t_base.data_ptr(),
                 V, K, q_out.data_ptr(), t_out.data_ptr())
    return q_out, t_out


def compose_backward(q_base, delta, grad_q, grad_t, reg: float = 0.0, grad_delta=None):
    """gs_pose_compose_backward, no autograd: -> grad_delta (V,6) = d/d delta of the composed poses against (grad_q, grad_t),
    plus reg * delta.  Every element is written, not added; grad_delta: a contiguous (V,6) tensor to write into."""
    V, K = _check_q(q_base)
    check_delta(delta, q_base)
    _check_tensor(grad_q, "grad_q", (V, K, 4), q_base)
    _check_tensor(grad_t, "grad_t", (V, K, 3), q_base)
    if not math.isfinite(float(reg)):
        raise ValueError("reg must be finite")
    if grad_delta is None:
        grad_delta = torch.empty_like(delta)
    else:
        check_delta(grad_delta, q_base, "grad_delta")
    _bind()
    _native.call("gs_pose_compose_backward", q_base.device, _native.shared_ctx(q_base.device), delta.data_ptr(), q_base.data_ptr(),
                 grad_q.data_ptr(), grad_t.data_ptr(), V, K, float(reg), grad_delta.data_ptr())
    return grad_delta


class _Compose(torch.autograd.Function):
    """compose() as an autograd node; base poses are data and get no gradient.  A delta that names a `grad_out` tensor
    (PoseTable.row sets it, and sets the row's .grad to the same memory) has its gradient WRITTEN there by the backward's own
    launch, with the row's `reg` added, and autograd is handed nothing for it.  Such a row feeds one compose() per backward.
    Any other delta gets its gradient the usual way, accumulated into .grad."""

    @staticmethod
    def forward(ctx, q_base, t_base, delta, grad_out, reg):
        q, t = compose_forward(q_base, t_base, delta.detach())
        ctx.save_for_backward(q_base, delta)
        ctx.grad_out, ctx.reg = grad_out, reg
        return q, t

    @staticmethod
    def backward(ctx, grad_q, grad_t):
        q_base, delta = ctx.saved_tensors
        if not ctx.needs_input_grad[2]:
            return None, None, None, None, None
        grad_q = torch.zeros_like(q_base) if grad_q is None else grad_q.to(torch.float32).contiguous()
        grad_t = torch.zeros_like(q_base[..., :3]).contiguous() if grad_t is None else grad_t.to(torch.float32).contiguous()
        direct = ctx.grad_out is not None
        grad_delta = compose_backward(q_base, delta.detach(), grad_q, grad_t, ctx.reg, grad_delta=ctx.grad_out if direct else None)
        return None, None, (None if direct else grad_delta), None, None


def compose(q_base, t_base, delta, reg: Optional[float] = None):
    """-> the corrected (q, t) of base poses under `delta`; differentiable in delta only.  (V,K,4), (V,K,3) and (V,6); or one
    view: (K,4), (K,3) and (6,) -- what the rasteriser takes, and what PoseTable.row hands out.  reg: the weight of the L2 pull
    (reg * delta is added to delta's gradient); None: the row's own (PoseTable.row) or 0."""
    single = isinstance(q_base, torch.Tensor) and q_base.dim() == 2
    grad_out = getattr(delta, "grad_out", None)
    if reg is None:
        reg = float(getattr(delta, "reg", 0.0))
    if single:
        if not isinstance(t_base, torch.Tensor) or not isinstance(delta, torch.Tensor) or t_base.dim() != 2 or delta.dim() != 1:
            raise ValueError("one view is q_base (K,4), t_base (K,3) and delta (6,)")
        q3, t3, d2 = q_base.detach().unsqueeze(0), t_base.detach().unsqueeze(0), delta.unsqueeze(0)
        g2 = None if grad_out is None else grad_out.unsqueeze(0)
    else:
        q3, t3, d2, g2 = q_base.detach(), t_base.detach(), delta, grad_out
    check_poses(q3, t3)
    check_delta(d2, q3)
    if g2 is not None:
        check_delta(g2, q3, "grad_out")
    q, t = _Compose.apply(q3, t3, d2, g2, float(reg))
    return (q[0], t[0]) if single else (q, t)


# ---- the same on the host, float64 --------------------------------------------------------------------------------------
def _rotation_f64(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def correction_matrix(delta) -> np.ndarray:
    """-> the 4x4 float64 D(delta) = [exp(w^) | u] of six numbers (Rodrigues' formula, its series below GS_POSE_SERIES_S)"""
    d = np.asarray(delta, dtype=np.float64).reshape(DELTA_FLOATS)
    w, s = d[:3], float(d[:3] @ d[:3])
    Wx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if s >= SERIES_S:
        th = math.sqrt(s)
        a, b = math.sin(th) / th, (1.0 - math.cos(th)) / s
    else:
        a, b = 1.0 - s / 6.0, 0.5 - s / 24.0
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + a * Wx + b * (Wx @ Wx)
    D[:3, 3] = d[3:]
    return D


# ---- the table of a training set ----------------------------------------------------------------------------------------
@dataclass
class PoseRefinementConfig:
    """lr falls exponentially from lr at start_iteration to lr_final at num_iterations.  num_iterations None: the trainer fills
    in its own.  Before start_iteration the trainer passes the dataset's poses as they are.  reg: the weight of the L2 pull to
    the dataset's pose (reg * delta joins the gradient).  eps is FusedAdam's."""
    lr: float = 1e-3
    lr_final: float = 1e-4
    num_iterations: Optional[int] = None
    start_iteration: int = 0
    reg: float = 1e-6
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8

    def check(self):
        if not (math.isfinite(self.lr) and math.isfinite(self.lr_final) and self.lr > 0.0 and self.lr_final > 0.0):
            raise ValueError("lr and lr_final must be finite and > 0")
        if self.num_iterations is not None and self.num_iterations < 1:
            raise ValueError("num_iterations must be >= 1")
        if int(self.start_iteration) != self.start_iteration or self.start_iteration < 0:
            raise ValueError("start_iteration must be an integer >= 0")
        if not (math.isfinite(self.reg) and self.reg >= 0.0):
            raise ValueError("reg must be finite and >= 0")
        if not (0.0 <= self.betas[0] < 1.0 and 0.0 <= self.betas[1] < 1.0 and self.eps > 0.0):
            raise ValueError("betas must be in [0, 1) and eps > 0")

    def lr_at(self, iteration: int) -> float:
        """exp((1 - t) log lr + t log lr_final), t = (iteration - start_iteration) / (num_iterations - start_iteration) clipped
        to [0, 1]"""
        if self.num_iterations is None:
            return float(self.lr)
        span = max(float(self.num_iterations) - float(self.start_iteration), 1.0)
        t = min(max((float(iteration) - float(self.start_iteration)) / span, 0.0), 1.0)
        return float(math.exp((1.0 - t) * math.log(self.lr) + t * math.log(self.lr_final)))


class PoseTable:
    """One correction per training view: delta, grad, exp_avg and exp_avg_sq are (V,6) float32 on the device, steps the
    host-side Adam step count of every row.  A new table is all zeros: the dataset's poses, bit for bit."""

    def __init__(self, num_views: int, device, config: Optional[PoseRefinementConfig] = None):
        self.config = PoseRefinementConfig() if config is None else config
        self.config.check()
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("pose corrections run on the GPU: the table must be on a cuda/hip device (there is no CPU path)")
        if not 1 <= num_views <= MAX_VIEWS:
            raise ValueError(f"num_views must be in [1, {MAX_VIEWS}]")
        self.num_views = int(num_views)
        self.delta = torch.zeros(self.num_views, DELTA_FLOATS, dtype=torch.float32, device=device)
        self.grad = torch.zeros_like(self.delta)
        self.exp_avg = torch.zeros_like(self.delta)
        self.exp_avg_sq = torch.zeros_like(self.delta)
        self.steps: List[int] = [0] * self.num_views

    @property
    def device(self):
        return self.delta.device

    def _view(self, v: int) -> int:
        v = int(v)
        if not 0 <= v < self.num_views:
            raise IndexError(f"view {v} is not in [0, {self.num_views})")
        return v

    def row(self, v: int):
        """-> the (6,) correction of view v: a leaf that shares the table's memory and requires grad.  Its .grad IS row v of
        self.grad, and compose()'s backward writes (not adds) the gradient there, config.reg * delta included (row.grad_out,
        row.reg): one compose() per backward."""
        v = self._view(v)
        row = self.delta[v].detach().requires_grad_(True)
        row.grad = row.grad_out = self.grad[v]
        row.reg = float(self.config.reg)
        return row

    def step(self, v: int, iteration: int):
        """One Adam step (gs_adam_step, as FusedAdam.step) on row v alone, with the gradient in row v of self.grad, the row's
        own step count and config.lr_at(iteration).  No other row, and no moment of another row, moves."""
        v = self._view(v)
        self.steps[v] += 1
        dev = self.delta.device
        with torch.no_grad():
            _native.call("gs_adam_step", dev, _native.shared_ctx(dev), self.delta[v].data_ptr(), self.grad[v].data_ptr(),
                         self.exp_avg[v].data_ptr(), self.exp_avg_sq[v].data_ptr(), DELTA_FLOATS, self.config.lr_at(iteration),
                         float(self.config.betas[0]), float(self.config.betas[1]), float(self.config.eps), self.steps[v])

    def corrected(self, q_base, t_base):
        """-> the corrected (q, t) of every view in one launch, no autograd: q_base (V,K,4) or (V,4), t_base (V,K,3) or (V,3)"""
        flat = isinstance(q_base, torch.Tensor) and q_base.dim() == 2
        if flat:
            q_base, t_base = q_base.unsqueeze(1), t_base.unsqueeze(1)
        with torch.no_grad():
            q, t = compose_forward(q_base.detach().contiguous(), t_base.detach().contiguous(), self.delta)
        return (q[:, 0], t[:, 0]) if flat else (q, t)

    def save(self, path: str, image_paths: Sequence[str]):
        """A .pt of the table and the image paths its rows belong to (row v is image_paths[v])"""
        image_paths = [str(p) for p in image_paths]
        if len(image_paths) != self.num_views:
            raise ValueError(f"{len(image_paths)} image paths for a table of {self.num_views} views")
        torch.save(dict(delta=self.delta.cpu(), exp_avg=self.exp_avg.cpu(), exp_avg_sq=self.exp_avg_sq.cpu(), steps=list(self.steps),
                        image_paths=image_paths), path)

    @classmethod
    def load(cls, path: str, device="cuda", config: Optional[PoseRefinementConfig] = None):
        """-> (table, image_paths) of a file save() wrote"""
        data = read_file(path)
        table = cls(data["delta"].shape[0], device, config)
        table.delta.copy_(data["delta"])
        table.exp_avg.copy_(data["exp_avg"])
        table.exp_avg_sq.copy_(data["exp_avg_sq"])
        table.steps = [int(s) for s in data["steps"]]
        return table, list(data["image_paths"])

    def by_image_path(self, image_paths: Sequence[str]) -> dict:
        """{image path: its (6,) correction}, views of the table"""
        return {str(p): self.delta[v] for v, p in enumerate(image_paths)}


def read_file(path: str) -> dict:
    """The dict of a file PoseTable.save() wrote, on the host, checked"""
    data = torch.load(path, map_location="cpu")
    delta = data["delta"]
    if delta.dim() != 2 or delta.shape[1] != DELTA_FLOATS or delta.dtype != torch.float32:
        raise ValueError(f"{path}: delta must be (V,{DELTA_FLOATS}) float32")
    if len(data["image_paths"]) != delta.shape[0]:
        raise ValueError(f"{path}: {len(data['image_paths'])} image paths for {delta.shape[0]} rows")
    return data


def corrected_matrices(table_file: str, records: Sequence[dict]) -> List[Optional[np.ndarray]]:
    """For every dataset record: its 4x4 float64 T_pointcloud_camera * D(delta) when its image_path is in the table file, else
    None.  Composed on the host in float64."""
    data = read_file(table_file)
    rows = {str(p): data["delta"][v].numpy().astype(np.float64) for v, p in enumerate(data["image_paths"])}
    out = []
    for record in records:
        delta = rows.get(str(record["image_path"]))
        out.append(None if delta is None else np.asarray(record["T_pointcloud_camera"], dtype=np.float64).reshape(4, 4) @ correction_matrix(delta))
    return out


def write_dataset(table_file: str, src_json: str, dst_json: str) -> int:
    """Writes dst_json: the dataset src_json with the T_pointcloud_camera of every view whose image_path is in the table file
    replaced by the corrected pose, composed on the host in float64; every other field and view as it is.  A refined capture
    can then be handed to any other tool.  -> the number of views corrected"""
    with open(src_json) as fh:
        records = json.load(fh)
    n = 0
    for record, T in zip(records, corrected_matrices(table_file, records)):
        if T is not None:
            record["T_pointcloud_camera"] = T.tolist()
            n += 1
    with open(dst_json, "w") as fh:
        json.dump(records, fh)
    return n


# ---- one view against a frozen scene ------------------------------------------------------------------------------------
def refine_pose(rasterisation, rasterisation_input, target, steps: int, lr: float = 1e-3, pixel_weight=None, lr_final: Optional[float] = None,
                loss_function=None):
    """Test-time alignment (localisation) of one view against a FROZEN scene: `steps` Adam steps on the six floats of a
    correction to rasterisation_input's pose, against `target` ((3,H,W) float32 on the device), under the L1 + SSIM loss
    (loss_function: a LossFunction; None: the default one without the scale regulariser) with an optional per-pixel weight.
    Only the pose requires grad: the backward takes its pose-only path and touches neither the hook nor the controller's
    accumulators, and rasterisation.last_touched_rows stays what it was.  lr falls exponentially to lr_final (None: lr / 10).
    -> (q (K,4), t (K,3), delta (6,)): the corrected pose and the six floats, detached."""
    import dataclasses
    from .LossFunction import LossFunction
    if steps < 0:
        raise ValueError("steps must be >= 0")
    if loss_function is None:
        loss_function = LossFunction(LossFunction.LossFunctionConfig(enable_regularization=False))
    inp = rasterisation_input
    q_base = inp.q_pointcloud_camera.detach().to(torch.float32).contiguous()
    t_base = inp.t_pointcloud_camera.detach().to(torch.float32).contiguous()
    config = PoseRefinementConfig(lr=lr, lr_final=lr / 10.0 if lr_final is None else lr_final, num_iterations=max(int(steps), 1), reg=0.0)
    table = PoseTable(1, q_base.device, config)
    touched = getattr(rasterisation, "last_touched_rows", None)
    frozen = dataclasses.replace(inp, point_cloud=inp.point_cloud.detach(), point_cloud_features=inp.point_cloud_features.detach())
    for step in range(int(steps)):
        q, t = compose(q_base, t_base, table.row(0))
        image = rasterisation(dataclasses.replace(frozen, q_pointcloud_camera=q, t_pointcloud_camera=t))[0]
        loss = loss_function(image.permute(2, 0, 1), target, clamp_predicted=True, pixel_weight=pixel_weight)[0]
        loss.backward()
        table.step(0, step)
    if hasattr(rasterisation, "last_touched_rows"):
        rasterisation.last_touched_rows = touched
    q, t = table.corrected(q_base.unsqueeze(0), t_base.unsqueeze(0))
    return q[0], t[0], table.delta[0].detach().clone()
