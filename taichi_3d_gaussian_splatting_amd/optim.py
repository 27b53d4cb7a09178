"""FusedAdam -- torch.optim.Adam(params, lr, betas=(0.9, 0.999)) as the reference trainer uses it for the
feature and position tensors (GaussianPointTrainer.py:131-134, 183-184), one HIP launch per tensor
(gs_adam_step) instead of torch's multi-kernel foreach path.  `lr` is a plain attribute so an exponential
decay (GaussianPointTrainer.py:136-137,191-192) is `opt.lr *= rate`.  The library call goes through _native.call().

step(rows=...) is the row-selective form (gs_adam_step_rows, sparse.py): the same update on the rows a backward touched."""
from typing import Iterable, Optional

import torch

from . import _native, sparse
from ._native import ptr as _ptr


class FusedAdam:
    def __init__(self, params: Iterable[torch.Tensor], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
        self.params = list(params)
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous():
                raise TypeError("FusedAdam handles contiguous float32 GPU tensors")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.state = [dict(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p)) for p in self.params]

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    @torch.no_grad()
    def step(self, rows: Optional["sparse.TouchedRows"] = None):
        """Without `rows`: torch.optim.Adam's update of every element.

        With `rows` (rast.last_touched_rows of the backward that produced the gradients): the same update, element for element
        the same arithmetic, on the listed rows only -- torch.optim.Adam restricted to those rows, with the global step count
        in the bias correction (state["step"] advances for every parameter that has a gradient, as in the dense step).  Rows
        not listed keep every bit of the parameter AND of both moments: their moments are not decayed, which is what gsplat's
        SelectiveAdam does, and torch.optim.SparseAdam except for where eps enters (SparseAdam adds it to sqrt(v) before the
        bias correction, this adds it after, as Adam does).  Gradient rows outside the list are ignored, whatever they hold.
        Every parameter with a gradient must have rows.n_points rows (ValueError otherwise).  The list describes ONE backward: a
        caller who accumulates several backwards into one .grad before stepping uses the dense step."""
        if rows is not None:
            for p in self.params:
                if p.grad is not None and (p.dim() < 1 or p.shape[0] != rows.n_points):
                    raise ValueError(f"step(rows=...): a parameter of shape {tuple(p.shape)} does not have the list's {rows.n_points} rows")
        for p, st in zip(self.params, self.state):
            if p.grad is None:
                continue
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            st["step"] += 1
            if rows is not None:
                sparse.adam_step_rows(p, g, st["exp_avg"], st["exp_avg_sq"], rows, self.lr, self.betas[0], self.betas[1], self.eps, st["step"])
                continue
            _native.call("gs_adam_step", p.device, _native.shared_ctx(p.device), _ptr(p), _ptr(g),
                         _ptr(st["exp_avg"]), _ptr(st["exp_avg_sq"]), p.numel(), self.lr, self.betas[0], self.betas[1], self.eps,
                         st["step"])
