"""Float64 reference of the row-selective Adam step (FusedAdam.step(rows=...), gs_adam_step_rows): loss_ref.Adam64 applied
to a list of rows per step.  tests/test_sparse_ref_host.py pins it on the CPU (against Adam64 itself and against
torch.optim.SparseAdam), tests/test_gpu_sparse_step.py holds the kernel to it."""
import torch

import loss_ref


class RowAdam64(loss_ref.Adam64):
    """Adam64 on (n_rows, ...) tensors whose step takes the rows to update: the listed rows take Adam64's float64 update, op
    for op, with the global step count t in both bias corrections, and accumulate S; every other row keeps p, m, v and S."""

    def step(self, grad, lr, rows):
        """rows: unique row indices (a tensor or a sequence), any order"""
        b1, b2 = self.betas
        r = torch.as_tensor(rows, dtype=torch.long, device=self.p.device).reshape(-1)
        g = grad.detach().double()[r]
        self.t += 1
        m = self.m[r].lerp_(g, 1 - b1)
        v = self.v[r].mul_(b2).addcmul_(g, g, value=1 - b2)
        bias_correction1 = 1 - b1 ** self.t
        bias_correction2_sqrt = (1 - b2 ** self.t) ** 0.5
        step_size = lr / bias_correction1
        denom = (v.sqrt() / bias_correction2_sqrt).add_(self.eps)
        self.p[r] = self.p[r].addcdiv_(m, denom, value=-step_size)
        self.S[r] = self.S[r].add_((m / denom).abs_(), alpha=step_size)
        self.m[r], self.v[r] = m, v
        return self.p
