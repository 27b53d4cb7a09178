"""CPU: pins tests/sparse_ref.RowAdam64, the float64 reference of the row-selective Adam step, against loss_ref.Adam64 (every
row listed) and against torch.optim.SparseAdam (hybrid-sparse float64 gradients), and the public surface the step needs."""
import numpy as np
import torch

import loss_ref
from sparse_ref import RowAdam64


def _bits(x):
    return x.detach().numpy().view(np.uint8)


def test_every_row_listed_equals_adam64_exactly():
    gen = torch.Generator().manual_seed(1)
    p = torch.randn(37, 56, generator=gen)
    a, b = loss_ref.Adam64(p), RowAdam64(p)
    lr = 1e-3
    for t in range(10):
        g = torch.randn(37, 56, generator=gen) * 3
        a.step(g, lr)
        b.step(g, lr, torch.randperm(37, generator=gen))          # any order: the rows are independent
        lr *= 0.97
    for name in ("p", "m", "v", "S"):
        assert np.array_equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    assert a.t == b.t == 10


def test_matches_sparse_adam_at_tiny_eps():
    """torch.optim.SparseAdam on (1,nnz) indices and (nnz,56) values is the same update except for where eps enters (it adds
    eps to sqrt(v) before the bias correction): at eps = 1e-30 the two agree to rounding.  Lists re-drawn every step, each
    with one listed row whose gradient is all zero (its moments decay and it moves, in both)."""
    gen = torch.Generator().manual_seed(2)
    n, c, eps, lr = 200, 56, 1e-30, 1e-3
    p0 = torch.randn(n, c, generator=gen, dtype=torch.float64)
    ps = p0.clone().requires_grad_(True)
    opt = torch.optim.SparseAdam([ps], lr=lr, betas=(0.9, 0.999), eps=eps)
    ref = RowAdam64(p0, (0.9, 0.999), eps)
    worst = 0.0
    for t in range(25):
        rows = torch.randperm(n, generator=gen)[:40].sort().values
        vals = torch.randn(40, c, generator=gen, dtype=torch.float64)
        vals[t % 40] = 0.0
        ps.grad = torch.sparse_coo_tensor(rows[None], vals, (n, c)).coalesce()
        opt.step()
        dense = torch.zeros(n, c, dtype=torch.float64)
        dense[rows] = vals
        dense[~torch.isin(torch.arange(n), rows)] = 7.0           # what a row outside the list holds is never read
        ref.step(dense, lr, rows)
        worst = max(worst, (ps.detach() - ref.p).abs().max().item())
    print("RowAdam64 against SparseAdam, 25 steps, eps 1e-30: max abs difference", worst)
    assert worst <= 1e-13, worst
    st = opt.state[ps]
    assert (st["exp_avg"] - ref.m).abs().max().item() <= 1e-13 and (st["exp_avg_sq"] - ref.v).abs().max().item() <= 1e-13


def test_rows_never_listed_keep_their_bits():
    gen = torch.Generator().manual_seed(3)
    p = torch.randn(50, 3, generator=gen)
    ref = RowAdam64(p)
    p0 = ref.p.clone()
    never = torch.tensor([0, 7, 49])
    pool = torch.tensor([i for i in range(50) if i not in never.tolist()])
    for t in range(12):
        rows = pool[torch.randperm(pool.numel(), generator=gen)[:10]]
        ref.step(torch.randn(50, 3, generator=gen), 1e-2, rows)
    assert np.array_equal(_bits(ref.p[never]), _bits(p0[never]))
    for name in ("m", "v", "S"):
        assert not getattr(ref, name)[never].any(), name
    assert ref.S[pool].any() and ref.t == 12
    # a listed row's bias correction uses the global step, not the number of times the row was listed
    one = RowAdam64(torch.zeros(2, 1))
    one.step(torch.ones(2, 1), 0.1, [0])
    one.step(torch.ones(2, 1), 0.1, [1])
    b1, b2 = one.betas
    m, v = 1 - b1, 1 - b2
    expect = -(0.1 / (1 - b1 ** 2)) * m / (v ** 0.5 / (1 - b2 ** 2) ** 0.5 + one.eps)
    assert abs(one.p[1].item() - expect) < 1e-15 and one.p[0].item() != one.p[1].item()


def test_the_step_documents_these_semantics():
    """What this file pins is what FusedAdam.step(rows=...) promises in its docstring"""
    from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
    doc = " ".join((FusedAdam.step.__doc__ or "").split())
    for phrase in ("listed rows only", "global step", "not decayed", "SelectiveAdam", "SparseAdam", "eps", "dense step"):
        assert phrase in doc, phrase
