"""The gradients of the scene-as-mixture evaluations, restated in torch on the CPU: the reference the mixture-gradient tests
judge mixture_grad.py and k_mixture_grad.hip by.

Two routes to every gradient, which test_mixture_grad_ref_host.py holds against each other:
  autograd_density / autograd_fourier   torch autograd through mixture_ref.log_density / mixture_ref.fourier in a dtype
      (float64: the reference proper; float32: the error an f32 evaluation of the same formula has, which sets the bars),
      one slice of the queries at a time so that no graph is larger than rows x N pairs
  closed_density / closed_fourier       the ten sums per row (W, m, M or sum A, sum B k, Z) and the step from them to the
      gradients of mu, q, log s and the opacity logit, for the cases too large for an autograd graph
Every gradient comes back as a dict of the groups mu (N,3), q (N,4), log_s (N,3), alpha (N,) and, for the density, x (P,3);
rows that take no part hold zeros."""
import torch

import mixture_ref as R

GROUPS = ("mu", "q", "log_s", "alpha")


def upstream(p, columns, seed):
    """(p, columns) f32: magnitudes uniform in (0.5, 1.5), random signs"""
    g = torch.Generator().manual_seed(seed)
    mag = 0.5 + torch.rand(p, columns, generator=g)
    return (mag * (torch.randint(0, 2, (p, columns), generator=g) * 2 - 1)).float()


def groups_of(grad_pc, grad_feat, grad_x=None):
    out = {"mu": grad_pc, "q": grad_feat[:, :4], "log_s": grad_feat[:, 4:7], "alpha": grad_feat[:, 7]}
    if grad_x is not None:
        out["x"] = grad_x
    return out


def _autograd(fn, pc, feat, queries, g, dtype, rows, want_queries):
    pc_ = pc.to(dtype).clone().requires_grad_(True)
    feat_ = feat.to(dtype).clone().requires_grad_(True)
    grad_q = []
    for q_, g_ in zip(queries.to(dtype).split(rows), g.to(dtype).split(rows)):
        q_ = q_.clone().requires_grad_(want_queries)
        (fn(pc_, feat_, q_) * g_).sum().backward()
        grad_q.append(q_.grad if want_queries else None)
    gp = pc_.grad if pc_.grad is not None else torch.zeros_like(pc_)
    gf = feat_.grad if feat_.grad is not None else torch.zeros_like(feat_)
    return groups_of(gp, gf, torch.cat(grad_q) if want_queries else None)


def autograd_density(pc, feat, mask, x, g, dtype=torch.float64, rows=512):
    """gradients of sum_j g_j log p(x_j) (g (P,) or (P,1)) by autograd through mixture_ref.log_density"""
    return _autograd(lambda p, f, q: R.log_density(p, f, mask, q, dtype), pc, feat, x, g.reshape(-1), dtype, rows, True)


def autograd_fourier(pc, feat, mask, k, centre, g, dtype=torch.float64, rows=512):
    """gradients of sum_j g_j0 Re F(k_j) + g_j1 Im F(k_j) (g (P,2)) by autograd through mixture_ref.fourier"""
    def fn(p, f, q):
        return torch.view_as_real(R.fourier(p, f, mask, q, centre, dtype))
    return _autograd(fn, pc, feat, k, g, dtype, rows, False)


def _rotation_backward(q, G):
    """dL/dq (M,4) from dL/dR (M,3,3) through R of q / |q| (q = xyzw): R = 1 + ts N(q), ts = 2 / |q|^2"""
    x, y, z, w = q.unbind(-1)
    ts = 2.0 / (q * q).sum(-1)
    G = G.reshape(-1, 9)
    g = [G[:, j] for j in range(9)]
    GN = (G * (R.rotation(q).reshape(-1, 9) - torch.eye(3, dtype=q.dtype).reshape(1, 9))).sum(-1)      # ts sum G N
    d = torch.stack([(g[1] + g[3]) * y + (g[2] + g[6]) * z + (g[7] - g[5]) * w - 2 * x * (g[4] + g[8]),
                     (g[1] + g[3]) * x + (g[5] + g[7]) * z + (g[2] - g[6]) * w - 2 * y * (g[0] + g[8]),
                     (g[2] + g[6]) * x + (g[5] + g[7]) * y + (g[3] - g[1]) * w - 2 * z * (g[0] + g[4]),
                     (g[3] - g[1]) * z + (g[2] - g[6]) * y + (g[7] - g[5]) * x], -1)
    return ts[:, None] * d - (ts * GN)[:, None] * q


def _scatter(part, n, groups):
    out = {}
    for name, v in groups.items():
        if name == "x":
            out[name] = v
            continue
        full = torch.zeros((n,) + v.shape[1:], dtype=v.dtype)
        full[part] = v
        out[name] = full
    return out


def closed_density(pc, feat, mask, x, g, dtype=torch.float64, rows=1024):
    """the ten sums W = sum w, m = sum w y, M = sum w y y^T per row, w = g pi N / p, y = S^-1 R^T (x - mu); then
    dL/dmu = R S^-1 m, dL/dlog s_a = M_aa - W, dL/dalpha = (1 - sigma)(W - pi sum g), dL/dR = -R S M S^-1, dL/dx = -sum w A^T y.
    A query with g = 0, a non-finite position or a non-finite log p contributes nothing."""
    part = R.takes_part(pc, feat, mask)
    w, mu, Rm, ls = R.parameters(pc, feat, mask, dtype)
    f = feat[part].to(dtype)
    sig, s = torch.sigmoid(f[:, 7]), torch.exp(ls)
    m_rows = w.shape[0]
    g = g.reshape(-1).to(dtype)
    A = torch.exp(-ls).unsqueeze(-1) * Rm.transpose(-1, -2)
    c = torch.log(w) - ls.sum(1) - 1.5 * torch.log(torch.tensor(2 * torch.pi, dtype=dtype))
    W, m, M = torch.zeros(m_rows, dtype=dtype), torch.zeros(m_rows, 3, dtype=dtype), torch.zeros(m_rows, 3, 3, dtype=dtype)
    g_sum, grad_x = torch.zeros((), dtype=dtype), []
    for x_, g_ in zip(x.to(dtype).split(rows), g.split(rows)):
        ok = torch.isfinite(x_).all(1) & (g_ != 0)
        x_ = torch.where(ok[:, None], x_, torch.zeros((), dtype=dtype))
        y = torch.einsum("nij,pnj->pni", A, x_[:, None, :] - mu[None])
        log_n = c[None] - 0.5 * y.square().sum(-1)
        log_p = torch.logsumexp(log_n, dim=1) if m_rows else torch.full((x_.shape[0],), -torch.inf, dtype=dtype)
        ok = ok & torch.isfinite(log_p)
        wgt = torch.where(ok[:, None], g_[:, None] * torch.exp(log_n - torch.where(ok, log_p, torch.zeros((), dtype=dtype))[:, None]),
                          torch.zeros((), dtype=dtype))
        W += wgt.sum(0)
        m += torch.einsum("pn,pni->ni", wgt, y)
        M += torch.einsum("pn,pni,pnj->nij", wgt, y, y)
        g_sum = g_sum + g_[ok].sum()
        grad_x.append(-torch.einsum("pn,nai,pna->pi", wgt, A, y))
    G = -Rm @ (s.unsqueeze(-1) * M / s.unsqueeze(-2))
    groups = {"mu": torch.einsum("nia,na->ni", Rm, m / s), "q": _rotation_backward(f[:, :4], G),
              "log_s": torch.diagonal(M, dim1=-2, dim2=-1) - W[:, None], "alpha": (1 - sig) * (W - w * g_sum), "x": torch.cat(grad_x)}
    return _scatter(part, pc.shape[0], groups)


def closed_fourier(pc, feat, mask, k, centre, g, dtype=torch.float64, rows=1024):
    """z = S R^T k, E = pi exp(-1/2 |z|^2), phi = k.(mu - c); A = E (g_re cos phi - g_im sin phi), B = -E (g_re sin phi +
    g_im cos phi); per row sum A, sum B k, Z = sum A z z^T; dL/dmu = sum B k, dL/dlog s_a = -Z_aa,
    dL/dalpha = (1 - sigma)(sum A - pi sum_rows sum A), dL/dR = -R S^-1 Z S"""
    part = R.takes_part(pc, feat, mask)
    w, mu, Rm, ls = R.parameters(pc, feat, mask, dtype)
    f = feat[part].to(dtype)
    sig, s = torch.sigmoid(f[:, 7]), torch.exp(ls)
    m_rows = w.shape[0]
    B_ = s.unsqueeze(-1) * Rm.transpose(-1, -2)
    shifted = mu - centre.to(dtype)
    sA, sBk, Z = torch.zeros(m_rows, dtype=dtype), torch.zeros(m_rows, 3, dtype=dtype), torch.zeros(m_rows, 3, 3, dtype=dtype)
    for k_, g_ in zip(k.to(dtype).split(rows), g.to(dtype).split(rows)):
        ok = torch.isfinite(k_).all(1) & (g_ != 0).any(1)
        k_ = torch.where(ok[:, None], k_, torch.zeros((), dtype=dtype))
        g_ = torch.where(ok[:, None], g_, torch.zeros((), dtype=dtype))
        z = torch.einsum("nij,pj->pni", B_, k_)
        E = w[None] * torch.exp(-0.5 * z.square().sum(-1))
        phi = k_ @ shifted.T
        a = E * (g_[:, :1] * torch.cos(phi) - g_[:, 1:] * torch.sin(phi))
        b = -E * (g_[:, :1] * torch.sin(phi) + g_[:, 1:] * torch.cos(phi))
        sA += a.sum(0)
        sBk += torch.einsum("pn,pi->ni", b, k_)
        Z += torch.einsum("pn,pni,pnj->nij", a, z, z)
    G = -Rm @ (Z / s.unsqueeze(-1) * s.unsqueeze(-2))
    groups = {"mu": sBk, "q": _rotation_backward(f[:, :4], G), "log_s": -torch.diagonal(Z, dim1=-2, dim2=-1),
              "alpha": (1 - sig) * (sA - w * sA.sum())}
    return _scatter(part, pc.shape[0], groups)
