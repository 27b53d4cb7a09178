"""The scene as a Gaussian mixture, restated in torch on the CPU: the reference the mixture tests judge mixture.py and
k_mixture.hip by.  Everything takes a dtype (float64 for the reference proper, float32 for the error an f32 evaluation of the
same formula has, which sets the density bar).

Two forms of each quantity, which test_mixture_ref_host.py holds against each other:
  log_density / fourier                           the closed whitened forms |S^-1 R^T (x - mu)|^2 and |S R^T k|^2
  log_density_distributions / fourier_covariance  the construction of the project this one is modelled on: covariance
      R S^2 R^T, torch.linalg.cholesky, MultivariateNormal / Categorical / MixtureSameFamily.log_prob, and the literal
      k^T Sigma k with a covariance matrix
and the grid helpers with torch.linspace / torch.fft.fftfreq as that project calls them."""
import math

import torch
from torch.distributions.categorical import Categorical
from torch.distributions.mixture_same_family import MixtureSameFamily
from torch.distributions.multivariate_normal import MultivariateNormal


def make_scene(n, seed, log_scale=(-3.0, -1.0), logit=(-1.0, 1.0)):
    """(point_cloud (n,3), features (n,56), mask (n,) int8 zeros), f32: means N(0,1), quaternions NOT normalised with norms in
    (0.5, 2), log s and opacity logits uniform in the given ranges, the SH columns random (they must not matter)"""
    g = torch.Generator().manual_seed(seed)
    pc = torch.randn(n, 3, generator=g)
    feat = torch.randn(n, 56, generator=g)
    q = torch.randn(n, 4, generator=g)
    norm = 0.5 + 1.5 * torch.rand(n, 1, generator=g)
    feat[:, :4] = q / q.norm(dim=1, keepdim=True) * norm
    feat[:, 4:7] = log_scale[0] + (log_scale[1] - log_scale[0]) * torch.rand(n, 3, generator=g)
    feat[:, 7] = logit[0] + (logit[1] - logit[0]) * torch.rand(n, generator=g)
    return pc.float().contiguous(), feat.float().contiguous(), torch.zeros(n, dtype=torch.int8)


def takes_part(pc, feat, mask=None):
    part = torch.isfinite(pc).all(1) & torch.isfinite(feat[:, :8]).all(1) & (feat[:, :4].double().square().sum(1) > 0)
    return part if mask is None else part & (mask == 0)


def rotation(q_xyzw):
    """the rotation of q / |q|: pytorch3d.transforms.quaternion_to_matrix of the quaternion rolled to wxyz"""
    i, j, k, r = q_xyzw.unbind(-1)
    two_s = 2.0 / (q_xyzw * q_xyzw).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q_xyzw.shape[:-1] + (3, 3))


def parameters(pc, feat, mask=None, dtype=torch.float64):
    """(weights (M,), means (M,3), R (M,3,3), log s (M,3)) of the rows that take part, in dtype"""
    part = takes_part(pc, feat, mask)
    f = feat[part].to(dtype)
    sig = torch.sigmoid(f[:, 7])
    return sig / sig.sum(), pc[part].to(dtype), rotation(f[:, :4]), f[:, 4:7]


def log_density(pc, feat, mask, x, dtype=torch.float64, drop=None, rows=1024):
    """closed whitened form; drop = index (among the rows that take part) of a row to leave out, the rest renormalised"""
    w, mu, R, ls = parameters(pc, feat, mask, dtype)
    if drop is not None:
        keep = torch.arange(w.shape[0]) != drop
        w, mu, R, ls = w[keep] / w[keep].sum(), mu[keep], R[keep], ls[keep]
    if w.shape[0] == 0:
        return torch.full((x.shape[0],), -math.inf, dtype=dtype)
    A = torch.exp(-ls).unsqueeze(-1) * R.transpose(-1, -2)                     # S^-1 R^T
    c = torch.log(w) - ls.sum(1) - 1.5 * math.log(2 * math.pi)
    out = []
    for x_ in x.to(dtype).split(rows):
        d = x_[:, None, :] - mu[None]
        y = torch.einsum("nij,pnj->pni", A, d)
        out.append(torch.logsumexp(c[None] - 0.5 * y.square().sum(-1), dim=1))
    return torch.cat(out)


def covariances(R, ls):
    S = R * torch.exp(ls).unsqueeze(-2)
    return S @ S.transpose(-1, -2)


def log_density_distributions(pc, feat, mask, x, dtype=torch.float64):
    """covariance -> Cholesky -> MultivariateNormal / Categorical / MixtureSameFamily, as define_gmm + sample_gmm do it"""
    w, mu, R, ls = parameters(pc, feat, mask, dtype)
    comp = MultivariateNormal(mu, scale_tril=torch.linalg.cholesky(covariances(R, ls)), validate_args=False)
    return MixtureSameFamily(Categorical(w), comp).log_prob(x.to(dtype))


def phases(pc, feat, mask, k, centre, dtype=torch.float64):
    """(P, M): k . (mu - centre)"""
    _, mu, _, _ = parameters(pc, feat, mask, dtype)
    return k.to(dtype) @ (mu - centre.to(dtype)).T


def fourier(pc, feat, mask, k, centre, dtype=torch.float64, drop=None, rows=1024):
    """sum_i pi_i exp(-1/2 |S R^T k|^2) (cos phi_i - i sin phi_i), complex"""
    w, mu, R, ls = parameters(pc, feat, mask, dtype)
    if drop is not None:
        keep = torch.arange(w.shape[0]) != drop
        w, mu, R, ls = w[keep] / w[keep].sum(), mu[keep], R[keep], ls[keep]
    cdtype = torch.complex128 if dtype == torch.float64 else torch.complex64
    if w.shape[0] == 0:
        return torch.zeros(k.shape[0], dtype=cdtype)
    B = torch.exp(ls).unsqueeze(-1) * R.transpose(-1, -2)                      # S R^T
    m = mu - centre.to(dtype)
    out = []
    for k_ in k.to(dtype).split(rows):
        y = torch.einsum("nij,pj->pni", B, k_)
        e = w[None] * torch.exp(-0.5 * y.square().sum(-1))
        phi = k_ @ m.T
        out.append(torch.complex((e * torch.cos(phi)).sum(1), -(e * torch.sin(phi)).sum(1)))
    return torch.cat(out)


def fourier_covariance(pc, feat, mask, k, centre, dtype=torch.float64):
    """the literal form of transform_gmm_to_fourier1: exp(-i k.(mu - c) - 1/2 k^T Sigma k) with the covariance matrices"""
    w, mu, R, ls = parameters(pc, feat, mask, dtype)
    cov = covariances(R, ls)
    k = k.to(dtype)
    quad = torch.einsum("pi,nij,pj->pn", k, cov, k)
    exponent = -1j * (k @ (mu - centre.to(dtype)).T) - 0.5 * quad
    return (w[None] * torch.exp(exponent)).sum(-1)


def bounding_box(pc, feat, mask=None, n_std=3.0):
    """per axis mean -+ n_std population standard deviations (scipy's norm.fit) of the means, float64 -> (2,3) f32"""
    mu = pc[takes_part(pc, feat, mask)].double()
    mean, std = mu.mean(0), mu.std(0, unbiased=False)
    return torch.stack([mean - n_std * std, mean + n_std * std]).float()


def sample_grid(bbox, G):
    axes = [torch.linspace(bbox[0, a], bbox[1, a], G) for a in range(3)]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)


def frequency_grid(bbox, G, sample_spacing=False, shift=True):
    L = bbox[1] - bbox[0]
    axes = [torch.fft.fftfreq(G, d=(L[a].item() / (G - 1 if sample_spacing else G))) * 2 * torch.pi for a in range(3)]
    k = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)
    return torch.fft.fftshift(k, dim=(0, 1, 2)) if shift else k


def compare(volume_dft, transform):
    diff = (volume_dft - transform).abs().mean()
    num = (volume_dft.real * transform.real + volume_dft.imag * transform.imag).sum()
    den = ((volume_dft.real ** 2 + volume_dft.imag ** 2).sum() * (transform.real ** 2 + transform.imag ** 2).sum()).sqrt()
    return float(diff), float(num / den)


def volume_and_transform(pc, feat, mask, G, bbox, consistent, dtype=torch.float64):
    """(DFT of the normalised sampled density, analytic transform, the sampled density), each (G,G,G); consistent as in
    mixture.compare_volume_to_transform"""
    volume = torch.exp(log_density(pc, feat, mask, sample_grid(bbox, G).reshape(-1, 3), dtype)).reshape(G, G, G)
    dft = torch.fft.fftn(volume / volume.sum())
    if consistent:
        k, centre = frequency_grid(bbox, G, True, False), bbox[0]
    else:
        dft = torch.fft.fftshift(dft, dim=(0, 1, 2))
        k, centre = frequency_grid(bbox, G), (bbox[0] + bbox[1]) / 2.0
    return dft, fourier(pc, feat, mask, k.reshape(-1, 3), centre, dtype).reshape(G, G, G), volume


def compare_volume_to_transform(pc, feat, mask, G, bbox, consistent, dtype=torch.float64):
    """the two numbers of compare_gmm_volume_to_transforms in dtype"""
    dft, analytic, _ = volume_and_transform(pc, feat, mask, G, bbox, consistent, dtype)
    return compare(dft, analytic)
