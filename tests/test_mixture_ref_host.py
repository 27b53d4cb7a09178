"""CPU: the float64 reference of the mixture tests (tests/mixture_ref.py) against itself -- the closed whitened forms against
the covariance / Cholesky / torch.distributions construction -- the grid helpers of mixture.py against their restatements, and
the consistency that ties the density to the transform through one FFT."""
import functools

import torch

import mixture_ref as R
from taichi_3d_gaussian_splatting_amd import mixture

N, G = 300, 16


@functools.lru_cache(maxsize=None)
def case():
    """N = 300, log s uniform in (-1, -0.3), box = mean -+ 4 std"""
    pc, feat, mask = R.make_scene(N, seed=3, log_scale=(-1.0, -0.3))
    return pc, feat, mask, R.bounding_box(pc, feat, mask, n_std=4.0)


def test_the_two_density_forms_agree_in_float64():
    pc, feat, mask, bbox = case()
    x = torch.cat([R.sample_grid(bbox, G).reshape(-1, 3), pc])
    a, b = R.log_density(pc, feat, mask, x), R.log_density_distributions(pc, feat, mask, x)
    assert a.dtype == torch.float64 and float((a - b).abs().max()) < 1e-10
    pc2, feat2, mask2 = R.make_scene(N, seed=4)                       # the anisotropic scales of the GPU tests too
    x2 = torch.cat([R.sample_grid(bbox, 8).reshape(-1, 3), pc2])
    assert float((R.log_density(pc2, feat2, mask2, x2) - R.log_density_distributions(pc2, feat2, mask2, x2)).abs().max()) < 1e-10


def test_the_two_transform_forms_agree_in_float64():
    pc, feat, mask, bbox = case()
    k = torch.cat([R.frequency_grid(bbox, G).reshape(-1, 3), torch.zeros(1, 3), pc])
    centre = (bbox[0] + bbox[1]) / 2.0
    a, b = R.fourier(pc, feat, mask, k, centre), R.fourier_covariance(pc, feat, mask, k, centre)
    assert a.dtype == torch.complex128 and float((a - b).abs().max()) < 1e-10
    assert abs(complex(a[G ** 3]) - 1.0) < 1e-12                       # F(0) = 1


def test_rows_that_take_no_part_and_the_unnormalised_quaternion():
    pc, feat, mask, _ = case()
    assert int(R.takes_part(pc, feat, mask).sum()) == N
    feat2 = feat.clone()
    feat2[:, :4] *= 4.0                                                # R is the rotation of q / |q|: the length does not matter
    x = pc[:50]
    assert float((R.log_density(pc, feat, mask, x) - R.log_density(pc, feat2, mask, x)).abs().max()) < 1e-10
    rot = R.rotation(feat[:, :4].double())
    assert float((rot @ rot.transpose(-1, -2) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12
    assert float((torch.linalg.det(rot) - 1).abs().max()) < 1e-12
    bad = pc.clone()
    bad[7, 0] = float("nan")
    mask2 = mask.clone()
    mask2[9] = 1
    part = R.takes_part(bad, feat, mask2)
    assert int(part.sum()) == N - 2 and not part[7] and not part[9]
    assert torch.equal(mixture.takes_part((bad, feat, mask2)), part)
    keep = torch.arange(N) != 7
    assert float((R.log_density(bad, feat, mask, x) - R.log_density(pc[keep], feat[keep], mask[keep], x)).abs().max()) < 1e-12


def test_bounding_box_and_grids_equal_their_restatements():
    pc, feat, mask, _ = case()
    mask = mask.clone()
    mask[::7] = 1
    for n_std in (3.0, 4.0):
        assert torch.equal(mixture.bounding_box((pc, feat, mask), n_std), R.bounding_box(pc, feat, mask, n_std))
    bbox = R.bounding_box(pc, feat, mask)
    mu = pc[mask == 0].double()
    assert torch.allclose(bbox.double(), torch.stack([mu.mean(0) - 3 * mu.std(0, unbiased=False), mu.mean(0) + 3 * mu.std(0, unbiased=False)]),
                          atol=1e-6)
    for g in (1 + 1, 16, 35, 96):
        assert torch.equal(mixture.sample_grid(bbox, g), R.sample_grid(bbox, g)), g
        assert torch.equal(mixture.frequency_grid(bbox, g), R.frequency_grid(bbox, g)), g
        assert torch.equal(mixture.frequency_grid(bbox, g, sample_spacing=True, shift=False), R.frequency_grid(bbox, g, True, False)), g
    k = mixture.frequency_grid(bbox, 16)
    assert k.shape == (16, 16, 16, 3) and bool((k[8, 8, 8] == 0).all())          # fftshift puts k = 0 in the middle
    x = mixture.sample_grid(bbox, 16)
    assert torch.equal(x[0, 0, 0], bbox[0]) and torch.equal(x[-1, -1, -1], bbox[1])


def test_compare_is_the_restatement():
    g = torch.Generator().manual_seed(0)
    a = torch.complex(torch.randn(4, 4, 4, generator=g, dtype=torch.float64), torch.randn(4, 4, 4, generator=g, dtype=torch.float64))
    b = a + 0.1 * torch.complex(torch.randn(4, 4, 4, generator=g, dtype=torch.float64), torch.randn(4, 4, 4, generator=g, dtype=torch.float64))
    diff, cosine = mixture.compare(a, b)
    assert (float(diff), float(cosine)) == R.compare(a, b)
    assert abs(float(mixture.compare(a, a)[1]) - 1.0) < 1e-12


def test_the_fft_of_the_sampled_density_is_the_analytic_transform():
    """frequencies from the true spacing L / (G - 1), unshifted, phases relative to the first sample: the DFT of the normalised
    volume is the transform up to aliasing and truncation (measured: 0.999985)"""
    pc, feat, mask, bbox = case()
    diff, cosine = R.compare_volume_to_transform(pc, feat, mask, G, bbox, consistent=True)
    print(f"consistent convention in float64: mean difference {diff:.3e}, cosine {cosine:.6f}")
    assert cosine >= 0.9999
    _, as_written = R.compare_volume_to_transform(pc, feat, mask, G, bbox, consistent=False)
    assert as_written < cosine                                         # the convention as written does not line the two up
