"""CPU: the two routes of tests/mixture_grad_ref.py to the mixture's gradients against each other -- the ten-sum closed forms
that k_mixture_grad.hip implements, and torch autograd through mixture_ref.log_density / mixture_ref.fourier -- in float64 at
small sizes, with a masked row and rows that take no part among them.

Tolerance: both routes are float64 evaluations of the same sums of P x N terms; 1e-11 of the group's largest magnitude is four
orders above what their roundings differ by (measured 1e-15 to 1e-13 relative) and seven below any formula error."""
import math

import pytest
import torch

import mixture_grad_ref as GR
import mixture_ref as R

N, P = 37, 50
CENTRE = torch.tensor([0.1, -0.2, 0.3])


def scene():
    pc, feat, mask = R.make_scene(N, seed=5)
    mask[3] = 1
    pc[7, 1] = math.nan
    feat[11, 5] = math.inf
    feat[19, :4] = 0.0
    return pc, feat, mask


def queries(pc):
    rest = torch.randn(P - 20, 3, generator=torch.Generator().manual_seed(1)) * 2
    return torch.cat([pc[:20].nan_to_num(0.0), rest])


def assert_groups_agree(a, b, part):
    assert set(a) == set(b)
    for name in a:
        scale = float(b[name].abs().max())
        assert scale > 0, name
        assert float((a[name] - b[name]).abs().max()) <= 1e-11 * scale, name
        if name != "x":
            assert bool((a[name][~part] == 0).all()) and bool((b[name][~part] == 0).all()), name


def test_density_closed_form_is_the_autograd_gradient():
    pc, feat, mask = scene()
    part = R.takes_part(pc, feat, mask)
    assert int(part.sum()) == N - 4
    x, g = queries(pc), GR.upstream(P, 1, 3)
    closed = GR.closed_density(pc, feat, mask, x, g, rows=16)
    assert_groups_agree(closed, GR.autograd_density(pc, feat, mask, x, g, rows=7), part)
    assert set(closed) == set(GR.GROUPS) | {"x"}


def test_fourier_closed_form_is_the_autograd_gradient():
    pc, feat, mask = scene()
    k, g = queries(pc), GR.upstream(P, 2, 4)
    closed = GR.closed_fourier(pc, feat, mask, k, CENTRE, g, rows=16)
    assert_groups_agree(closed, GR.autograd_fourier(pc, feat, mask, k, CENTRE, g, rows=7), R.takes_part(pc, feat, mask))


def test_the_quaternion_gradient_is_orthogonal_to_q_and_scales_with_its_inverse_norm():
    pc, feat, mask = scene()
    x, g = queries(pc), GR.upstream(P, 1, 3)
    a = GR.closed_density(pc, feat, mask, x, g)
    part = R.takes_part(pc, feat, mask)
    q = feat[:, :4].double()
    assert float((a["q"][part] * q[part]).sum(1).abs().max()) <= 1e-11 * float(a["q"].abs().max())
    doubled = feat.clone()
    doubled[:, :4] *= 2.0
    b = GR.closed_density(pc, doubled, mask, x, g)
    assert float((b["q"] * 2.0 - a["q"]).abs().max()) <= 1e-11 * float(a["q"].abs().max())


def test_queries_that_contribute_nothing():
    """g = 0 at a NaN or far-away point, and a -inf value: the closed form equals the same call without those queries"""
    pc, feat, mask = scene()
    x, g = queries(pc), GR.upstream(P, 1, 3).reshape(-1)
    x2, g2 = x.double(), g.clone()                  # float64 queries: 1e200 is far enough for log p = -inf in float64 too
    x2[5, 0], g2[5] = math.nan, 0.0
    x2[9], g2[9] = 1e200, 0.0
    x2[12] = 1e200                                  # log p = -inf with g != 0
    keep = torch.ones(P, dtype=torch.bool)
    keep[[5, 9, 12]] = False
    a = GR.closed_density(pc, feat, mask, x2, g2)
    b = GR.closed_density(pc, feat, mask, x2[keep], g2[keep])
    for name in GR.GROUPS:                              # the same terms in torch's own order for another length: to rounding
        assert bool(torch.isfinite(a[name]).all()), name
        assert float((a[name] - b[name]).abs().max()) <= 1e-11 * float(b[name].abs().max()), name
    assert torch.equal(a["x"][keep], b["x"]) and bool((a["x"][~keep] == 0).all())


@pytest.mark.parametrize("columns", [1, 2])
def test_upstream_gradients_are_seeded_and_away_from_zero(columns):
    g = GR.upstream(100, columns, 7)
    assert torch.equal(g, GR.upstream(100, columns, 7)) and g.shape == (100, columns)
    assert float(g.abs().min()) >= 0.5 and float(g.abs().max()) <= 1.5 and bool((g < 0).any()) and bool((g > 0).any())
