"""CPU: tests/mcmc_ref.py, the restatement of include/gs_mcmc.h, against itself and against exact arithmetic."""
import decimal
import math

import numpy as np
import pytest

import mcmc_ref

OPACITIES = [0.006, 0.01, 0.05, 0.2, 0.5, 0.8, 0.95, 0.999, 1.0 - 2.0 ** -20, 1.0 - 2.0 ** -24]
GROUPS = [2, 3, 8, 20, 35, 51]


@pytest.mark.parametrize("M", GROUPS)
def test_relocated_opacity_composes_back(M):
    """M Gaussians of opacity p on one spot are as opaque as the one of opacity o: 1 - (1 - p)^M = o"""
    for o in OPACITIES:
        p = 1.0 - math.pow(1.0 - o, 1.0 / M)
        if mcmc_ref.P_MIN <= p <= mcmc_ref.P_MAX:                  # (outside, the clamp decides)
            assert abs((1.0 - (1.0 - p) ** M) - o) <= 1e-12, (o, M)
    assert mcmc_ref.clamp_p(0.0) == 0.005 and mcmc_ref.clamp_p(1.0) == 1.0 - 2.0 ** -24 and mcmc_ref.clamp_p(0.3) == 0.3


def _double_sum_exact(p, M, digits=60):
    decimal.getcontext().prec = digits
    p = decimal.Decimal(p)
    d = decimal.Decimal(0)
    for i in range(1, M + 1):
        for k in range(i):
            term = decimal.Decimal(math.comb(i - 1, k)) * p ** (k + 1) / decimal.Decimal(k + 1).sqrt()
            d = d - term if k & 1 else d + term
    return d


@pytest.mark.parametrize("M", GROUPS)
def test_double_sum_in_float64_against_60_digits(M):
    """the alternating sum with binomials up to C(50,25) loses nothing that an f32 result would see"""
    worst = 0.0
    for o in OPACITIES:
        p = mcmc_ref.clamp_p(1.0 - math.pow(1.0 - o, 1.0 / M))
        exact = _double_sum_exact(p, M)
        got = mcmc_ref.double_sum(p, M)
        assert got > 0
        worst = max(worst, float(abs(decimal.Decimal(got) - exact) / exact))
    assert worst <= 8e-13, worst


def test_scale_shrinks_and_one_copy_changes_nothing_but_the_clamp():
    logit, ls, (o, p, d) = mcmc_ref.relocated(np.float32(1.5), np.float32([-3.0, -2.5, -4.0]), 3, 51)
    assert p < o and logit < 1.5 and (ls < [-3.0, -2.5, -4.0]).all()
    # n_max = 1: M = 1, p = o, d = o: the row keeps its opacity and scale
    logit, ls, (o, p, d) = mcmc_ref.relocated(np.float32(1.5), np.float32([-3.0, -2.5, -4.0]), 7, 1)
    assert p == o and d == o and abs(logit - 1.5) < 1e-6 and (ls == [-3.0, -2.5, -4.0]).all()


def test_weights_prefix_and_draws_in_integers():
    rng = np.random.default_rng(0)
    n = 700
    ft = np.zeros((n, 56), np.float32)
    ft[:, 7] = rng.normal(0.0, 4.0, n).astype(np.float32)
    ft[5, 7], ft[6, 7], ft[7, 7], ft[8, 7] = np.nan, 30.0, -30.0, mcmc_ref.min_opacity_logit()
    mask = rng.choice([0, 0, 0, 1, 2], n).astype(np.int8)
    mask[5:9] = 0
    cls, w = mcmc_ref.weights(ft, mask, mcmc_ref.min_opacity_logit())
    assert cls[5] == "d" and cls[7] == "d" and cls[8] == "d"        # NaN, far below, and exactly the threshold: not above it
    assert cls[6] == "a" and w[6] == 2 ** 24 - 1                    # sigmoid(30) is 1.0f: the clamp
    assert all((c == "a") == (x > 0) for c, x in zip(cls, w)) and all(1 <= x < 2 ** 24 for x in w if x)
    assert all(type(x) is int for x in w)
    D = 400
    source_of, ts, W = mcmc_ref.draw_sources(w, D, seed=11, call_index=2)
    assert W == sum(w) and len(source_of) == D
    prefix = [sum(w[:i]) for i in range(n)]
    for t, s in zip(ts, source_of):
        assert 0 <= t < W and w[s] > 0 and prefix[s] <= t < prefix[s] + w[s]
    assert mcmc_ref.draw_sources(w, D, seed=11, call_index=3)[0] != source_of
    assert mcmc_ref.draw_sources(w, D, seed=11, call_index=2)[0] == source_of
    # a block of 256 saturated rows sums past 2^31
    assert sum([2 ** 24 - 1] * 256) > 2 ** 31


def test_budget():
    assert mcmc_ref.budget(1000, 10, 990, 500, 50, 10 ** 6) == (50, 60)
    assert mcmc_ref.budget(1019, 0, 1019, 500, 50, 10 ** 6) == (50, 50)          # floor(1019 * 50 / 1000) = 50
    assert mcmc_ref.budget(1000, 10, 990, 20, 50, 10 ** 6) == (20, 30)           # clipped by the free rows
    assert mcmc_ref.budget(1000, 10, 990, 500, 50, 1020) == (20, 30)             # clipped by the cap
    assert mcmc_ref.budget(1000, 10, 990, 500, 50, 900) == (0, 10)               # a cap below the valid rows adds nothing
    assert mcmc_ref.budget(1000, 1000, 0, 500, 50, 10 ** 6) == (0, 0)            # nothing alive: nothing to copy


def test_draws_follow_the_weights():
    """2 * 10^5 draws over 7 weights land within 5 sigma of the binomial expectation"""
    w = [1, 2 ** 24 - 1, 0, 5_000_000, 123_456, 0, 9_000_000]
    D = 200_000
    source_of, _, W = mcmc_ref.draw_sources(w, D, seed=5, call_index=0)
    hits = np.bincount(source_of, minlength=len(w))
    for x, h in zip(w, hits):
        q = x / W
        assert abs(h - D * q) <= 5.0 * math.sqrt(D * q * (1.0 - q)) + (1 if x == 1 else 0), (x, h)
        assert x > 0 or h == 0


def test_noise_is_gated_and_row_local():
    rng = np.random.default_rng(1)
    n = 300
    ft = rng.normal(0.0, 0.5, (n, 56)).astype(np.float32)
    ft[:, 4:7] -= 3.0
    ft[0, 7], ft[1, 7], ft[2, 5] = 10.0, -6.0, np.nan
    mask = np.zeros(n, np.int8)
    mask[3], mask[4] = 1, 2
    delta, mag, moves = mcmc_ref.noise(ft, mask, 80.0, seed=9, step_index=4)
    assert not moves[2] and not moves[3] and not moves[4] and moves[0] and moves[1]
    assert np.abs(delta[0]).max() < 1e-30 and np.abs(delta[1]).max() > 1e-6       # an opaque row stays, a transparent one moves
    assert (np.abs(delta) <= mag + 1e-300).all()
    again, _, _ = mcmc_ref.noise(ft[:100], mask[:100], 80.0, seed=9, step_index=4)
    assert np.array_equal(again, delta[:100])
    other, _, _ = mcmc_ref.noise(ft, mask, 80.0, seed=9, step_index=5)
    assert not np.array_equal(other[moves], delta[moves])


def test_regulariser_gradient_is_the_derivative_of_the_value():
    rng = np.random.default_rng(2)
    n = 50
    ft = rng.normal(0.0, 1.0, (n, 56)).astype(np.float32)
    mask = rng.choice([0, 0, 1, 2], n).astype(np.int8)
    value, added = mcmc_ref.regulariser(ft, mask, 0.01, 0.02)
    assert value[2] == (mask == 0).sum() and (added[mask != 0] == 0).all() and (added[:, :4] == 0).all() and (added[:, 8:] == 0).all()
    valid = mask == 0
    o = 1.0 / (1.0 + np.exp(-ft[valid, 7].astype(np.float64)))
    assert abs(value[0] - 0.01 * o.mean()) < 1e-8 and abs(value[1] - 0.02 * np.exp(ft[valid, 4:7].astype(np.float64)).mean()) < 1e-7
    assert np.allclose(added[valid, 7], 0.01 * o * (1 - o) / valid.sum(), rtol=1e-5)
    assert np.allclose(added[valid, 4:7], 0.02 * np.exp(ft[valid, 4:7].astype(np.float64)) / (3 * valid.sum()), rtol=1e-5)
    assert (mcmc_ref.regulariser(ft, np.ones(n, np.int8), 0.01, 0.02)[0] == 0).all()
