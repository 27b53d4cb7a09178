"""CPU: tests/mcmc_ref.py, the restatement of include/gs_mcmc.h, against itself and against exact arithmetic."""
import decimal
import math

import numpy as np
import pytest

import mcmc_cases as MC
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


# ---- the scenes of tests/mcmc_cases.py are the ones the kernels change path at ------------------------------------------------
# Each test asserts, from tests/mcmc_ref.py alone, what its scene exists for.  One that fails means the scene must change.
def _thread_of(block, n):
    return block // MC.per_thread(n)


def test_case_past_1024_blocks_gives_every_scan_thread_two_blocks():
    s, ref = MC.scene("past_1024_blocks"), MC.reference("past_1024_blocks")
    n = s["pc"].shape[0]
    assert n == MC.N_LARGE and MC.blocks(n) == 1026 and MC.per_thread(n) == 2
    f, c = MC.block_facts("past_1024_blocks"), MC.counts(ref)
    print(c)
    both = [t for t in range(MC.blocks(n) // 2) if all(f[k][2 * t] > 0 and f[k][2 * t + 1] > 0 for k in ("weight", "dead"))]
    assert 150 in both and any(t < 512 for t in both)              # a thread whose second block adds to a running prefix
    assert _thread_of(1024, n) == _thread_of(1025, n) == 512 and 513 * MC.per_thread(n) >= MC.blocks(n)     # 513.. own nothing
    for b in (1024, 1025):                                          # the last full block and the partial one
        assert f["dead"][b] > 0 and f["free"][b] > 0 and f["alive"][b] > 0, b
    assert any(r >= MC.N_FULL for r in ref["source_of"]) and any(r >= MC.N_FULL for r in ref["dest_row"])
    assert c["new"] > 0 and c["dead"] > 0 and c["free"] > c["new"]                                          # some free rows stay free
    assert int((s["mask"] == 2).sum()) > n - 1200


def test_case_second_turn_has_destinations_past_1024_blocks_of_them():
    s = MC.scene("second_turn")
    for n_max in (51, 5):
        ref = MC.reference("second_turn", n_max=n_max)
        c = MC.counts(ref)
        print(n_max, c)
        assert c["destinations"] > MC.N_FULL and c["alive"] == c["sources"] == 5 and c["new"] == MC.SECOND_TURN_FREE
        rows = MC.second_turn_rows("second_turn", n_max=n_max)
        assert len(rows) == c["destinations"] - MC.N_FULL == 294
        assert int((s["mask"][rows] == 0).sum()) == 254 and int((s["mask"][rows] == 1).sum()) == 40         # dead rows, then free rows
        assert min(ref["multiplicity"][r] for r, _ in MC.SECOND_TURN_ALIVE) > 10_000 > n_max               # M is clamped to n_max
        assert {ref["source_of"][j] for j in range(MC.N_FULL, c["destinations"])} >= {7, MC.N_LARGE - 1}


def test_case_unit_weights_puts_draws_on_every_kind_of_prefix_boundary():
    s, ref = MC.scene("unit_weights"), MC.reference("unit_weights")
    f = MC.unit_facts()
    print(MC.counts(ref), f)
    assert s["settings"]["min_opacity"] == 1e-9 and s["settings"]["call_index"] == MC.UNIT_CALL_INDEX
    assert f["weights"] == [1, 2] and f["raised_to_one"] > 0 and f["W"] < 1000
    assert 2 * f["draws_on_a_prefix"] >= f["D"] > 0
    # the all-dead block between two blocks with weight, and a draw on the prefix it shares with its successor
    assert f["empty_block_weight"] == 0 and 0 < f["weight_before_the_empty_block"] < f["W"]
    hit = f["draws_on_the_shared_prefix"]
    assert len(hit) >= 1 and set(hit) == {f["first_alive_after_the_empty_block"]}
    assert f["first_alive_after_the_empty_block"] >= (MC.UNIT_EMPTY_BLOCK + 1) * MC.BLOCK
    assert len(f["seams_drawn_on_both_sides"]) >= 1                 # the last alive row of a block and the first of the next
    assert f["sources_clamped_up"] >= 1
    _, _, (o, p, d) = mcmc_ref.relocated(s["ft"][hit[0], 7], s["ft"][hit[0], 4:7], int(ref["multiplicity"][hit[0]]), 51)
    assert p == mcmc_ref.P_MIN and o < 2.0 ** -22 and -17.0 < math.log(o / d) < -9.0


@pytest.mark.parametrize("name, n, nb, per", [("blocks_1024", MC.N_FULL, 1024, 1), ("blocks_1025_last_alive", MC.N_FULL + 1, 1025, 2),
                                              ("blocks_1025_last_dead", MC.N_FULL + 1, 1025, 2)])
def test_case_boundary_sizes_around_one_block_per_scan_thread(name, n, nb, per):
    s, ref = MC.scene(name), MC.reference(name)
    c = MC.counts(ref)
    print(c)
    assert s["pc"].shape[0] == n and MC.blocks(n) == nb and MC.per_thread(n) == per
    assert c["dead"] > 0 and c["new"] > 0 and c["sources"] > 0
    f = MC.block_facts(name)
    if name == "blocks_1025_last_alive":                            # block 1024 is one row, alone with scan thread 512
        assert f["alive"][1024] == 1 and ref["weights"][-1] > 0 and n - 1 in ref["source_of"]
    if name == "blocks_1025_last_dead":
        assert f["dead"][1024] == 1 and ref["dest_row"][c["dead"] - 1] == n - 1
    if name == "blocks_1024":
        assert f["weight"][1023] > 0 and f["dead"][1023] > 0


def test_case_loop_scene_has_rows_the_noise_moves_and_rows_that_are_dead():
    import trainer_util as TU
    pc, ft, rows = MC.loop_initial(*TU.perturbed(TU.ground_truth_scene()))
    assert len(rows) == MC.LOOP_PLANTED == 40 and rows.max() < TU.N_POINTS
    logit = ft[rows, 7]
    threshold = mcmc_ref.min_opacity_logit()
    assert logit.min() == -6.0 and logit.max() == -2.5 and 5 <= int((logit <= threshold).sum()) <= 35
    mask = np.zeros(len(pc), np.int8)
    scale = MC.LOOP["noise_lr"] * MC.LOOP["position_learning_rate"]
    for step in (0, 1, 2):
        moved = MC.rows_moved_by_more_than_an_ulp(pc, ft, mask, scale, MC.LOOP["seed"], step)
        print(f"step {step}: {len(moved)} rows move by more than an ulp of their position, {len(set(moved) & set(rows))} of them planted")
        assert len(moved) >= 10
