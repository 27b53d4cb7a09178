"""CPU: tests/exchange_ref.py, the numpy statement of the packed-row layout and of the fixed-order merge, against the dense
rank-ordered sum of scattered gradients -- what an exchange of dense buffers computes."""
import numpy as np
import pytest

import exchange_ref as X

N = 400


def _gradients(rng, n=N):
    return rng.standard_normal((n, 56)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)


def _random_lists(rng, n_lists, n=N, share=0.3):
    lists = []
    for _ in range(n_lists):
        gf, gp = _gradients(rng, n)
        ids = np.flatnonzero(rng.random(n) < share).astype(np.int32)
        lists.append(X.pack(gf, gp, ids))
    return lists


def _merged(lists, n=N, fill=np.float32(7.5)):
    gf, gp = np.full((n, 56), fill, np.float32), np.full((n, 3), fill, np.float32)
    union = X.merge(lists, n, gf, gp)
    return union, np.concatenate([gf, gp], axis=1)


def test_packed_layout_word_for_word():
    rng = np.random.default_rng(0)
    gf, gp = _gradients(rng)
    gf[5, 0], gp[5, 2] = np.float32(-0.0), np.float32(np.inf)
    ids = np.array([0, 5, N - 1, N, -3], np.int32)
    p = X.pack(gf, gp, ids)
    assert p.shape == (5, 60) and p.dtype == np.uint32 and p.nbytes == 5 * 240
    for r in range(3):
        assert np.array_equal(p[r, :56], gf[ids[r]].view(np.uint32))
        assert np.array_equal(p[r, 56:59], gp[ids[r]].view(np.uint32))
    assert X.ids_of(p).tolist() == [0, 5, N - 1, -1, -1]
    assert p[1, 0] == 0x80000000 and p[1, 58] == 0x7F800000
    assert not p[3:, :59].any()


@pytest.mark.parametrize("n_lists", [1, 2, 3, 8])
def test_merge_against_the_dense_rank_ordered_sum(n_lists):
    rng = np.random.default_rng(n_lists)
    lists = _random_lists(rng, n_lists)
    union, got = _merged(lists)
    want_union = np.unique(np.concatenate([X.ids_of(p) for p in lists]))
    assert np.array_equal(union, want_union) and (np.diff(union) > 0).all()
    dense = X.dense_rank_ordered_sum(lists, N)
    assert (got[union] == dense[union]).all()                                  # equal under == everywhere on the union
    holders = np.zeros(N, np.int64)
    for p in lists:
        holders[X.ids_of(p)] += 1
    single_not_negative_zero = got.view(np.uint32) != 0x80000000
    same = got.view(np.uint32) == dense.view(np.uint32)
    assert same[union][(holders[union] >= 2)[:, None] | single_not_negative_zero[union]].all()
    # the general law behind it: the two differ only where the contract's answer is -0.0 and the zero-seeded sum gives +0.0
    diff = ~same[union]
    assert (got[union].view(np.uint32)[diff] == 0x80000000).all() and (dense[union].view(np.uint32)[diff] == 0).all()
    # rows outside the union keep every bit of the outputs; the dense sum is zero there
    out = np.setdiff1d(np.arange(N), union)
    assert (got[out] == np.float32(7.5)).all() and not dense[out].view(np.uint32).any()


def test_negative_zero_is_where_the_two_differ():
    rng = np.random.default_rng(9)
    gf, gp = _gradients(rng)
    gf[7, :] = np.float32(-0.0)
    gp[7, :] = np.float32(-0.0)
    empty = X.pack(gf, gp, np.zeros(0, np.int32))
    lists = [X.pack(gf, gp, np.array([3], np.int32)), X.pack(gf, gp, np.array([7, 9], np.int32)), empty]
    union, got = _merged(lists)
    assert union.tolist() == [3, 7, 9]
    dense = X.dense_rank_ordered_sum(lists, N)
    assert (got[union] == dense[union]).all()
    assert (got[7].view(np.uint32) == 0x80000000).all()                         # the contract: the single holder's bits, -0.0
    assert not dense[7].view(np.uint32).any()                                   # 0.0 + -0.0 = +0.0
    for row in (3, 9):
        assert np.array_equal(got[row].view(np.uint32), dense[row].view(np.uint32))
    # two holders of -0.0 with a non-holder before them: (0.0 + -0.0) + -0.0 = +0.0 against -0.0 + -0.0 = -0.0
    lists = [X.pack(gf, gp, np.array([3], np.int32)), X.pack(gf, gp, np.array([7], np.int32)), X.pack(gf, gp, np.array([7], np.int32))]
    union, got = _merged(lists)
    assert (got[7].view(np.uint32) == 0x80000000).all() and not X.dense_rank_ordered_sum(lists, N)[7].view(np.uint32).any()


def test_order_is_list_order_and_skipped_rows_are_skipped():
    a, b, c = np.float32(1e8), np.float32(-1e8), np.float32(1.0)
    assert np.float32(np.float32(a + b) + c) != np.float32(a + np.float32(b + c))
    rows = []
    for v in (a, b, c):
        gf, gp = np.full((N, 56), v, np.float32), np.full((N, 3), v, np.float32)
        rows.append(X.pack(gf, gp, np.array([-1, 11, N + 5], np.int32)))     # the bad ids pack to id word -1 and are skipped
    union, got = _merged([rows[0], X.pack(gf, gp, np.zeros(0, np.int32)), rows[1], rows[2]])
    assert union.tolist() == [11] and (got[11] == np.float32(1.0)).all()
    union, got = _merged([rows[1], rows[2], rows[0]])
    assert union.tolist() == [11] and (got[11] == np.float32(np.float32(b + c) + a)).all()
    union, got = _merged([X.pack(gf, gp, np.zeros(0, np.int32))] * 3)
    assert union.size == 0 and (got == np.float32(7.5)).all()
