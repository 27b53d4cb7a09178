"""CPU: the brute-force f32 reference of the k-NN entry point (tests/knn_ref.py) against scipy's cKDTree in float64 -- the
call the reference's scene initialiser makes (GaussianPointCloudScene.py:82-85) -- on the five clouds every k-NN test shares.

The mean 3-NN distance in f32 is within 1e-6 relative of float64 on the same f32 coordinates: one rounding in each of dx, the
three squares, the two sums, the square root, the two sums of the mean and the division is about 6 * 2^-24 = 3.6e-7, and
picking another neighbour among near-ties moves the value by no more than that.  Where the k + 1 smallest float64 distances
of a row (itself and its k neighbours) are distinct beyond 1e-6 relative, and the k-th neighbour's from the one behind it,
the neighbours are cKDTree's.

Without scipy: what the reference says about pairs at +inf, on a case small enough to read; torch_knn, the same brute force in
torch (the yardstick of the GPU tests at sizes numpy cannot cover row by row), equal to it bit for bit on every cloud and mask
the k-NN tests use; and the rows= form equal to the same rows of the full result."""
import numpy as np
import pytest
import torch

import knn_ref

CLOUDS = knn_ref.clouds()
K = 3


@pytest.fixture(scope="module")
def results():
    scipy_spatial = pytest.importorskip("scipy.spatial", reason="scipy is the yardstick here")
    out = {}
    for name, x in CLOUDS.items():
        x64 = x.astype(np.float64)
        dist, idx = scipy_spatial.cKDTree(x64).query(x64, k=K + 2)
        out[name] = (knn_ref.knn(x, K), dist, idx)
    return out


def test_the_clouds_are_what_the_tests_say():
    assert {n: c.shape[0] for n, c in CLOUDS.items()} == dict(uniform=4096, outliers=4008, duplicates=3000, coplanar=2000, clusters=2100)
    assert all(c.dtype == np.float32 and c.shape[1] == 3 for c in CLOUDS.values())
    dup = CLOUDS["duplicates"]
    assert len(np.unique(dup, axis=0)) < len(dup), "the f32 grid at 1000 should merge some of the points"
    assert np.abs(CLOUDS["outliers"]).max() > 1e5 and (CLOUDS["coplanar"][:, 2] == 0.25).all()


@pytest.mark.parametrize("name", list(CLOUDS))
def test_mean_distance_matches_ckdtree_in_float64(results, name):
    (d2, _), dist, _ = results[name]
    want = dist[:, 1:K + 1].mean(axis=1)                # the row itself is the first hit (or, among duplicates, one of them)
    got = np.sqrt(d2.astype(np.float64)).mean(axis=1)
    assert ((want == 0) == (got == 0)).all()
    nz = want > 0
    rel = np.abs(got[nz] - want[nz]) / want[nz]
    print(f"{name}: largest relative error of the mean 3-NN distance {rel.max():.3e}")
    assert rel.max() < 1e-6
    # the float64 brute force agrees with the tree as well (it is the yardstick of the GPU tests, which have no scipy need)
    ref64 = knn_ref.mean_distance(CLOUDS[name], K)
    assert (np.abs(ref64[nz] - want[nz]) <= 1e-12 * want[nz]).all()


@pytest.mark.parametrize("name", list(CLOUDS))
def test_neighbours_are_ckdtrees_where_the_distances_are_distinct(results, name):
    (_, idx), dist, tree_idx = results[name]
    rows = np.arange(len(idx))
    # the row itself, its K neighbours, and the one behind them: where the K-th ties with the (K+1)-th -- on the f32 grid of
    # the duplicates cloud thousands do, exactly -- the K nearest are not one set and the tree's pick is arbitrary
    d = dist[:, :K + 2]
    gaps = np.diff(d, axis=1) > 1e-6 * d[:, 1:]
    clear = gaps.all(axis=1) & (tree_idx[:, 0] == rows)
    # (on the duplicates cloud most rows tie somewhere; the comparison still has rows to stand on)
    assert clear.sum() > (0 if name == "duplicates" else 0.5 * len(idx)), int(clear.sum())
    assert (idx[clear] == tree_idx[clear, 1:K + 1]).all()


def test_reference_semantics_on_a_case_small_enough_to_read():
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 2, 0], [np.nan, 0, 0], [5, 5, 5]], np.float32)
    mask = np.array([0, 0, 0, 0, 0, 1], np.int8)
    d2, idx = knn_ref.knn(x, 4, mask)
    assert idx.tolist() == [[2, 1, 3, -1], [0, 2, 3, -1], [0, 1, 3, -1], [0, 2, 1, -1], [-1] * 4, [-1] * 4]
    assert d2[0].tolist() == [0.0, 1.0, 4.0, np.inf] and d2[3].tolist() == [4.0, 4.0, 5.0, np.inf]
    assert np.isinf(d2[4:]).all()


def test_pairs_at_infinity_on_a_case_small_enough_to_read():
    """Row 0 has two finite pairs, then two at +inf that come with their rows, the smaller row first, then the -1 tail: five
    rows take part, so four others answer and k = 6 leaves two places empty.  Rows 3 and 4 are at +inf from everything,
    each other included (their difference overflows before it is squared)."""
    inf, big = np.inf, 3e38
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [big, 0, 0], [-big, big, 0], [7, 7, 7], [0, np.inf, 0]], np.float32)
    mask = np.array([0, 0, 0, 0, 0, 1, 0], np.int8)
    d2, idx = knn_ref.knn(x, 6, mask)
    assert not np.isnan(d2).any()
    assert idx.tolist() == [[1, 2, 3, 4, -1, -1], [0, 2, 3, 4, -1, -1], [0, 1, 3, 4, -1, -1], [0, 1, 2, 4, -1, -1],
                            [0, 1, 2, 3, -1, -1], [-1] * 6, [-1] * 6]
    assert d2.tolist() == [[1, 4, inf, inf, inf, inf], [1, 5, inf, inf, inf, inf], [4, 5, inf, inf, inf, inf], [inf] * 6, [inf] * 6,
                           [inf] * 6, [inf] * 6]
    # k below the number of pairs: a pair at +inf is the last one chosen, never NaN, never the row itself
    d2, idx = knn_ref.knn(x, 3, mask)
    assert idx[:5].tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 2]] and d2[0].tolist() == [1, 4, inf]


def _cases():
    named = {**{n: (lambda c=c: c) for n, c in CLOUDS.items()}, **knn_ref.EXTRA}
    del named["big_clusters"]                    # 65 537 rows: on the GPU only, against a sample of numpy rows
    out = [(n, None) for n in named]
    return out + [("overflow", "fifth")] + [("uniform", m) for m in ("third", "all", "garbage", "nan_row")], named


CASES, NAMED = _cases()


@pytest.fixture(scope="module")
def full():
    """k = 8 by numpy, once per (cloud, mask)"""
    cache = {}

    def get(name, mask_name):
        if (name, mask_name) not in cache:
            x, mask = knn_ref.masked(NAMED[name](), mask_name)
            cache[name, mask_name] = (x, mask, knn_ref.knn(x, 8, mask))
        return cache[name, mask_name]
    return get


@pytest.mark.parametrize("name,mask_name", CASES)
def test_torch_knn_equals_the_numpy_reference_bit_for_bit(full, name, mask_name):
    x, mask, (d2, idx) = full(name, mask_name)
    assert not np.isnan(d2).any()
    for k in (8, 3):
        td2, tidx = knn_ref.torch_knn(torch.from_numpy(x), k, None if mask is None else torch.from_numpy(mask),
                                      chunk=2048 if k == 8 else 1000)
        assert td2.dtype == torch.float32 and tidx.dtype == torch.int32 and td2.shape == tidx.shape == (len(x), k)
        assert np.array_equal(td2.numpy().view(np.uint32), d2[:, :k].view(np.uint32)), (name, mask_name, k)
        assert np.array_equal(tidx.numpy(), idx[:, :k]), (name, mask_name, k)


@pytest.mark.parametrize("name,mask_name", [("uniform", "garbage"), ("overflow", "fifth"), ("copies", None), ("clusters", None)])
def test_chosen_rows_equal_the_same_rows_of_the_full_result(full, name, mask_name):
    x, mask, (d2, idx) = full(name, mask_name)
    rows = np.random.default_rng(3).permutation(len(x))[:97]             # unordered, masked rows among them
    rows = np.concatenate([rows, rows[:2], [0, len(x) - 1]])             # ... and a row may be asked for twice
    rd2, ridx = knn_ref.knn(x, 8, mask, rows=rows, chunk=40)
    assert rd2.shape == ridx.shape == (len(rows), 8)
    assert np.array_equal(rd2.view(np.uint32), d2[rows].view(np.uint32)) and np.array_equal(ridx, idx[rows])
    empty = knn_ref.knn(x, 8, mask, rows=np.zeros(0, np.int64))
    assert empty[0].shape == empty[1].shape == (0, 8)
