"""CPU: the brute-force f32 reference of the k-NN entry point (tests/knn_ref.py) against scipy's cKDTree in float64 -- the
call the reference's scene initialiser makes (GaussianPointCloudScene.py:82-85) -- on the five clouds every k-NN test shares.

The mean 3-NN distance in f32 is within 1e-6 relative of float64 on the same f32 coordinates: one rounding in each of dx, the
three squares, the two sums, the square root, the two sums of the mean and the division is about 6 * 2^-24 = 3.6e-7, and
picking another neighbour among near-ties moves the value by no more than that.  Where the k + 1 smallest float64 distances
of a row (itself and its k neighbours) are distinct beyond 1e-6 relative, and the k-th neighbour's from the one behind it,
the neighbours are cKDTree's."""
import numpy as np
import pytest

import knn_ref

scipy_spatial = pytest.importorskip("scipy.spatial", reason="scipy is the yardstick here")

CLOUDS = knn_ref.clouds()
K = 3


@pytest.fixture(scope="module")
def results():
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
