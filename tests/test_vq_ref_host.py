"""CPU: the host restatement of include/gs_vq.h (vq_ref.py, vq_ref.c) against float64 brute force, within a derived bound:
for every row, d2(label) <= min_k d2(k) + tol_n and |dist - d2(label)| <= tol_n with
tol_n = 2 (Dp + 3) 2^-24 (max_k (2 sum_j |x_j c_kj| + sum_j c_kj^2) + sum_j x_j^2) in float64 (vq_ref.brute_force says why)."""
import numpy as np
import pytest

import vq_ref

CASES = [(3000, 300, 45), (2000, 64, 3), (2000, 513, 64)]


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("vq_ref")


def _planted(n, k, d, seed):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 1.0, (max(k // 3, 1), d))
    x = centres[rng.integers(0, centres.shape[0], n)] + rng.normal(0.0, 0.05, (n, d))
    codebook = np.concatenate([centres, rng.normal(0.0, 1.0, (k - centres.shape[0], d))])
    return x.astype(np.float32), codebook.astype(np.float32)


def _iid(n, k, d, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1.0, (n, d)).astype(np.float32), rng.normal(0.0, 1.0, (k, d)).astype(np.float32)


@pytest.mark.parametrize("data", ["planted", "iid"])
@pytest.mark.parametrize("n,k,d", CASES)
def test_assignment_is_the_nearest_centroid_within_the_bound(build_dir, data, n, k, d):
    x, codebook = (_planted if data == "planted" else _iid)(n, k, d, seed=n + k + d)
    codebook[k // 2] = codebook[1]                                  # a duplicated centroid never wins over its first copy
    labels, dist = vq_ref.assign(build_dir, x, codebook)
    d2, tol = vq_ref.brute_force(x, codebook)
    rows = np.arange(n)
    assert labels.min() >= 0 and labels.max() < k and not np.any(labels == k // 2)
    assert np.all(d2[rows, labels] <= d2.min(1) + tol)
    assert np.all(np.abs(dist.astype(np.float64) - d2[rows, labels]) <= tol)


def test_ties_non_finite_values_and_unread_columns(build_dir):
    rng = np.random.default_rng(5)
    x, codebook = _iid(40, 12, 5, seed=5)
    codebook[9] = codebook[5]
    x[3] = codebook[5]
    labels, dist = vq_ref.assign(build_dir, x, codebook)
    assert labels[3] == 5 and dist[3] <= 1e-5 and not np.any(labels == 9)
    bad = x.copy()
    bad[7, 2], bad[8, 0] = np.nan, np.inf
    cb = codebook.copy()
    cb[labels[0], 1] = np.nan
    got, gd = vq_ref.assign(build_dir, bad, cb)
    assert got[7] == -1 and got[8] == -1 and np.isnan(gd[7]) and np.isnan(gd[8])
    assert got[0] != labels[0] and got[0] >= 0 and not np.any(got == labels[0])
    cb[:, 0] = np.inf
    got, gd = vq_ref.assign(build_dir, x, cb)
    assert np.all(got == -1) and np.all(np.isnan(gd))
    # columns past dim are not read: NaN there changes nothing
    xp, ldx = vq_ref.padded(x)
    cp, ldc = vq_ref.padded(codebook)
    xp[:, 5:], cp[:, 5:] = np.nan, np.nan
    got, gd = vq_ref.assign(build_dir, xp, cp, ldx=ldx, ldc=ldc, dim=5)
    assert np.array_equal(got, labels) and np.array_equal(gd, dist)
    assert rng is not None


def test_update_adds_members_strictly_in_row_order():
    x = np.zeros((1000, 3), np.float32)
    x[0], x[300], x[900] = 3e30, 1.0, -3e30
    labels = np.full(1000, -1, np.int32)
    labels[[0, 300, 900]] = 1
    codebook = np.arange(9, dtype=np.float32).reshape(3, 3)
    new, counts, W = vq_ref.update(x, labels, codebook)
    # (3e30 + 1) + -3e30 is 0 in float64; 3e30 + -3e30 + 1 would be 1
    assert np.array_equal(new[1], np.zeros(3, np.float32)) and list(counts) == [0, 3, 0] and list(W) == [0.0, 3.0, 0.0]
    assert np.array_equal(new[[0, 2]], codebook[[0, 2]])
    reordered, _, _ = vq_ref.update(x[[0, 900, 300]], labels[[0, 900, 300]], codebook)
    assert np.array_equal(reordered[1], np.full(3, 1.0 / 3.0, np.float32))


def test_update_skips_bad_weights_and_foreign_labels():
    rng = np.random.default_rng(2)
    x = rng.normal(0, 1, (50, 4)).astype(np.float32)
    labels = rng.integers(-1, 5, 50).astype(np.int32)              # -1 and 4 belong to nobody of K = 4
    weights = rng.uniform(0.5, 2.0, 50).astype(np.float32)
    weights[[1, 2, 3, 4]] = [0.0, -1.0, np.nan, np.inf]
    codebook = rng.normal(0, 1, (4, 4)).astype(np.float32)
    new, counts, W = vq_ref.update(x, labels, codebook, weights)
    for k in range(4):
        m = (labels == k) & (weights > 0) & np.isfinite(weights)
        assert counts[k] == m.sum()
        want = (weights[m, None].astype(np.float64) * x[m]).sum(0) / weights[m].astype(np.float64).sum()
        assert np.allclose(new[k], want, rtol=1e-6, atol=1e-7) and np.isclose(W[k], weights[m].astype(np.float64).sum())
