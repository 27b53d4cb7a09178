"""GPU (-m gpu): gs_vq_assign and gs_vq_update (vq.py) against the host restatement of include/gs_vq.h (vq_ref.py, vq_ref.c): labels,
distances, centroids, counts and weight sums bit for bit; and, independently of the restatement, the assignment against float64
brute force within the derived bound of vq_ref.brute_force."""
import numpy as np
import pytest
import torch

import vq_ref
from taichi_3d_gaussian_splatting_amd import vq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = (1, 31, 33, 64, 65, 257, 1000)
CODES = (1, 2, 31, 33, 255, 257)


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("vq_ref")


def _data(n, k, d, seed, planted=True):
    rng = np.random.default_rng(seed)
    codebook = rng.normal(0.0, 1.0, (k, d)).astype(np.float32)
    if planted:
        x = (codebook[rng.integers(0, k, n)] + rng.normal(0.0, 0.3, (n, d))).astype(np.float32)
    else:
        x = rng.normal(0.0, 1.0, (n, d)).astype(np.float32)
    return x, codebook


def _dev(a):
    return torch.tensor(a, device=DEV)


def _same_bits(got, want):
    """the same dtype, shape and bits; a NaN matches any NaN"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    nan = np.isnan(want)
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(bits), want[~nan].view(bits))


def _check_assign(build_dir, x, codebook):
    labels, dist = vq.assign(_dev(x), _dev(codebook))
    want_labels, want_dist = vq_ref.assign(build_dir, x, codebook)
    got_labels, got_dist = labels.cpu().numpy(), dist.cpu().numpy()
    bad = np.nonzero(got_labels != want_labels)[0]
    assert bad.size == 0, (bad[:8], got_labels[bad[:8]], want_labels[bad[:8]])
    assert _same_bits(got_dist, want_dist), np.nonzero(got_dist != want_dist)[0][:8]
    return got_labels, got_dist


@pytest.mark.parametrize("n", ROWS)
def test_assign_matches_the_header_bit_for_bit_over_rows_and_codes(build_dir, n):
    for k in CODES:
        x, codebook = _data(n, k, 45, seed=1000 * n + k, planted=k % 2 == 1)
        _check_assign(build_dir, x, codebook)


@pytest.mark.parametrize("d", (1, 3, 4, 48, 63, 64))
def test_assign_matches_over_dimensions(build_dir, d):
    x, codebook = _data(257, 33, d, seed=d)
    _check_assign(build_dir, x, codebook)


def test_assign_with_the_largest_codebook(build_dir):
    x, codebook = _data(40, 65536, 4, seed=9, planted=False)
    labels, _ = _check_assign(build_dir, x, codebook)
    assert labels.max() > 4096


def test_assign_does_not_read_columns_past_dim(build_dir):
    x, codebook = _data(130, 70, 45, seed=3)
    want = vq_ref.assign(build_dir, x, codebook)
    xp = torch.full((130, 52), float("nan"), device=DEV)
    cp = torch.full((70, 48), float("nan"), device=DEV)
    xp[:, :45], cp[:, :45] = _dev(x), _dev(codebook)
    assert vq.padded(xp[:, :45])[0] is not None and vq.padded(xp[:, :45])[1] == 52 and vq.padded(cp[:, :45])[1] == 48
    labels, dist = vq.assign(xp[:, :45], cp[:, :45])
    assert np.array_equal(labels.cpu().numpy(), want[0]) and _same_bits(dist, want[1])


@pytest.mark.parametrize("first,second", [(5, 9), (5, 40), (31, 32), (1, 5), (5, 70), (63, 64), (2, 130)])
def test_the_smaller_index_wins_between_duplicated_centroids(build_dir, first, second):
    """within a tile, across the two accumulators of a tile, across tiles and across the lane halves of a column"""
    x, codebook = _data(200, 140, 45, seed=first * 256 + second)
    codebook[second] = codebook[first]
    x[::3] = codebook[first]                                        # exact ties: s is the same number for both copies
    x[1::3] = codebook[first] + np.float32(0.01) * x[1::3]
    labels, _ = _check_assign(build_dir, x, codebook)
    assert np.all(labels[::3] == first) and not np.any(labels == second)


def test_non_finite_rows_and_centroids(build_dir):
    x, codebook = _data(100, 70, 45, seed=21)
    x[3, 7], x[40, 0], x[41, 44] = np.nan, np.inf, -np.inf
    base, _ = vq_ref.assign(build_dir, x, codebook)
    codebook[base[0], 5] = np.nan
    codebook[base[1], 0] = np.inf
    labels, dist = _check_assign(build_dir, x, codebook)
    assert list(labels[[3, 40, 41]]) == [-1, -1, -1] and np.all(np.isnan(dist[[3, 40, 41]]))
    assert labels[0] not in (-1, base[0]) and labels[1] not in (-1, base[1])
    codebook[:, 2] = np.nan
    codebook[::2, 2] = np.inf
    labels, dist = _check_assign(build_dir, x, codebook)
    assert np.all(labels == -1) and np.all(np.isnan(dist))


def test_assign_against_float64_brute_force_within_the_derived_bound():
    x, codebook = _data(1000, 257, 45, seed=77)
    labels, dist = vq.assign(_dev(x), _dev(codebook))
    labels, dist = labels.cpu().numpy(), dist.cpu().numpy().astype(np.float64)
    d2, tol = vq_ref.brute_force(x, codebook)
    rows = np.arange(1000)
    assert labels.min() >= 0 and labels.max() < 257
    print("largest excess over the minimum / tol:", float(((d2[rows, labels] - d2.min(1)) / tol).max()),
          " largest |dist - d2| / tol:", float((np.abs(dist - d2[rows, labels]) / tol).max()))
    assert np.all(d2[rows, labels] <= d2.min(1) + tol)
    assert np.all(np.abs(dist - d2[rows, labels]) <= tol)


def _check_update(x, labels, codebook, weights=None):
    cb = _dev(codebook)
    counts, sums = vq.update(_dev(x), _dev(labels), cb, None if weights is None else _dev(weights))
    want_cb, want_counts, want_sums = vq_ref.update(x, labels, codebook, weights)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    assert _same_bits(sums, want_sums)
    assert _same_bits(cb, want_cb), np.nonzero(cb.cpu().numpy() != want_cb)
    return cb.cpu().numpy(), want_counts


@pytest.mark.parametrize("k,d", [(37, 45), (1500, 5), (3, 64), (1, 1)])
def test_update_matches_the_header_bit_for_bit(k, d):
    """both kernel shapes (one code per wave up to 1024 codes, four beyond), empty codes, labels of nobody, one large code"""
    rng = np.random.default_rng(k + d)
    n = 3000
    x = rng.normal(0, 1, (n, d)).astype(np.float32)
    labels = rng.integers(-1, k + 1, n).astype(np.int32)           # -1 and k belong to nobody
    labels[rng.random(n) < 0.4] = k // 2                            # one code with more than 1000 members
    if k > 4:
        labels[labels == 3] = -5                                    # an empty code keeps its bits
    labels[7], labels[8] = 2 ** 31 - 1, -2 ** 31
    codebook = rng.normal(0, 1, (k, d)).astype(np.float32)
    _, counts = _check_update(x, labels, codebook)
    assert counts[k // 2] > 1000 and (k <= 4 or counts[3] == 0)
    weights = rng.uniform(0.1, 3.0, n).astype(np.float32)
    weights[rng.random(n) < 0.1] = 0.0
    weights[10:14] = [-1.0, np.nan, np.inf, -np.inf]
    _check_update(x, labels, codebook, weights)


def test_update_adds_in_row_order_and_handles_no_rows():
    x = np.zeros((1000, 3), np.float32)
    x[0], x[300], x[900] = 3e30, 1.0, -3e30
    labels = np.full(1000, -1, np.int32)
    labels[[0, 300, 900]] = 1
    codebook = np.arange(9, dtype=np.float32).reshape(3, 3)
    got, _ = _check_update(x, labels, codebook)
    assert np.array_equal(got[1], np.zeros(3, np.float32))          # (3e30 + 1) - 3e30; any other order gives 1/3
    cb = _dev(codebook)
    counts, sums = vq.update(torch.zeros(0, 3, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), cb)
    assert counts.tolist() == [0, 0, 0] and sums.tolist() == [0.0, 0.0, 0.0] and np.array_equal(cb.cpu().numpy(), codebook)
    labels0, dist0 = vq.assign(torch.zeros(0, 3, device=DEV), cb)
    assert labels0.numel() == 0 and dist0.numel() == 0


def test_three_kmeans_iterations_match_the_reference_loop(build_dir):
    rng = np.random.default_rng(4)
    protos = rng.normal(0, 1, (30, 45))
    x = (protos[rng.integers(0, 30, 2000)] + rng.normal(0, 0.1, (2000, 45))).astype(np.float32)
    weights = rng.uniform(0.2, 2.0, 2000).astype(np.float32)
    for w in (None, weights):
        rows = vq.initial_rows(2000, 37, seed=5).numpy()
        want_cb, want_labels, want_dist, want_counts = vq_ref.kmeans(build_dir, x, rows, 3, w)
        codebook, labels, history = vq.kmeans(_dev(x), 37, iters=3, weights=None if w is None else _dev(w), seed=5, reseed_empty=False)
        assert _same_bits(codebook, want_cb) and np.array_equal(labels.cpu().numpy(), want_labels)
        assert len(history) == 4 and all(np.isfinite(history)) and history[-1] <= history[0]
        ww = np.ones(2000) if w is None else w.astype(np.float64)
        assert np.isclose(history[-1], float((want_dist.astype(np.float64) * ww).sum()), rtol=1e-12)
    # with reseeding no code stays empty when there are rows enough
    codebook, labels, _ = vq.kmeans(_dev(x[:600]), 64, iters=4, seed=1)
    assert codebook.shape == (64, 45) and torch.bincount(labels.long(), minlength=64).min() > 0
    assert vq.kmeans(_dev(x[:5]), 9, iters=1)[0].shape == (5, 45)   # k is clipped to n


def test_the_same_call_twice_and_on_a_side_stream_gives_the_same_bits():
    x, codebook = _data(1000, 300, 45, seed=31)
    xd, cd = _dev(x), _dev(codebook)
    first = vq.assign(xd, cd)
    second = vq.assign(xd, cd)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        third = vq.assign(xd, cd)
        c3 = cd.clone()
        u3 = vq.update(xd, third[0], c3)
    stream.synchronize()
    c1 = cd.clone()
    u1 = vq.update(xd, first[0], c1)
    for other in (second, third):
        assert torch.equal(first[0], other[0]) and torch.equal(first[1].view(torch.int32), other[1].view(torch.int32))
    assert torch.equal(c1.view(torch.int32), c3.view(torch.int32)) and torch.equal(u1[0], u3[0]) and torch.equal(u1[1], u3[1])
