"""GPU (-m gpu): gs_knn (include/gs_knn.h) against brute force in the same f32 arithmetic (tests/knn_ref.py): the squared
distances BIT-IDENTICAL and the neighbour rows EQUAL, at every size around a leaf (L = 64 rows) and around a complete tree, on
clouds whose distances tie, repeat and span eleven orders of magnitude, with masked and non-finite rows, through interior
pointers, across calls of different sizes on one context, on another stream, and between a forward and its backward.

Every k from 1 to 8 (four instantiations of the query kernel, and the store guard of a k below its instantiation's), pairs
whose distance overflows to +inf, subnormal distances, a cloud of identical points, and two clouds past one block of a tree
level and past two trips of the sort's digit scan.  Those two are compared on every row with knn_ref.torch_knn on the device,
which is itself compared with numpy there on a sample of rows first."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import knn_ref
import parity_util as P
from taichi_3d_gaussian_splatting_amd import _native, knn
from taichi_3d_gaussian_splatting_amd.synthetic import synth, view_pose

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = knn.LEAF
SIZES = [0, 1, 2, 3, 4, 5, L - 1, L, L + 1, 2 * L - 1, 2 * L + 1, 64 * L - 1, 64 * L, 64 * L + 1]
CLOUDS = knn_ref.clouds()
INF_BITS = np.float32(np.inf).view(np.uint32)


EXTRA = knn_ref.EXTRA


@functools.lru_cache(maxsize=None)
def cloud(name):
    if name in CLOUDS:
        return CLOUDS[name]
    if name in EXTRA:
        return EXTRA[name]()
    return knn_ref.uniform(int(name))            # the uniform generator, seed 0, by size


@functools.lru_cache(maxsize=None)
def reference(name, mask_name=None):
    """k = 8 once per cloud: the first k columns are the answer for every smaller k"""
    return knn_ref.knn(masked(name, mask_name)[0], 8, masked(name, mask_name)[1])


@functools.lru_cache(maxsize=None)
def masked(name, mask_name):
    return knn_ref.masked(cloud(name), mask_name)


def gpu(x, k, mask=None, indices=True):
    out = knn.nearest_neighbours(torch.from_numpy(x).to(DEV), k, None if mask is None else torch.from_numpy(mask).to(DEV), return_indices=indices)
    return tuple(t.cpu().numpy() for t in out) if indices else out.cpu().numpy()


def assert_equal(got, want, k, what):
    d2, idx = got
    rd2, ridx = want[0][:, :k], want[1][:, :k]
    assert d2.shape == rd2.shape and idx.shape == ridx.shape and d2.dtype == np.float32 and idx.dtype == np.int32
    same = d2.view(np.uint32) == rd2.view(np.uint32)
    assert same.all(), (what, "d2", int((~same).sum()), np.argwhere(~same)[:4].tolist())
    assert (idx == ridx).all(), (what, "idx", int((idx != ridx).sum()), np.argwhere(idx != ridx)[:4].tolist())


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_a_leaf_and_a_complete_tree(n, k):
    assert_equal(gpu(cloud(str(n)), k), reference(str(n)), k, (n, k))


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("name", list(CLOUDS) + ["lattice", "copies"])
def test_distributions(name, k):
    assert_equal(gpu(cloud(name), k), reference(name), k, (name, k))


def test_the_lattice_and_the_copies_are_decided_by_the_row_order():
    _, idx = reference("lattice")
    d2, _ = reference("lattice")
    assert (d2[:, 0] == 1).all() and (d2[:, :3] == 1).all(axis=1).sum() > 3000      # ties everywhere
    d2, idx = reference("copies")
    assert (d2[:100, :8] == 0).all() and idx[0].tolist() == [1, 2, 3, 4, 5, 6, 7, 8] and idx[5, :6].tolist() == [0, 1, 2, 3, 4, 6]


@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("mask_name", ["third", "all", "garbage", "nan_row"])
def test_masked_and_non_finite_rows(mask_name, k):
    x, mask = masked("uniform", mask_name)
    got = gpu(x, k, mask)
    assert_equal(got, reference("uniform", mask_name), k, (mask_name, k))
    out = ~knn_ref.takes_part(x, mask)
    assert out.sum() == {"third": 1366, "all": 4096, "garbage": 1366, "nan_row": 2}[mask_name]
    assert (got[0][out].view(np.uint32) == INF_BITS).all() and (got[1][out] == -1).all()
    assert not np.isin(got[1], np.flatnonzero(out)).any()
    if mask_name == "garbage":                   # ... the result is that of the clean cloud under the same mask
        assert_equal(got, reference("uniform", "third"), k, "garbage rows moved a valid row's result")
    if mask_name == "all":
        assert (got[1] == -1).all()


def raw_call(ctx, xyz, mask, n, k, d2_ptr, idx_ptr):
    knn._bind()
    _native.call("gs_knn", torch.device(DEV), ctx, xyz.data_ptr(), None if mask is None else mask.data_ptr(), n, k, d2_ptr, idx_ptr)


@pytest.mark.parametrize("n", [L + 1, 64 * L + 1])
def test_outputs_stay_inside_their_bounds(n):
    k, pad = 3, 257
    x = torch.from_numpy(cloud(str(n))).to(DEV)
    ctx = _native.Context(0)
    d2 = torch.full((n * k + 2 * pad,), -7.5, dtype=torch.float32, device=DEV)
    idx = torch.full((n * k + 2 * pad,), -77, dtype=torch.int32, device=DEV)
    raw_call(ctx.handle, x, None, n, k, d2.data_ptr() + 4 * pad, idx.data_ptr() + 4 * pad)
    for buf, sentinel in ((d2, -7.5), (idx, -77)):
        assert (buf[:pad] == sentinel).all() and (buf[-pad:] == sentinel).all()
    got = d2[pad:-pad].reshape(n, k).cpu().numpy(), idx[pad:-pad].reshape(n, k).cpu().numpy()
    assert_equal(got, reference(str(n)), k, n)
    assert not (got[0] == -7.5).any() and not (got[1] == -77).any()
    # distances alone: the same distances
    only = torch.full_like(d2, -7.5)
    raw_call(ctx.handle, x, None, n, k, only.data_ptr() + 4 * pad, None)
    P.assert_same_bits(only, d2)


def test_calls_of_different_sizes_on_one_context_and_another_stream():
    ctx = _native.Context(0)
    k = 3

    def call(n):
        x = torch.from_numpy(cloud(str(n))).to(DEV)
        d2 = torch.empty((n, k), dtype=torch.float32, device=DEV)
        idx = torch.empty((n, k), dtype=torch.int32, device=DEV)
        raw_call(ctx.handle, x, None, n, k, d2.data_ptr(), idx.data_ptr())
        return d2, idx

    big, small = 64 * L + 1, L + 1
    first = call(big)
    assert_equal(tuple(t.cpu().numpy() for t in first), reference(str(big)), k, "first call")
    second = call(small)                         # the work memory still holds the larger call's tail
    assert_equal(tuple(t.cpu().numpy() for t in second), reference(str(small)), k, "smaller call after a larger one")
    again = call(big)
    P.assert_same_bits(again[0], first[0])
    P.assert_same_bits(again[1], first[1])
    bytes_before = _native.lib().gs_ctx_device_bytes(ctx.handle)
    assert bytes_before >= big * 40              # the work memory is the context's and is counted
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = call(big)
    side.synchronize()
    P.assert_same_bits(other[0], first[0])
    P.assert_same_bits(other[1], first[1])
    assert _native.lib().gs_ctx_device_bytes(ctx.handle) == bytes_before          # steady state: nothing grows


def test_a_query_between_forward_and_backward_leaves_the_gradients_alone():
    s = synth(2000, 128, 96, 0.08, sh_deg=3, seed=0)
    q, t = view_pose(1, 3)
    x = torch.from_numpy(cloud(str(64 * L + 1))).to(DEV)
    grads = []
    for with_query in (False, True):
        module = P.module()
        inp = P.make_input(s, q, t)
        image = module(inp, keep_frame=True)[0]
        g = 2.0 * (image.detach() - 0.5)
        if with_query:
            d2 = torch.empty((len(x), 3), dtype=torch.float32, device=DEV)
            raw_call(module._ctx_for(torch.device(DEV)), x, None, len(x), 3, d2.data_ptr(), None)
        image.backward(g)
        grads.append((inp.point_cloud.grad.clone(), inp.point_cloud_features.grad.clone()))
        if with_query:
            assert_equal((d2.cpu().numpy(), reference(str(len(x)))[1][:, :3]), reference(str(len(x))), 3, "the query itself")
    assert grads[0][1].abs().max() > 0
    P.assert_same_bits(grads[0][0], grads[1][0], "grad_pointcloud")
    P.assert_same_bits(grads[0][1], grads[1][1], "grad_pointcloud_features")


@pytest.mark.parametrize("name", list(CLOUDS))
def test_mean_neighbour_distance(name):
    x = cloud(name)
    got = knn.mean_neighbour_distance(torch.from_numpy(x).to(DEV)).cpu().numpy().astype(np.float64)
    want = knn_ref.mean_distance(x, 3)
    assert got.shape == want.shape and ((got == 0) == (want == 0)).all()
    nz = want > 0
    rel = np.abs(got[nz] - want[nz]) / want[nz]
    print(f"{name}: largest relative error of the mean 3-NN distance {rel.max():.3e}")
    assert rel.max() < 1e-6


def test_python_surface():
    x = torch.from_numpy(cloud("100")).to(DEV)
    d2 = knn.nearest_neighbours(x)
    assert isinstance(d2, torch.Tensor) and d2.shape == (100, 3) and d2.dtype == torch.float32 and d2.device == x.device
    d2b, idx = knn.nearest_neighbours(x, 3, return_indices=True)
    assert idx.dtype == torch.int32 and idx.shape == (100, 3)
    P.assert_same_bits(d2, d2b)
    # a float64 point cloud, a bool mask and a strided view are converted, not refused
    mask = torch.zeros(100, dtype=torch.bool, device=DEV)
    mask[::3] = True
    wide = torch.zeros(100, 4, dtype=torch.float64, device=DEV)
    wide[:, :3] = x
    got = knn.nearest_neighbours(wide[:, :3], 3, mask, return_indices=True)
    m8 = np.zeros(100, np.int8)
    m8[::3] = 1
    assert_equal(tuple(t.cpu().numpy() for t in got), knn_ref.knn(cloud("100"), 8, m8), 3, "converted inputs")
    empty = knn.nearest_neighbours(torch.zeros(0, 3, device=DEV), 2, return_indices=True)
    assert empty[0].shape == (0, 2) and empty[1].shape == (0, 2)


# ---- every k, +inf pairs, subnormal distances, identical points -------------------------------------------------------------
EVERY_K = [("4097", None), ("lattice", None), ("copies", None), ("overflow", None), ("overflow", "fifth"), ("identical", None),
           ("uniform", "garbage")]


@pytest.mark.parametrize("k", range(1, 9))
@pytest.mark.parametrize("name,mask_name", EVERY_K)
def test_every_k(name, mask_name, k):
    """k = 4 is an instantiation of its own; 2, 5, 6 and 7 store fewer columns than theirs keeps"""
    x, mask = masked(name, mask_name)
    assert_equal(gpu(x, k, mask), reference(name, mask_name), k, (name, mask_name, k))


@pytest.mark.parametrize("k", range(1, 9))
def test_every_k_writes_its_block_and_nothing_else(k):
    """through the raw call, outputs inside sentinel-filled buffers, with the rows and with idx_out = NULL"""
    n, pad = 64 * L + 1, 257
    x = torch.from_numpy(cloud(str(n))).to(DEV)
    ctx = _native.Context(0)
    d2 = torch.full((n * k + 2 * pad,), -7.5, dtype=torch.float32, device=DEV)
    idx = torch.full((n * k + 2 * pad,), -77, dtype=torch.int32, device=DEV)
    only = torch.full_like(d2, -7.5)
    raw_call(ctx.handle, x, None, n, k, d2.data_ptr() + 4 * pad, idx.data_ptr() + 4 * pad)
    raw_call(ctx.handle, x, None, n, k, only.data_ptr() + 4 * pad, None)
    for buf, sentinel in ((d2, -7.5), (idx, -77), (only, -7.5)):
        assert (buf[:pad] == sentinel).all() and (buf[-pad:] == sentinel).all()
        assert not (buf[pad:-pad] == sentinel).any()
    got = d2[pad:-pad].reshape(n, k).cpu().numpy(), idx[pad:-pad].reshape(n, k).cpu().numpy()
    assert_equal(got, reference(str(n)), k, (n, k))
    P.assert_same_bits(only, d2)


def test_the_overflow_cloud_has_every_kind_of_row():
    """On the reference, before any GPU result.  Of the (300, 8) entries, bare / with every fifth row masked: 394 / 333 are at
    +inf and carry a row, in 58 / 53 rows; 15 / 18 rows hold finite pairs first and +inf pairs behind them; 242 / 187 rows are
    all finite; 0 / 480 entries are the -1 tail (60 masked rows).  No NaN anywhere."""
    for mask_name, want in ((None, (394, 58, 15, 242, 0)), ("fifth", (333, 53, 18, 187, 480))):
        d2, idx = reference("overflow", mask_name)
        assert not np.isnan(d2).any()
        far = np.isinf(d2) & (idx >= 0)
        assert (np.isinf(d2) | (idx >= 0)).all() and (np.isfinite(d2) <= (idx >= 0)).all()
        mixed = np.isfinite(d2).any(axis=1) & far.any(axis=1)
        got = (int(far.sum()), int(far.any(axis=1).sum()), int(mixed.sum()), int(np.isfinite(d2).all(axis=1).sum()), int((idx < 0).sum()))
        assert got == want, (mask_name, got)
        assert (far.all(axis=1)).any() and mixed.any() and np.isfinite(d2).all(axis=1).any()
        rows = np.arange(len(idx))[:, None]
        assert not (idx == rows).any()                       # never the row itself
        part = knn_ref.takes_part(*masked("overflow", mask_name))
        for r in np.flatnonzero(far.any(axis=1))[:20]:       # pairs at +inf: ascending rows, and the smallest rows that are left
            rest = np.setdiff1d(np.flatnonzero(part), np.concatenate([idx[r][~far[r]], [r]]))
            assert idx[r][far[r]].tolist() == rest[:far[r].sum()].tolist()


@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("mask_name", [None, "fifth"])
def test_pairs_at_infinity_come_with_their_rows(mask_name, k):
    x, mask = masked("overflow", mask_name)
    assert_equal(gpu(x, k, mask), reference("overflow", mask_name), k, ("overflow", mask_name, k))


def test_the_subnormal_cloud_is_what_it_says():
    """Its 8-NN squared distances: all below the smallest normal f32 (the largest is 7.9e-43), 8 exactly zero, 392 distinct
    values, 719 ties between neighbours of one row; no coordinate is itself subnormal."""
    x = cloud("subnormal")
    d2, idx = reference("subnormal")
    tiny = np.finfo(np.float32).tiny
    assert (d2 < tiny).all() and d2.max() > 7e-43
    assert int((d2 == 0).sum()) == 8
    assert len(np.unique(d2)) == 392
    assert int((np.diff(d2, axis=1) == 0).sum()) == 719
    assert not ((np.abs(x) < tiny) & (x != 0)).any()


@pytest.mark.parametrize("k", [3, 8])
def test_subnormal_distances_are_kept(k):
    """flushed to zero, every distance here would be 0 and every row's neighbours the first rows of the cloud"""
    assert_equal(gpu(cloud("subnormal"), k), reference("subnormal"), k, ("subnormal", k))


@pytest.mark.parametrize("k", [3, 8])
def test_identical_points(k):
    """every key has the same digit in every pass of the sort, every distance is 0: the k smallest other rows"""
    d2, idx = reference("identical")
    assert (d2 == 0).all() and idx[3].tolist() == [0, 1, 2, 4, 5, 6, 7, 8] and idx[4999].tolist() == list(range(8))
    assert_equal(gpu(cloud("identical"), k), reference("identical"), k, ("identical", k))


# ---- past one block of a tree level and two trips of the digit scan ------------------------------------------------------------
#   rows     leaves                 tree   levels of more than 256 nodes   sort blocks -> trips of the 1024-word scan
#   32 833   513 full + one row     1024   512                             33 -> 9
#   65 537   1025                   2048   1024 and 512                    65 -> 17     (the right half of the tree: empty boxes)
BIG = {"32833": None, "big_clusters": "half_garbage"}


@functools.lru_cache(maxsize=None)
def big(name):
    """-> the cloud and its mask on the device, a sample of rows (512 that ask and 64 that do not, random with a fixed seed,
    every outlier, the rows holding the six extreme coordinates of the box) with their numpy reference, and torch_knn on the
    device for all rows, k = 8 once: the first k columns serve the smaller k"""
    x, mask = masked(name, BIG[name])
    part = knn_ref.takes_part(x, mask)
    clean = np.isfinite(x).all(axis=1) & (np.abs(x).max(axis=1) < 1e29)             # (neither NaN nor 1e30)
    centre = np.median(x[part], axis=0)
    outliers = np.flatnonzero(clean & (np.abs(np.where(clean[:, None], x, 0.0) - centre).max(axis=1) > 1e3))
    live = np.flatnonzero(part)
    extremes = live[np.concatenate([x[live].argmin(axis=0), x[live].argmax(axis=0)])]
    rng = np.random.default_rng(7)
    rest = np.flatnonzero(~part)
    rows = np.unique(np.concatenate([rng.choice(live, 512, replace=False), rng.choice(rest, min(64, rest.size), replace=False),
                                     outliers, extremes]))
    xd = torch.from_numpy(x).to(DEV)
    md = None if mask is None else torch.from_numpy(mask).to(DEV)
    return dict(x=x, mask=mask, part=part, outliers=outliers, rows=rows, numpy=knn_ref.knn(x, 8, mask, rows=rows), xd=xd, md=md,
                torch=knn_ref.torch_knn(xd, 8, md))


@pytest.mark.parametrize("name", list(BIG))
def test_big_clouds_reach_the_code_they_are_for(name):
    b = big(name)
    n = len(b["x"])
    leaves = -(-n // L)
    tree = 1 << (leaves - 1).bit_length()
    blocks = -(-n // 1024)
    trips = -(-blocks * 256 // 1024)
    assert (n, leaves, tree, trips) == {"32833": (32833, 514, 1024, 9), "big_clusters": (65537, 1025, 2048, 17)}[name]
    assert tree // 2 > 256 and trips > 2
    assert b["part"][b["rows"]].sum() >= 512
    if name == "big_clusters":
        # rows that take no part sort behind the others: the 1025th leaf is theirs, so the right half of the tree is empty boxes,
        # and more than 300 leaves hold no asking row at all
        asking_leaves = -(-int(b["part"].sum()) // L)
        assert asking_leaves <= 1024 and leaves - asking_leaves > 300
        out = ~b["part"]
        garbage = ~np.isfinite(b["x"]).all(axis=1) | (b["x"] == 1e30).any(axis=1)
        assert int(out.sum()) == 21846 and int(garbage.sum()) == 10924 and not garbage[b["part"]].any()
        assert np.isnan(b["x"]).any() and (b["x"] == 1e30).any()
        far = b["outliers"]
        assert (len(far), int(b["part"][far].sum())) == (13, 12) and np.isin(far, b["rows"]).all()      # (3 of the 16 hold garbage now)
        extent = np.ptp(b["x"][b["part"]], axis=0).max()
        assert extent > 1e5                              # the box is four decades wider than the clusters


@pytest.mark.parametrize("name", list(BIG))
def test_the_device_reference_equals_numpy_on_a_sample_of_rows(name):
    """The reference's own check at this size, on this device: a failure here is torch_knn's, not gs_knn's."""
    b = big(name)
    rows = torch.from_numpy(b["rows"]).to(DEV)
    got = tuple(t[rows].cpu().numpy() for t in b["torch"])
    assert not np.isnan(b["numpy"][0]).any()
    assert_equal(got, b["numpy"], 8, ("REFERENCE FAILURE: torch_knn on the device differs from numpy", name))


@pytest.mark.parametrize("k", [1, 3, 4, 8])
@pytest.mark.parametrize("name", list(BIG))
def test_big_clouds_equal_the_device_reference_on_every_row(name, k):
    b = big(name)
    n = len(b["x"])
    d2 = torch.full((n, k), -7.5, dtype=torch.float32, device=DEV)
    idx = torch.full((n, k), -77, dtype=torch.int32, device=DEV)
    raw_call(_native.shared_ctx(torch.device(DEV)), b["xd"], b["md"], n, k, d2.data_ptr(), idx.data_ptr())
    assert not (d2 == -7.5).any() and not (idx == -77).any(), "a row was not written"
    want = b["torch"][0][:, :k], b["torch"][1][:, :k]
    bad = (d2.view(torch.int32) != want[0].view(torch.int32)) | (idx != want[1])
    assert not bad.any(), (name, k, int(bad.sum()), torch.nonzero(bad)[:4].tolist())
