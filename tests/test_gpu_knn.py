"""GPU (-m gpu): gs_knn (include/gs_knn.h) against brute force in the same f32 arithmetic (tests/knn_ref.py): the squared
distances BIT-IDENTICAL and the neighbour rows EQUAL, at every size around a leaf (L = 64 rows) and around a complete tree, on
clouds whose distances tie, repeat and span eleven orders of magnitude, with masked and non-finite rows, through interior
pointers, across calls of different sizes on one context, on another stream, and between a forward and its backward."""
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


def lattice():
    g = np.arange(16, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def copies():
    x = np.tile(np.array([[0.3, -1.7, 2.9]], np.float32), (302, 1))
    x[100] = (0.3, -1.7, 3.0)
    x[301] = (5.0, 5.0, 5.0)
    return x


EXTRA = {"lattice": lattice, "copies": copies}


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
    x = cloud(name).copy()
    n = len(x)
    if mask_name is None:
        return x, None
    mask = np.zeros(n, np.int8)
    if mask_name == "third":
        mask[::3] = 1
    elif mask_name == "all":
        mask[:] = 1
    elif mask_name == "garbage":                 # invalid rows hold NaN and 1e30: they must not move anything
        mask[::3] = 1
        x[::6] = np.nan
        x[3::6] = 1e30
    elif mask_name == "nan_row":                 # a VALID row with one NaN coordinate (and one with an infinite one)
        x[17, 1] = np.nan
        x[40, 2] = np.inf
    return x, mask


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
@pytest.mark.parametrize("name", list(CLOUDS) + list(EXTRA))
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
