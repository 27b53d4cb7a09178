"""GPU (-m gpu): exchange.pack_rows / exchange.merge_rows (gs_pack_rows, gs_merge_rows) bit for bit against the numpy
statement of their contracts (tests/exchange_ref.py), and end to end behind the real operator: three views packed, merged
and stepped with FusedAdam.step(rows=union) against the sequential dense sum.

Sizes: N = 5000 rows (five workgroups of the tag compaction, the last one partial); unions of 1023, 1024, 1025 and 2049 rows
(one compaction workgroup less one, full, plus one; two plus one); one case at N = 70 000, where the compaction runs 69
workgroups and every scatter workgroup past the 64th adds up the totals before it over more than one wave of its loop.
Counts stay below list_stride throughout, and the rows behind every count hold poison ids (-1, N + 5, copies of listed ids)
and NaN payloads that must never be read."""
import functools

import numpy as np
import pytest
import torch

import exchange_ref as X
import parity_util as P
from taichi_3d_gaussian_splatting_amd import _native, exchange, sparse
from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
from taichi_3d_gaussian_splatting_amd.synthetic import view_pose

pytestmark = pytest.mark.gpu
DEV = P.DEV
N = 5000
NAN_BITS = 0x7FC12345          # a quiet NaN with a payload: what untouched memory is pre-filled with
SPARE = 8


def _dev_words(a):
    """a uint32 numpy array as a float32 device tensor of the same bits"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(DEV).view(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _special_values(rng, ids, which):
    """(len(ids), 59) f32 for list number `which`: normal values with -0.0, +0.0 and denormals sprinkled in (places that differ
    from list to list, so they meet ordinary values in the sums) and infinities whose place and sign depend on (id, column)
    only, so that no sum is inf - inf (the payload of a generated NaN is not part of the contract)."""
    ids = np.asarray(ids, np.int64)
    v = rng.standard_normal((len(ids), 59)).astype(np.float32)
    col = np.arange(59, dtype=np.int64)[None, :]
    h = (ids[:, None] * 7919 + col * 104729 + which * 611953) % 50
    v[h == 0] = np.float32(-0.0)
    v[h == 1] = np.float32(0.0)
    den = rng.choice(np.array([1e-40, -1e-40, 1.4e-45, -3e-39], np.float32), size=v.shape)
    v[h == 2] = den[h == 2]
    g = (ids[:, None] * 31 + col * 17) % 97
    v[g == 0] = np.float32(np.inf)
    v[g == 1] = np.float32(-np.inf)
    return v


def _rows_of(ids, values):
    rows = np.zeros((len(ids), 60), np.uint32)
    rows[:, :59] = np.ascontiguousarray(values, np.float32).view(np.uint32)
    rows[:, 59] = np.asarray(ids, np.int32).view(np.uint32)
    return rows


class _Case:
    """n_lists packed lists at one stride, poison behind every count, on the host (uint32) and what goes to the device"""

    def __init__(self, n, id_lists, seed, edit=None):
        rng = np.random.default_rng(seed)
        self.n = n
        self.lists = [_rows_of(ids, _special_values(rng, ids, l)) for l, ids in enumerate(id_lists)]
        if edit is not None:
            edit(self.lists)
        self.counts = np.array([len(r) for r in self.lists], np.int32)
        self.stride = int(self.counts.max()) + 5
        self.packed = np.full((len(self.lists), self.stride, 60), NAN_BITS, np.uint32)
        every = np.concatenate([np.asarray(i, np.int64) for i in id_lists] + [np.array([0], np.int64)])
        for l, rows in enumerate(self.lists):
            self.packed[l, :len(rows)] = rows
            pad = self.stride - len(rows)
            poison = np.array([-1, n + 5, every[l % len(every)], every[-1], every[l % len(every)]], np.int64)
            self.packed[l, len(rows):, 59] = np.resize(poison, pad).astype(np.int32).view(np.uint32)

    def reference(self):
        gf, gp = np.full((self.n, 56), NAN_BITS, np.uint32).view(np.float32), np.full((self.n, 3), NAN_BITS, np.uint32).view(np.float32)
        union = X.merge(self.lists, self.n, gf, gp)
        return union, gf.view(np.uint32), gp.view(np.uint32)

    def run(self):
        """gs_merge_rows called directly, every output pre-filled -> (union ids buffer with SPARE entries behind the capacity,
        count, feature bits, position bits)"""
        exchange._bind()
        cap = min(self.n, len(self.lists) * self.stride)
        packed, counts = _dev_words(self.packed), torch.from_numpy(self.counts).to(DEV)
        out = _dev_words(np.full(59 * self.n, NAN_BITS, np.uint32))
        ids = torch.full((cap + SPARE,), -7, dtype=torch.int32, device=DEV)
        count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        gf, gp = out[:56 * self.n].view(self.n, 56), out[56 * self.n:].view(self.n, 3)
        _native.call("gs_merge_rows", packed.device, _native.shared_ctx(packed.device), packed.data_ptr(), counts.data_ptr(), len(self.lists),
                     self.stride, self.n, gf.data_ptr(), gp.data_ptr(), ids.data_ptr(), cap, count.data_ptr())
        return ids.cpu().numpy(), int(count.item()), _bits(gf), _bits(gp)

    def check(self, want_union_size=None):
        union, ref_gf, ref_gp = self.reference()
        if want_union_size is not None:
            assert union.size == want_union_size
        ids, count, gf, gp = self.run()
        assert count == union.size
        assert np.array_equal(ids[:count], union) and (np.diff(ids[:count]) > 0).all()
        assert (ids[count:] == -7).all()                                       # nothing at or beyond the count is written
        assert np.array_equal(gf, ref_gf) and np.array_equal(gp, ref_gp)        # union rows: the reference's bits; the others: the pre-fill
        out = np.setdiff1d(np.arange(self.n), union)
        assert (gf[out] == NAN_BITS).all() and (gp[out] == NAN_BITS).all()
        again = self.run()
        assert again[1] == count and np.array_equal(again[0], ids) and np.array_equal(again[2], gf) and np.array_equal(again[3], gp)
        return union


# ----------------------------------------------------------------------------------------------------------------------
# pack

@functools.lru_cache(maxsize=None)
def _dense_gradients(seed, n=N):
    """(N,56) and (N,3) f32 with the special values of _special_values; computed once per seed and never written"""
    rng = np.random.default_rng(seed)
    v = _special_values(rng, np.arange(n), 0)
    return np.ascontiguousarray(v[:, :56]), np.ascontiguousarray(v[:, 56:])


def _raw_pack(gf, gp, ids, count, max_count, n=N):
    """gs_pack_rows called directly into a buffer of max_count + SPARE rows pre-filled with NAN_BITS -> its bits"""
    exchange._bind()
    out = _dev_words(np.full((max_count + SPARE, 60), NAN_BITS, np.uint32))
    ids_t = torch.from_numpy(np.asarray(ids, np.int32)).to(DEV)
    count_t = torch.tensor([count], dtype=torch.int32, device=DEV)
    _native.call("gs_pack_rows", gf.device, _native.shared_ctx(gf.device), gf.data_ptr(), gp.data_ptr(), n, ids_t.data_ptr(),
                 count_t.data_ptr(), max_count, out.data_ptr())
    return _bits(out)


def _listed(rng, count, n=N):
    """`count` ascending ids with 0 and n - 1 among them (from two on), then seven valid ids behind the count"""
    if count >= 2:
        ids = np.concatenate([[0], np.sort(rng.choice(np.arange(1, n - 1), count - 2, replace=False)), [n - 1]])
    else:
        ids = np.array([17][:count], np.int64)
    return np.concatenate([ids, rng.choice(n, 7)]).astype(np.int32)


@pytest.mark.parametrize("count", [0, 1, 15, 1023, 1024, 1025])
def test_pack_rows_against_the_reference(count):
    gf, gp = _dense_gradients(1)
    ids = _listed(np.random.default_rng(count), count)
    got = _raw_pack(_dev_words(gf.view(np.uint32)), _dev_words(gp.view(np.uint32)), ids, count, count + 7)
    assert np.array_equal(got[:count], X.pack(gf, gp, ids[:count]))
    assert (got[count:] == NAN_BITS).all()                                     # rows at and beyond the count are not written
    if count >= 2:
        assert X.ids_of(got[:count])[0] == 0 and X.ids_of(got[:count])[-1] == N - 1


def test_pack_rows_bad_ids_and_a_count_above_the_bound():
    gf, gp = _dense_gradients(2)
    d_gf, d_gp = _dev_words(gf.view(np.uint32)), _dev_words(gp.view(np.uint32))
    ids = np.array([-2, 0, 40, N - 1, N, N + 3, 2 ** 31 - 1, 41, 42], np.int32)
    got = _raw_pack(d_gf, d_gp, ids, 7, 20)
    want = X.pack(gf, gp, ids[:7])
    assert X.ids_of(want).tolist() == [-1, 0, 40, N - 1, -1, -1, -1] and not want[[0, 4, 5, 6], :59].any()
    assert np.array_equal(got[:7], want) and (got[7:] == NAN_BITS).all()
    # *count above max_count: the host's bound holds
    got = _raw_pack(d_gf, d_gp, ids, 9, 3)
    assert np.array_equal(got[:3], X.pack(gf, gp, ids[:3])) and (got[3:] == NAN_BITS).all()
    # a negative count packs nothing
    assert (_raw_pack(d_gf, d_gp, ids, -4, 5) == NAN_BITS).all()


@pytest.mark.parametrize("offset_floats", [4, 1], ids=["aligned16", "aligned4"])
def test_pack_rows_from_views_inside_a_larger_allocation(offset_floats):
    """offset 16 bytes: the 16-byte loads; offset 4 bytes: the source is not 16-byte aligned and the kernel loads floats"""
    gf, gp = _dense_gradients(3)
    big_f = torch.zeros(56 * N + 64, device=DEV)
    big_p = torch.zeros(3 * N + 64, device=DEV)
    v_gf = big_f[offset_floats:offset_floats + 56 * N].view(N, 56)
    v_gp = big_p[offset_floats:offset_floats + 3 * N].view(N, 3)
    v_gf.view(torch.int32).copy_(_dev_words(gf.view(np.uint32)).view(torch.int32))
    v_gp.view(torch.int32).copy_(_dev_words(gp.view(np.uint32)).view(torch.int32))
    assert v_gf.data_ptr() % 16 == (4 * offset_floats) % 16
    ids = _listed(np.random.default_rng(5), 300)
    got = _raw_pack(v_gf, v_gp, ids, 300, 310)
    assert np.array_equal(got[:300], X.pack(gf, gp, ids[:300])) and (got[300:] == NAN_BITS).all()
    # the wrapper on the same views: a PackedRows that shares the list's count
    rows = sparse.TouchedRows(torch.from_numpy(ids).to(DEV), torch.tensor(300, dtype=torch.int32, device=DEV), N, 305)
    p = exchange.pack_rows(v_gp, v_gf, rows)
    assert p.count is rows.count and p.max_count == 305 and p.n_points == N and tuple(p.data.shape) == (305, 60)
    assert np.array_equal(_bits(p.data)[:300], got[:300])
    # out=: straight into a slice of a (n_lists, list_stride, 60) buffer, nothing written behind the count or in the other slice
    both = _dev_words(np.full((2, 400, 60), NAN_BITS, np.uint32))
    p = exchange.pack_rows(v_gp, v_gf, rows, out=both[1])
    assert p.data.data_ptr() == both[1].data_ptr() and p.max_count == 305
    assert np.array_equal(_bits(both[1])[:300], got[:300]) and (_bits(both[1])[300:] == NAN_BITS).all() and (_bits(both[0]) == NAN_BITS).all()
    with pytest.raises(ValueError):
        exchange.pack_rows(v_gp, v_gf, rows, out=both[1, :304])


# ----------------------------------------------------------------------------------------------------------------------
# merge

def _subset(rng, pool, size):
    return np.sort(rng.choice(pool, size, replace=False))


def _id_lists(kind, n_lists, rng, n=N):
    size = max(8, min(700, 2400 // n_lists))
    if kind == "disjoint":
        perm = rng.permutation(n)
        return [np.sort(perm[l * size:(l + 1) * size]) for l in range(n_lists)]
    if kind == "identical":
        ids = _subset(rng, n, size)
        return [ids.copy() for _ in range(n_lists)]
    if kind == "nested":                 # list l + 1 is a subset of list l; the innermost keeps at least one row
        lists = [_subset(rng, n, 700)]
        for _ in range(n_lists - 1):
            lists.append(_subset(rng, lists[-1], max(1, int(len(lists[-1]) * 0.8))))
        return lists
    return [_subset(rng, n, int(rng.integers(1, 2 * size))) for _ in range(n_lists)]       # random overlap


@pytest.mark.parametrize("n_lists", [1, 2, 3, 8, 64])
@pytest.mark.parametrize("kind", ["disjoint", "identical", "nested", "random"])
def test_merge_rows_against_the_reference(kind, n_lists):
    rng = np.random.default_rng(1000 * n_lists + len(kind))
    id_lists = _id_lists(kind, n_lists, rng)
    id_lists[0] = np.unique(np.concatenate([[0, N - 1], id_lists[0]]))          # the first and the last row of the tensors
    union = _Case(N, id_lists, seed=n_lists).check()
    assert union[0] == 0 and union[-1] == N - 1


@pytest.mark.parametrize("n_lists", [1, 3, 64])
def test_merge_rows_with_empty_lists(n_lists):
    rng = np.random.default_rng(n_lists)
    nothing = np.zeros(0, np.int64)
    assert _Case(N, [nothing] * n_lists, seed=1).check(want_union_size=0).size == 0      # all empty: union count 0, nothing written
    if n_lists > 1:
        id_lists = [_subset(rng, N, 300) for _ in range(n_lists)]
        id_lists[n_lists // 2] = nothing
        id_lists[0] = nothing
        _Case(N, id_lists, seed=2).check()


@pytest.mark.parametrize("size", [1023, 1024, 1025, 2049])
def test_merge_rows_union_sizes_across_the_compaction_blocks(size):
    rng = np.random.default_rng(size)
    union = _subset(rng, N, size)
    owner = rng.integers(0, 3, size)
    also = rng.random((3, size)) < 0.3
    id_lists = [union[(owner == l) | also[l]] for l in range(3)]
    _Case(N, id_lists, seed=size).check(want_union_size=size)


def test_merge_rows_past_64_compaction_blocks():
    n = 70000
    rng = np.random.default_rng(70)
    id_lists = [np.unique(np.concatenate([[0, 65536, n - 1], _subset(rng, n, 1500)])), _subset(rng, n, 900), _subset(rng, np.arange(66000, n), 700)]
    union = _Case(n, id_lists, seed=70).check()
    assert -(-n // sparse.COMPACT_BLOCK) > 64 and union[-1] == n - 1 and (union > 64 * sparse.COMPACT_BLOCK).sum() > 500


def test_merge_rows_skips_bad_id_words_inside_a_count():
    """-1 (what gs_pack_rows leaves for a bad id) and other ids outside [0, N), at the head, in the middle (alone and in a run) and
    at the tail of a list: skipped, and the rows around them are still found"""
    rng = np.random.default_rng(8)
    id_lists = [_subset(rng, N, 400), _subset(rng, N, 400), _subset(rng, N, 50)]

    def edit(lists):
        bad = np.array([-1, -1, N, N + 5, -2 ** 31, 2 ** 31 - 1], np.int64).astype(np.int32).view(np.uint32)
        lists[0][[0, 7, 200, 201, 202, 399], 59] = bad
        lists[1][[100], 59] = bad[:1]
        lists[2][:, 59] = bad[0]                                               # a list of skipped rows only
    case = _Case(N, id_lists, seed=8, edit=edit)
    union = case.check()
    kept = np.concatenate([np.delete(id_lists[0], [0, 7, 200, 201, 202, 399]), np.delete(id_lists[1], [100])])
    assert np.array_equal(union, np.unique(kept))


def test_merge_rows_order_is_list_order():
    """(1e8 + -1e8) + 1 = 1 in list order, 0 in any order that adds the last two first; -0.0 alone stays -0.0"""
    vals = [np.float32(1e8), np.float32(-1e8), np.float32(1.0)]
    case = _Case(N, [np.array([5, 9])] * 3 + [np.array([4])], seed=0)
    for l, v in enumerate(vals):
        case.packed[l, :2, :59] = np.full(59, v, np.float32).view(np.uint32)
    case.packed[3, :1, :59] = 0x80000000
    case.lists = [case.packed[l, :c].copy() for l, c in enumerate(case.counts)]
    case.check(want_union_size=3)
    _, _, gf, gp = case.run()
    assert (gf[[5, 9]].view(np.float32) == 1.0).all() and (gp[[5, 9]].view(np.float32) == 1.0).all()
    assert (gf[4] == 0x80000000).all() and (gp[4] == 0x80000000).all()


def test_merge_rows_wrapper_zero_and_out():
    rng = np.random.default_rng(4)
    case = _Case(N, [_subset(rng, N, 300), _subset(rng, N, 200)], seed=4)
    union, ref_gf, ref_gp = case.reference()
    packed, counts = _dev_words(case.packed), torch.from_numpy(case.counts).to(DEV)
    gp, gf, rows = exchange.merge_rows(packed, counts, N, zero=True)
    assert isinstance(rows, sparse.TouchedRows) and rows.n_points == N and rows.max_count == min(N, 2 * case.stride) and rows.count.dim() == 0
    assert np.array_equal(rows.tensor().cpu().numpy(), union)
    out = np.setdiff1d(np.arange(N), union)
    b_gf, b_gp = _bits(gf), _bits(gp)
    assert not b_gf[out].any() and not b_gp[out].any()                          # zero=True: zeros outside the union
    assert np.array_equal(b_gf[union], ref_gf[union]) and np.array_equal(b_gp[union], ref_gp[union])
    # the two gradients are views of one flat [features | positions] buffer
    from taichi_3d_gaussian_splatting_amd.distributed import _flat_base
    flat = _flat_base(gp, gf)
    assert flat is not None and flat.data_ptr() == gf.data_ptr() and flat.shape[0] == 59 * N
    # out=: rows outside the union keep the caller's bits; zero=True clears them first
    mine = _dev_words(np.full(59 * N, NAN_BITS, np.uint32))
    gp2, gf2, rows2 = exchange.merge_rows(packed, counts, N, out=mine)
    assert gf2.data_ptr() == mine.data_ptr() and np.array_equal(_bits(gf2), ref_gf) and np.array_equal(_bits(gp2), ref_gp)
    exchange.merge_rows(packed, counts, N, out=mine, zero=True)
    assert np.array_equal(_bits(gf2), b_gf) and np.array_equal(_bits(gp2), b_gp)
    # no rows at all: an empty union without a launch
    gp0, gf0, rows0 = exchange.merge_rows(packed[:, :0], counts, N)
    assert rows0.max_count == 0 and int(rows0.count.item()) == 0
    gp0, gf0, rows0 = exchange.merge_rows(packed, counts, 0)
    assert rows0.max_count == 0 and int(rows0.count.item()) == 0 and tuple(gf0.shape) == (0, 56)
    with pytest.raises(RuntimeError, match=r"gs_merge_rows failed \(-1\).*n_lists"):
        exchange.merge_rows(torch.zeros(65, 2, 60, device=DEV), torch.zeros(65, dtype=torch.int32, device=DEV), N)


# ----------------------------------------------------------------------------------------------------------------------
# end to end: operator -> lists -> packed rows -> merge -> selective step

def test_three_views_packed_merged_and_stepped_against_the_dense_sum():
    from test_gpu_multiprocess import H_IMG, N_PTS, W_IMG, _grad_of_image, _input, _scene
    s = _scene()
    got = {}
    module = P.module(hook=lambda h: got.update(ids=h.point_id_in_camera_list.clone(), npix=h.num_affected_pixels.clone()))
    module.track_touched_rows = True
    q, t = view_pose(0, 3)
    inp = _input(s, 0, N_PTS, DEV, q, t, requires_grad=True)
    packed_lists, dense, touched = [], None, []
    for v in range(3):
        q, t = view_pose(v, 3)
        inp.q_pointcloud_camera, inp.t_pointcloud_camera = torch.tensor(q, device=DEV), torch.tensor(t, device=DEV)
        inp.point_cloud.grad = inp.point_cloud_features.grad = None
        img = module(inp)[0]
        img.backward(_grad_of_image(img.detach()))
        gp, gf = inp.point_cloud.grad, inp.point_cloud_features.grad
        packed_lists.append(exchange.pack_rows(gp, gf, module.last_touched_rows))
        touched.append(got["ids"][got["npix"] > 0].cpu().numpy())
        dense = (gp.clone(), gf.clone()) if dense is None else (dense[0] + gp, dense[1] + gf)      # (g0 + g1) + g2
    packed, counts = exchange.stack_packed(packed_lists)
    assert packed.shape[0] == 3 and packed.shape[1] == max(p.max_count for p in packed_lists)
    m_gp, m_gf, union = exchange.merge_rows(packed, counts, N_PTS)
    want = np.unique(np.concatenate(touched))
    rows = union.tensor().cpu().numpy()
    print(f"N {N_PTS}, touched per view {[len(x) for x in touched]}, union {rows.size}, image {W_IMG}x{H_IMG}")
    assert 0 < want.size < N_PTS and all(0 < len(x) < want.size for x in touched)
    assert np.array_equal(rows, want)                                       # the rows where any view's num_affected_pixels > 0
    idx = torch.from_numpy(want).to(DEV).long()
    assert bool((m_gp[idx] == dense[0][idx]).all()) and bool((m_gf[idx] == dense[1][idx]).all())
    out = torch.from_numpy(np.setdiff1d(np.arange(N_PTS), want)).to(DEV).long()
    assert not _bits(dense[0][out]).any() and not _bits(dense[1][out]).any()    # the dense sum is zero on every other row
    # the selective step on the merged buffer leaves what it leaves on the dense sum, bit for bit
    results = []
    for g_pc, g_ft in ((m_gp, m_gf), dense):
        pc, ft = inp.point_cloud.detach().clone(), inp.point_cloud_features.detach().clone()
        pc.grad, ft.grad = g_pc, g_ft
        opt = FusedAdam([pc, ft], lr=1e-2)
        for _ in range(2):
            opt.step(rows=union)
        results.append([pc, ft] + [st[k] for st in opt.state for k in ("exp_avg", "exp_avg_sq")])
    for a, b in zip(*results):
        P.assert_same_bits(a, b)
    assert not torch.equal(results[0][1], inp.point_cloud_features.detach())
