"""GPU (-m gpu): the touched-row list (gs_touched_rows) against the CPU oracle's backward of the same scene, the
row-selective Adam step (gs_adam_step_rows, FusedAdam.step(rows=...)) against tests/sparse_ref.RowAdam64 and against the dense
kernel, and the two wired together behind the operator (track_touched_rows).

The compaction has one level: a single workgroup and one launch up to sparse.COMPACT_BLOCK in-camera points, a count launch
and a scatter launch (every workgroup adds up the totals before it) beyond.  The 32x32 scenes and block_edges take the first
shape, tiny-3000 (three workgroups, the last one partial) and dense_corner (26) the second.  Every scatter workgroup adds up the
totals before it with a 256-thread strided loop, which takes a second trip beyond 256 workgroups: the large frame of
parity_util (293), checked against the hook payload of the same backward because no CPU backward is needed for it."""
import functools

import numpy as np
import pytest
import torch

import parity_util as P
from oracle import oracle
from sparse_ref import RowAdam64
from taichi_3d_gaussian_splatting_amd import _native, sparse
from taichi_3d_gaussian_splatting_amd.optim import FusedAdam
from taichi_3d_gaussian_splatting_amd.synthetic import synth, view_pose

pytestmark = pytest.mark.gpu
DEV = P.DEV
# |p - p64| <= ADAM_C S + 4 ulp(p), S = sum over steps of lr_t |m_hat / (sqrt(v_hat) + eps)|: form and value of
# tests/test_gpu_loss_kernels.py:35-39 (three times the largest use measured for the dense kernel at 28e6 elements and 200
# steps); the row-selective kernel is the same arithmetic element for element, so the same bar holds it
ADAM_C = 3e-3


# ----------------------------------------------------------------------------------------------------------------------
# the list

def _cases():
    d = {}
    for kind, arg in P.SCENES[:3]:
        d[f"{kind}-{arg[0]}"] = functools.partial(P.scene_case, kind, arg)
    d["dense_corner"] = lambda: (P.dense_corner_scene(), *view_pose(), 0)
    d["block_edges"] = lambda: (P.block_edges_scene(64, 64, 0.3), *view_pose(), 0)
    d["tiny-3000"] = lambda: P.tiny_case(5, 3000, 0.1, 64)
    return d


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _oracle_list(name):
    """-> (scene, q, t, partial, M, the oracle's ascending list of rows with num_affected_pixels > 0); computed once per scene"""
    s, q, t, partial = CASES[name]()
    return (s, q, t, partial) + _oracle_rows(s, q, t, partial)


def _oracle_rows(s, q, t, partial):
    cfg = oracle.default_config(allow_partial_tiles=int(partial))
    f, _ = P.run_oracle(s, q, t, cfg)
    b = oracle.backward(f, np.ones((s.height, s.width, 3), np.float32), 3, cfg)       # the count does not depend on the upstream
    rows = np.sort(f.point_id_in_camera_list[b["num_affected_pixels"] > 0]).astype(np.int32)
    return int(f.M), rows


def _fwd_bwd(module, s, q, t, depth=False, seed=3):
    """One forward and backward of the operator with a random upstream (and, with depth, one on rasterized_depth: gs_backward_ex)"""
    inp = P.make_input(s, q, t, 3)
    outs = module(inp)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    loss = (outs[0] * torch.randn(outs[0].shape, device=DEV, generator=gen)).sum()
    if depth:
        loss = loss + (outs[1] * torch.randn(outs[1].shape, device=DEV, generator=gen)).sum()
    loss.backward()
    return inp


def _raw_list(frame, capacity=None):
    """gs_touched_rows called directly, into buffers prefilled with -1 (eight spare entries behind the capacity) -> (ids, count)"""
    sparse._bind()
    cap = frame.n_points_in_camera if capacity is None else capacity
    ids = torch.full((cap + 8,), -1, dtype=torch.int32, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    _native.call("gs_touched_rows", frame.device, frame._context.handle, frame.handle, ids.data_ptr(), cap, count.data_ptr())
    return ids.cpu().numpy(), int(count.item())


def _tracking(partial=False, depth=False):
    module = P.module(partial=partial, depth=depth)
    module.track_touched_rows = True
    return module


@pytest.mark.parametrize("name", list(CASES))
def test_list_equals_the_oracles(name):
    s, q, t, partial, M, want = _oracle_list(name)
    N = s.point_cloud.shape[0]
    if name == "dense_corner":           # saturated pixels hide points: in-camera rows that are not listed exist
        assert 0 < want.size < M, (want.size, M)
    if name == "tiny-3000":
        assert M > 2 * sparse.COMPACT_BLOCK and M % 64 != 0, M
    print(f"{name}: N {N}, M {M}, touched {want.size}, compaction workgroups {-(-M // sparse.COMPACT_BLOCK)}")
    module = _tracking(partial)
    inp = _fwd_bwd(module, s, q, t)
    frame = module.last_frame
    assert frame.n_points_in_camera == M
    if name == "tiny-3000":
        assert frame.n_points_in_camera > 2 * sparse.COMPACT_BLOCK and frame.n_points_in_camera % 64 != 0
    rows = module.last_touched_rows
    assert rows.n_points == N and rows.max_count == M and rows.ids.shape[0] >= M and rows.count.dim() == 0
    assert np.array_equal(rows.tensor().cpu().numpy(), want)
    ids, count = _raw_list(frame)
    assert count == want.size
    assert np.array_equal(ids[:count], want)
    assert (ids[count:] == -1).all()                                     # nothing at or beyond the count is written
    assert (np.diff(ids[:count]) > 0).all()                               # strictly ascending
    # every row outside the list has all-zero bits in both dense gradients
    out = np.setdiff1d(np.arange(N), want)
    gp, gf = inp.point_cloud.grad.cpu().numpy(), inp.point_cloud_features.grad.cpu().numpy()
    assert not gp[out].view(np.uint32).any() and not gf[out].view(np.uint32).any()
    assert gf[want].any(axis=1).all()                                     # (and the listed rows do carry a gradient)
    # a second run on the same module, and a fresh module, give the same bits
    _fwd_bwd(module, s, q, t)
    again = _raw_list(module.last_frame)
    fresh = _tracking(partial)
    _fwd_bwd(fresh, s, q, t)
    other = _raw_list(fresh.last_frame)
    for got in (again, other):
        assert got[1] == count and np.array_equal(got[0], ids)
    # gs_backward_ex (a depth gradient arrives) leaves the same list
    deep = _tracking(partial, depth=True)
    _fwd_bwd(deep, s, q, t, depth=True)
    assert np.array_equal(deep.last_touched_rows.tensor().cpu().numpy(), want)
    got = _raw_list(deep.last_frame)
    assert got[1] == count and np.array_equal(got[0], ids)


def test_list_past_one_trip_of_the_sum_of_earlier_blocks():
    s, q, t, partial = P.tiny_case(*P.LARGE_FRAME)
    N = s.point_cloud.shape[0]
    got = {}
    module = P.module(partial, hook=lambda h: got.update(ids=h.point_id_in_camera_list.clone(), npix=h.num_affected_pixels.clone()))
    module.track_touched_rows = True
    inp = _fwd_bwd(module, s, q, t)
    frame = module.last_frame
    M = frame.n_points_in_camera
    blocks = -(-M // sparse.COMPACT_BLOCK)
    assert M > 262144 and blocks > 256, (M, blocks)
    assert got["ids"].shape[0] == got["npix"].shape[0] == M
    want = got["ids"][got["npix"] > 0].cpu().numpy()
    print(f"N {N}, M {M}, touched {want.size}, compaction workgroups {blocks}")
    assert 0 < want.size < M
    assert bool((got["npix"][256 * sparse.COMPACT_BLOCK:] > 0).any())      # workgroups past the 256th own entries of the list
    rows = module.last_touched_rows
    assert rows.n_points == N and rows.max_count == M
    assert np.array_equal(rows.tensor().cpu().numpy(), want)
    ids, count = _raw_list(frame)
    assert count == want.size
    assert np.array_equal(ids[:count], want)
    assert (ids[count:] == -1).all()                                     # nothing at or beyond the count is written
    assert (np.diff(ids[:count]) > 0).all()                               # strictly ascending
    out = np.setdiff1d(np.arange(N), want)
    gp, gf = inp.point_cloud.grad.cpu().numpy(), inp.point_cloud_features.grad.cpu().numpy()
    assert not gp[out].view(np.uint32).any() and not gf[out].view(np.uint32).any()
    assert gf[want].any(axis=1).all()


def _one_visible():
    return synth(1, 32, 32, 0.3, seed=0)


def _behind():
    s = synth(300, 32, 32, 0.3, seed=4)
    s.point_cloud[:, 2] *= -1.0
    return s


def _all_invalid():
    s = synth(300, 32, 32, 0.3, seed=4)
    s.point_invalid_mask[:] = 1
    return s


@pytest.mark.parametrize("make,want", [(_behind, []), (_all_invalid, []), (_one_visible, [0])], ids=["behind", "invalid", "one"])
def test_empty_and_degenerate_frames(make, want):
    s = make()
    q, t = view_pose()
    module = _tracking()
    inp = _fwd_bwd(module, s, q, t)
    assert module.last_frame.n_points_in_camera == len(want)
    rows = module.last_touched_rows
    assert rows.max_count == len(want) and rows.tensor().cpu().tolist() == want
    ids, count = _raw_list(module.last_frame)
    assert count == len(want) and ids[:count].tolist() == want and (ids[count:] == -1).all()
    if not want:
        assert not inp.point_cloud.grad.cpu().numpy().view(np.uint32).any()
        assert not inp.point_cloud_features.grad.cpu().numpy().view(np.uint32).any()


def test_no_list_without_point_gradients():
    """a backward with want_points=False (only the pose requires grad) stores None"""
    s, q, t, partial = P.scene_case(*P.SCENES[0])
    module = _tracking(partial)
    _fwd_bwd(module, s, q, t)
    assert module.last_touched_rows is not None
    inp = P.make_input(s, q, t, 3, requires_grad=False, pose=True)
    module(inp)[0].sum().backward()
    assert module.last_touched_rows is None
    assert P.module().last_touched_rows is None and P.module().track_touched_rows is False


# ----------------------------------------------------------------------------------------------------------------------
# state: error returns

def test_state_errors():
    s, q, t, partial = P.scene_case(*P.SCENES[0])
    module = P.module(partial=partial)
    inp_a = P.make_input(s, q, t, 3)
    img_a = module(inp_a)[0]
    frame_a = module.last_frame
    with pytest.raises(RuntimeError, match=r"\(-4\).*no backward has run"):                 # GS_ERR_STATE
        _raw_list(frame_a)
    with pytest.raises(RuntimeError, match=r"gs_frame_heavy_tiles failed \(-4\)"):
        frame_a.heavy_tiles()
    t_b = t.copy()
    t_b[0, 0] += 0.3
    inp_b = P.make_input(s, q, t_b, 3)
    img_b = module(inp_b)[0]
    frame_b = module.last_frame
    img_a.sum().backward()
    ids_a, count_a = _raw_list(frame_a)
    assert count_a > 0 and frame_a.heavy_tiles() >= 0
    with pytest.raises(RuntimeError, match=r"\(-1\).*capacity"):                            # GS_ERR_INVALID_ARGUMENT
        _raw_list(frame_a, capacity=frame_a.n_points_in_camera - 1)
    img_b.sum().backward()
    with pytest.raises(RuntimeError, match=r"\(-4\).*another backward"):
        _raw_list(frame_a)
    ids_b, count_b = _raw_list(frame_b)
    want_b = _oracle_rows(s, q, t_b, partial)[1]
    assert count_b == want_b.size and np.array_equal(ids_b[:count_b], want_b)
    frame_b.release()
    with pytest.raises(RuntimeError, match=r"\(-4\).*not a live frame"):
        sparse._bind()
        _native.call("gs_touched_rows", frame_b.device, frame_b._context.handle, frame_b._stale, ids_b.ctypes.data, 0, ids_b.ctypes.data)


# ----------------------------------------------------------------------------------------------------------------------
# the step, on synthetic tensors

N_ROWS, GUARD = 1000, 8


def _guarded(row_len, gen=None, fill=None):
    """(N_ROWS, row_len) f32 as the head of an allocation with GUARD more rows behind it -> (tensor, guard rows, their copy)"""
    whole = torch.empty(N_ROWS + GUARD, row_len, device=DEV)
    if gen is not None:
        whole.copy_(torch.randn(whole.shape, device=DEV, generator=gen))
    else:
        whole.fill_(0.0 if fill is None else fill)
    whole[N_ROWS:] = 12345.0
    return whole[:N_ROWS], whole[N_ROWS:], whole[N_ROWS:].clone()


class _Setup:
    """A parameter, its gradient and both moments, each with guard rows, under a FusedAdam"""

    def __init__(self, row_len, seed, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.gen = torch.Generator(device=DEV).manual_seed(seed)
        self.row_len = row_len
        self.p, *gp = _guarded(row_len, self.gen)
        self.g, *gg = _guarded(row_len, self.gen)
        self.opt = FusedAdam([self.p], lr=lr, betas=betas, eps=eps)
        m, *gm = _guarded(row_len)
        v, *gv = _guarded(row_len)
        self.opt.state[0]["exp_avg"], self.opt.state[0]["exp_avg_sq"] = m, v
        self.guards = [gp, gg, gm, gv]
        self.p.grad = self.g

    def tensors(self):
        st = self.opt.state[0]
        return self.p, st["exp_avg"], st["exp_avg_sq"]

    def new_grad(self, scale=1.0):
        self.g.copy_(torch.randn(self.g.shape, device=DEV, generator=self.gen) * scale)

    def check_guards(self):
        for now, before in self.guards:
            assert torch.equal(now, before), "a guard row behind a tensor was written"


def _rows(listed, capacity=N_ROWS, max_count=None, pad=None):
    """TouchedRows of the ascending rows `listed`; entries beyond the count hold `pad` rows (valid ids a kernel that ignored the
    count would update) or -1"""
    listed = torch.as_tensor(listed, dtype=torch.int32).reshape(-1)
    ids = torch.full((capacity,), -1, dtype=torch.int32)
    ids[:listed.numel()] = listed
    if pad is not None:
        pad = torch.as_tensor(pad, dtype=torch.int32)[:capacity - listed.numel()]
        ids[listed.numel():listed.numel() + pad.numel()] = pad
    return sparse.TouchedRows(ids.to(DEV), torch.tensor(listed.numel(), dtype=torch.int32, device=DEV), N_ROWS,
                              capacity if max_count is None else max_count)


def _ulp(x):
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def _check_against(p, ref, what):
    err = (p.double() - ref.p).abs() - 4 * _ulp(ref.p)
    pos = ref.S > 0
    assert bool((err[~pos] <= 0).all()), f"{what}: a parameter without any update moved"
    used = (err[pos] / ref.S[pos]).max().item() if bool(pos.any()) else 0.0
    print(f"{what}: largest |p - p64| - 4 ulp over S = {used:.3g} (bar {ADAM_C})")
    assert used <= ADAM_C, (what, used)


def _dense_copy(su, step=None):
    """A FusedAdam on copies of su's parameter, gradient and moments, at su's step count"""
    p = su.p.clone()
    p.grad = su.g.clone()
    opt = FusedAdam([p], lr=su.opt.lr, betas=su.opt.betas, eps=su.opt.eps)
    st = su.opt.state[0]
    opt.state[0].update(step=st["step"] if step is None else step, exp_avg=st["exp_avg"].clone(), exp_avg_sq=st["exp_avg_sq"].clone())
    return opt


@pytest.mark.parametrize("row_len", [56, 3])
def test_step_over_all_rows_is_the_dense_step_bit_for_bit(row_len):
    su = _Setup(row_len, seed=row_len)
    rows = _rows(torch.arange(N_ROWS))
    for it in range(5):
        su.new_grad(scale=10.0 ** (it - 2))
        dense = _dense_copy(su)
        dense.step()
        su.opt.step(rows=rows)
        for a, b in zip(su.tensors(), (dense.params[0], dense.state[0]["exp_avg"], dense.state[0]["exp_avg_sq"])):
            P.assert_same_bits(a, b, (row_len, it))
        assert su.opt.state[0]["step"] == dense.state[0]["step"] == it + 1
    su.check_guards()


@pytest.mark.parametrize("row_len", [56, 3])
def test_step_random_tenth_of_the_rows_against_float64(row_len):
    su = _Setup(row_len, seed=100 + row_len)
    ref = RowAdam64(su.p)
    cpu = torch.Generator().manual_seed(5)
    scale = torch.exp(torch.randn(N_ROWS, row_len, device=DEV, generator=su.gen) * 2)
    lr = 1e-3
    for it in range(30):
        perm = torch.randperm(N_ROWS, generator=cpu)
        listed, others = perm[:100].sort().values, perm[100:]
        su.new_grad()
        su.g.mul_(scale)
        before = [x.clone() for x in su.tensors()]
        # the count (100) is below max_count (300), and the entries behind it name rows that must not be updated
        su.opt.step(rows=_rows(listed, max_count=300, pad=others))
        ref.step(su.g, lr, listed)
        keep = others.to(DEV)
        for now, was in zip(su.tensors(), before):
            P.assert_same_bits(now[keep], was[keep], it)
            assert not torch.equal(now[listed.to(DEV)], was[listed.to(DEV)])
        lr *= 0.97
        su.opt.lr = lr
    assert su.opt.state[0]["step"] == ref.t == 30
    _check_against(su.p, ref, f"random tenth, row_len {row_len}")
    su.check_guards()


@pytest.mark.parametrize("row_len", [56, 3])
def test_step_with_an_empty_list_changes_nothing_but_the_step_count(row_len):
    su = _Setup(row_len, seed=200 + row_len)
    ref = RowAdam64(su.p)
    before = [x.clone() for x in su.tensors()]
    su.opt.step(rows=_rows([], max_count=100, pad=torch.arange(N_ROWS)))
    ref.step(su.g, su.opt.lr, [])
    for now, was in zip(su.tensors(), before):
        P.assert_same_bits(now, was)
    assert su.opt.state[0]["step"] == 1
    su.opt.step(rows=sparse.TouchedRows(torch.empty(0, dtype=torch.int32, device=DEV), torch.zeros((), dtype=torch.int32, device=DEV), N_ROWS, 0))
    assert su.opt.state[0]["step"] == 2                                    # max_count == 0: no launch at all
    for now, was in zip(su.tensors(), before):
        P.assert_same_bits(now, was)
    su.opt.state[0]["step"] = 1
    # the following step over every row is step 2 of the reference, and the dense step 2 on untouched moments bit for bit
    dense = _dense_copy(su)
    dense.step()
    su.opt.step(rows=_rows(torch.arange(N_ROWS)))
    ref.step(su.g, su.opt.lr, torch.arange(N_ROWS))
    assert su.opt.state[0]["step"] == ref.t == 2
    P.assert_same_bits(su.p, dense.params[0])
    _check_against(su.p, ref, f"after an empty list, row_len {row_len}")
    su.check_guards()


@pytest.mark.parametrize("row_len", [56, 3])
def test_step_single_first_and_last_row(row_len):
    su = _Setup(row_len, seed=300 + row_len)
    ref = RowAdam64(su.p)
    for row in (0, N_ROWS - 1):
        before = [x.clone() for x in su.tensors()]
        dense = _dense_copy(su)
        dense.step()
        su.opt.step(rows=_rows([row], max_count=1, pad=[5, 6, 7]))
        ref.step(su.g, su.opt.lr, [row])
        rest = torch.arange(N_ROWS, device=DEV) != row
        for now, was, full in zip(su.tensors(), before, (dense.params[0], dense.state[0]["exp_avg"], dense.state[0]["exp_avg_sq"])):
            P.assert_same_bits(now[rest], was[rest], row)
            P.assert_same_bits(now[row], full[row], row)                  # the row itself: what the dense step gives it
            assert not torch.equal(now[row], was[row])
    _check_against(su.p, ref, f"single rows, row_len {row_len}")
    su.check_guards()


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)], ids=["b0.9_0.999", "b0.5_0.9"])
def test_step_extreme_gradients_match_torch_f32_on_the_listed_rows(betas):
    """Gradients of +-1e20 and +-1e-30 on the listed rows against f32 torch.optim.Adam(foreach=False) on those rows alone, as
    test_adam_extreme_gradients_match_torch_f32 holds the dense kernel: the same elements are infinite, NaN, zero and finite in
    the parameter and both moments, the finite ones within 1e-4 (not closer: 1 - beta2 is taken from the f32 beta2 here)."""
    su = _Setup(56, seed=31, betas=betas)
    listed = torch.arange(0, N_ROWS, 2)
    dev_listed = listed.to(DEV)
    rows = _rows(listed, pad=torch.arange(1, N_ROWS, 2))
    base = torch.randn(listed.numel(), 56, device=DEV, generator=su.gen)
    kinds = torch.tensor([1e20, -1e20, 1e-30, -1e-30, 0.0, 1.0], device=DEV).repeat(listed.numel() * 56 // 6 + 1)[:listed.numel() * 56]
    kinds = kinds.view(listed.numel(), 56)
    pa = su.p[dev_listed].clone().requires_grad_(True)
    ref = torch.optim.Adam([pa], lr=1e-3, betas=betas, eps=1e-8, foreach=False)
    before = [x.clone() for x in su.tensors()]
    for t in range(10):
        g = kinds * (1.0 + 0.5 * base.abs() * (t % 3))
        g = torch.where(kinds == 1.0, (base.abs() + 0.1) * (t + 1), g)
        su.g.fill_(3.0)                                                    # rows not listed: a gradient that is never read
        su.g[dev_listed] = g
        pa.grad = g.clone()
        ref.step()
        su.opt.step(rows=rows)
    st = ref.state[pa]
    unlisted = torch.arange(1, N_ROWS, 2, device=DEV)
    for name, a, b, was in zip(("param", "exp_avg", "exp_avg_sq"), (pa.detach(), st["exp_avg"], st["exp_avg_sq"]), su.tensors(), before):
        P.assert_same_bits(b[unlisted], was[unlisted], name)
        b = b[dev_listed]
        for cls in (torch.isinf, torch.isnan, lambda x: x == 0):
            assert torch.equal(cls(a), cls(b)), name
        fin = torch.isfinite(a) & (a != 0)
        assert bool(((a[fin] - b[fin]).abs() <= 1e-4 * a[fin].abs() + 1e-9).all()), (name, (a[fin] - b[fin]).abs().max().item())
    su.check_guards()


def test_step_refuses_a_parameter_of_another_row_count():
    p = torch.zeros(N_ROWS, 3, device=DEV)
    other = torch.zeros(N_ROWS + 1, 56, device=DEV)
    p.grad, other.grad = torch.ones_like(p), torch.ones_like(other)
    opt = FusedAdam([p, other])
    with pytest.raises(ValueError, match="rows"):
        opt.step(rows=_rows([1, 2]))
    assert not p.any() and [st["step"] for st in opt.state] == [0, 0]      # refused before anything was updated
    other.grad = None                                                       # a parameter without a gradient is not looked at
    opt.step(rows=_rows([1, 2]))
    assert p[1:3].all() and not p[0].any() and not p[3:].any()


# ----------------------------------------------------------------------------------------------------------------------
# end to end: operator -> list -> step

def test_operator_list_and_selective_step_over_three_poses():
    s, q, t, partial = P.tiny_case(7, 200, 0.15, 32)
    N = s.point_cloud.shape[0]
    module = _tracking(partial)
    pc = torch.tensor(s.point_cloud, device=DEV, requires_grad=True)
    feat = torch.tensor(s.point_cloud_features, device=DEV, requires_grad=True)
    pc0 = pc.detach().clone()
    control = feat.detach().clone()          # the forward normalises the quaternions of in-camera rows in place: a control copy
    opt = FusedAdam([pc, feat], lr=1e-3)     # sees the same three forwards and no optimiser
    static = P.make_input(s, q, t, 3, requires_grad=False)
    gen = torch.Generator(device=DEV).manual_seed(17)
    lists = []
    for it, dx in enumerate((0.0, 0.6, -0.6)):
        t_it = t.copy()
        t_it[0, 0] += dx
        now = type(s)(pc.detach().cpu().numpy(), feat.detach().cpu().numpy(), s.point_invalid_mask, s.point_object_id,
                      s.camera_intrinsics, s.height, s.width)
        lists.append(_oracle_rows(now, q, t_it, partial)[1])
        tq, tt = torch.tensor(q, device=DEV), torch.tensor(t_it, device=DEV)
        opt.zero_grad()
        inp = P.Rast.GaussianPointCloudRasterisationInput(
            point_cloud=pc, point_cloud_features=feat, point_object_id=static.point_object_id,
            point_invalid_mask=static.point_invalid_mask, camera_info=static.camera_info, q_pointcloud_camera=tq,
            t_pointcloud_camera=tt, color_max_sh_band=3)
        img = module(inp)[0]
        (img * torch.randn(img.shape, device=DEV, generator=gen)).sum().backward()
        with torch.no_grad():
            P.module(partial=partial)(P.Rast.GaussianPointCloudRasterisationInput(
                point_cloud=pc0, point_cloud_features=control, point_object_id=static.point_object_id,
                point_invalid_mask=static.point_invalid_mask, camera_info=static.camera_info, q_pointcloud_camera=tq,
                t_pointcloud_camera=tt, color_max_sh_band=3))
        rows = module.last_touched_rows
        assert np.array_equal(rows.tensor().cpu().numpy(), lists[-1]), it
        before = (pc.detach().clone(), feat.detach().clone())
        if it == 1:
            # rows listed in step 1 and not in step 2: the selective step leaves them alone; the dense step, on copies of the
            # same state, moves them (their moments of step 1 are not zero)
            gone = torch.tensor(np.setdiff1d(lists[0], lists[1]), device=DEV, dtype=torch.long)
            assert gone.numel() > 0
            dense_p = [pc.detach().clone(), feat.detach().clone()]
            for d, p in zip(dense_p, (pc, feat)):
                d.grad = p.grad.clone()
            dense = FusedAdam(dense_p, lr=1e-3)
            for dst, src in zip(dense.state, opt.state):
                dst.update(step=src["step"], exp_avg=src["exp_avg"].clone(), exp_avg_sq=src["exp_avg_sq"].clone())
            dense.step()
            assert (dense_p[0][gone] != before[0][gone]).any(dim=1).all() and (dense_p[1][gone] != before[1][gone]).any(dim=1).all()
        opt.step(rows=rows)
        out = torch.tensor(np.setdiff1d(np.arange(N), lists[-1]), device=DEV, dtype=torch.long)
        listed = torch.tensor(lists[-1], device=DEV, dtype=torch.long)
        for now_t, was in zip((pc, feat), before):
            P.assert_same_bits(now_t[out], was[out], it)
            assert (now_t[listed] != was[listed]).any(dim=1).all(), it
        if it == 1:
            P.assert_same_bits(pc[gone], before[0][gone])
            P.assert_same_bits(feat[gone], before[1][gone])
    never = np.setdiff1d(np.arange(N), np.concatenate(lists))
    assert never.size > 0
    P.assert_same_bits(pc[never], pc0[never])
    P.assert_same_bits(feat[never], control[never])
    assert [st["step"] for st in opt.state] == [3, 3]


def test_training_with_the_selective_step_reduces_the_loss():
    """test_training_step_with_fused_loss_and_adam_reduces_loss with the row-selective step, 60 iterations at 64x64; that
    test's own criterion"""
    from taichi_3d_gaussian_splatting_amd import CameraInfo
    from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction
    s = synth(2000, 64, 64, 0.1, seed=9)
    q, t = view_pose()
    pc = torch.tensor(s.point_cloud, device=DEV, requires_grad=True)
    feat = torch.tensor(s.point_cloud_features, device=DEV, requires_grad=True)
    mask, obj = torch.tensor(s.point_invalid_mask, device=DEV), torch.tensor(s.point_object_id, device=DEV)
    rast = P.Rast(P.Rast.GaussianPointCloudRasterisationConfig())
    rast.track_touched_rows = True
    lf = LossFunction(LossFunction.LossFunctionConfig())
    opt_f, opt_p = FusedAdam([feat], lr=1e-3), FusedAdam([pc], lr=1e-5)
    target = torch.rand(3, 64, 64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    cam = CameraInfo(torch.tensor(s.camera_intrinsics, device=DEV), 64, 64, 0)
    tq, tt = torch.tensor(q, device=DEV), torch.tensor(t, device=DEV)
    losses = []
    for it in range(60):
        opt_f.zero_grad(); opt_p.zero_grad()
        img, _, _ = rast(P.Rast.GaussianPointCloudRasterisationInput(
            point_cloud=pc, point_cloud_features=feat, point_object_id=obj, point_invalid_mask=mask, camera_info=cam,
            q_pointcloud_camera=tq, t_pointcloud_camera=tt, color_max_sh_band=3))
        img = torch.clamp(img, 0, 1).permute(2, 0, 1)
        L, L1, LD = lf(img, target, point_invalid_mask=mask, pointcloud_features=feat)
        L.backward()
        rows = rast.last_touched_rows
        opt_f.step(rows=rows); opt_p.step(rows=rows)
        losses.append(L.item())
    print(f"loss {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert losses[-1] < losses[0]
