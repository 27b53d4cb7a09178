"""GPU (-m gpu): the pose corrections (include/gs_pose_table.h, pose_table.py) against tests/pose_table_ref.py: compose equal
to the float64 restatement rounded to float32 or one ulp off it (the device's float64 sin and cos need not be numpy's), the
all-zero views bit for bit, the backward within the project's per-element gradient bar; at one view, a wave minus, exactly and
plus one view and more than a block, with one and with three object rows, and with every class of |w| in every batch."""
import functools

import numpy as np
import pytest
import torch

import pose_table_ref as ref
from taichi_3d_gaussian_splatting_amd import pose_table
from taichi_3d_gaussian_splatting_amd.LossFunction import LossFunction

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VS, KS = [1, 63, 64, 65, 257], [1, 3]
ROOT_S = float(np.sqrt(ref.SERIES_S))
# |w| of a view: exact 0 (all six floats zero), 0 with a translation, 1e-9, either side of the series threshold, 1e-3, 1,
# pi - 1e-3, 4; then the view whose floats are not finite
THETAS = [0.0, 0.0, 1e-9, ROOT_S * (1 - 1e-5), ROOT_S * (1 + 1e-5), 1e-3, 1.0, np.pi - 1e-3, 4.0]
ZERO, NAN = 0, len(THETAS)
CLASSES = len(THETAS) + 1
SENTINEL = 7.0
ADAM_C = 3e-3                       # tests/test_gpu_loss_kernels.py: |p - p64| <= ADAM_C S + 4 ulp(p)


def test_the_shapes_are_the_ones_the_kernels_change_path_at():
    T = pose_table.THREADS
    assert VS == [1, 63, 64, 65, T + 1] and KS == [1, 3]
    s = [np.float64(np.float32(th)) ** 2 for th in THETAS]
    assert s[3] < ref.SERIES_S <= s[4] and s[2] < ref.SERIES_S < s[5]      # float32 keeps them on their sides of the threshold


@functools.lru_cache(maxsize=None)
def case(V, K, first_class=0):
    """inputs and references of a shape, computed once"""
    rng = np.random.default_rng(1000 * V + 10 * K + first_class)
    classes = [(v + first_class) % CLASSES for v in range(V)]
    axis = rng.normal(size=(V, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    delta = np.zeros((V, 6), dtype=np.float32)
    for v, c in enumerate(classes):
        if c == NAN:
            delta[v] = rng.normal(0.0, 0.1, 6)
            delta[v, rng.integers(0, 6)] = [np.nan, np.inf, -np.inf][v % 3]
        else:
            delta[v, :3] = axis[v] * THETAS[c]
            if c != ZERO:
                delta[v, 3:] = rng.normal(0.0, 0.3, 3)
            elif v % 2:
                delta[v, [1, 4]] = -0.0                                      # -0 is zero
    q = rng.normal(size=(V, K, 4))
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    q[::3] *= rng.uniform(0.7, 1.4, (len(q[::3]), 1, 1))                     # quaternions that are not of unit length, as stored
    q, t = q.astype(np.float32), rng.normal(0.0, 2.0, (V, K, 3)).astype(np.float32)
    q[0, 0, 0], t[0, 0, 2] = -0.0, -0.0                                      # a zero view keeps the sign of a zero
    c = dict(classes=classes, delta=delta, q=q, t=t, gq=rng.normal(size=(V, K, 4)).astype(np.float32),
             gt=rng.normal(size=(V, K, 3)).astype(np.float32), reg=0.125)
    c["q_out"], c["t_out"] = ref.compose(delta, q, t)
    c["grad"] = {reg: ref.backward(delta, q, c["gq"], c["gt"], reg) for reg in (0.0, c["reg"])}
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def batches(V, K):
    """every class goes in every batch: a batch of at least CLASSES views holds them all; one view is run once per class"""
    return [case(V, K, first) for first in range(CLASSES)] if V < CLASSES else [case(V, K)]


def dev(a):
    return torch.tensor(np.asarray(a), device=DEV)


def bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("V", VS)
def test_compose_against_the_reference(V, K):
    differing = total = 0
    seen = set()
    for c in batches(V, K):
        seen.update(c["classes"])
        delta, q, t = dev(c["delta"]), dev(c["q"]), dev(c["t"])
        q_out, t_out = torch.full_like(q, SENTINEL), torch.full_like(t, SENTINEL)
        pose_table.compose_forward(q, t, delta, q_out=q_out, t_out=t_out)
        for got, want, base in ((q_out, c["q_out"], c["q"]), (t_out, c["t_out"], c["t"])):
            got = got.cpu().numpy()
            apart = ref.ulps_apart(got, want)
            assert apart.max() <= 1, (V, K, int(apart.max()))
            mask = np.array([cl not in (ZERO, NAN) for cl in c["classes"]])
            differing += int((apart[mask] != 0).sum())
            total += int(apart[mask].size)
            for v, cl in enumerate(c["classes"]):
                if cl == ZERO:
                    assert np.array_equal(got[v].view(np.uint32), base[v].view(np.uint32)), v      # the base rows, bit for bit
                if cl == NAN:
                    assert np.isnan(got[v]).all(), v                                               # its own view, and no other:
            assert np.isfinite(got[[cl != NAN for cl in c["classes"]]]).all()                     # every other view is finite
        # the same bits on a second run, into fresh tensors, and in place
        q2, t2 = pose_table.compose_forward(q, t, delta)
        assert np.array_equal(bits(q2), bits(q_out)) and np.array_equal(bits(t2), bits(t_out))
        q3, t3 = q.clone(), t.clone()
        pose_table.compose_forward(q3, t3, delta, q_out=q3, t_out=t3)
        assert np.array_equal(bits(q3), bits(q_out)) and np.array_equal(bits(t3), bits(t_out))
    assert seen == set(range(CLASSES))
    print(f"compose V={V} K={K}: {differing} of {total} values one float32 ulp off the reference ({100.0 * differing / max(total, 1):.4f} %)")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("V", VS)
def test_backward_against_the_reference(V, K):
    for c in batches(V, K):
        delta, q, gq, gt = dev(c["delta"]), dev(c["q"]), dev(c["gq"]), dev(c["gt"])
        finite = np.array([cl != NAN for cl in c["classes"]])
        results = {}
        for reg in (0.0, c["reg"]):
            out = torch.full((V, 6), float("nan") if reg else SENTINEL, device=DEV)        # garbage: written, not added
            assert pose_table.compose_backward(q, delta, gq, gt, reg, grad_delta=out) is out
            want, magnitude = c["grad"][reg]
            got = out.cpu().numpy()
            if finite.any():
                ok, worst = ref.within_bar(got[finite], want[finite], magnitude[finite])
                print(f"grad_delta V={V} K={K} reg={reg}: {worst:.3f} of the bar")
                assert ok, (reg, worst)
            assert (~np.isfinite(got[~finite])).any(axis=1).all()                           # a non-finite view poisons its own gradient only
            again = pose_table.compose_backward(q, delta, gq, gt, reg)
            assert np.array_equal(bits(again), bits(out))                                   # the same bits on every run
            results[reg] = got
        # reg adds reg * delta, in float64 before the one rounding: against zero upstream gradients it is all there is
        alone = pose_table.compose_backward(q, delta, torch.zeros_like(gq), torch.zeros_like(gt), c["reg"]).cpu().numpy()
        product = (np.float64(c["reg"]) * c["delta"].astype(np.float64)).astype(np.float32)
        assert np.array_equal(alone[finite], product[finite])
        step = results[c["reg"]][finite].astype(np.float64) - results[0.0][finite].astype(np.float64)
        ulp = np.spacing(np.maximum(np.abs(results[c["reg"]][finite]), np.abs(results[0.0][finite]))).astype(np.float64)
        # (three roundings: of either result, half an ulp each, and of the product, at most one ulp of the larger result)
        assert (np.abs(step - product[finite]) <= 2.0 * ulp).all()


def test_table_step_moves_one_row_like_adam(tmp_path):
    V, v = 5, 2
    config = pose_table.PoseRefinementConfig(num_iterations=40, start_iteration=4)
    table = pose_table.PoseTable(V, DEV, config)
    assert not bool(table.delta.any()) and table.steps == [0] * V
    gen = torch.Generator(device=DEV).manual_seed(9)
    table.delta.add_(torch.randn(V, 6, device=DEV, generator=gen) * 0.01)
    table.grad.copy_(torch.randn(V, 6, device=DEV, generator=gen))                 # other rows hold gradients too: they are not used
    before = {name: getattr(table, name).clone() for name in ("delta", "exp_avg", "exp_avg_sq")}
    p64 = table.delta[v].double().clone().requires_grad_(True)
    adam = torch.optim.Adam([p64], lr=config.lr, betas=config.betas, eps=config.eps)
    S = torch.zeros(6, dtype=torch.float64, device=DEV)
    iterations = [4, 7, 8, 20, 39]                                                   # the view comes up now and then
    for step, iteration in enumerate(iterations, 1):
        g = torch.randn(6, device=DEV, generator=gen) * torch.tensor([1.0, 1e-3, 10.0] * 2, device=DEV)
        table.grad[v] = g
        table.step(v, iteration)
        assert table.steps[v] == step
        for group in adam.param_groups:
            group["lr"] = ref.lr_at(iteration, config.lr, config.lr_final, config.num_iterations, config.start_iteration)
        p64.grad = g.double()
        last = p64.detach().clone()
        adam.step()
        S += (p64.detach() - last).abs()
    others = [i for i in range(V) if i != v]
    for name, tensor in before.items():
        assert torch.equal(getattr(table, name)[others], tensor[others]), name
        assert not torch.equal(getattr(table, name)[v], tensor[v]), name
    assert table.steps == [0, 0, 5, 0, 0]
    a = p64.detach().abs().float()
    ulp = (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()
    err = (table.delta[v].double() - p64.detach()).abs() - 4 * ulp
    used = (err / S).max().item()
    print(f"table step: {used / ADAM_C:.3f} of the Adam bar")
    assert bool((S > 0).all()) and used <= ADAM_C
    # all views in one launch: the direct call, and (V,4) poses like (V,1,4)
    q = torch.nn.functional.normalize(torch.randn(V, 3, 4, device=DEV, generator=gen), dim=2)
    t = torch.randn(V, 3, 3, device=DEV, generator=gen)
    qc, tc = table.corrected(q, t)
    want_q, want_t = pose_table.compose_forward(q, t, table.delta)
    assert torch.equal(qc, want_q) and torch.equal(tc, want_t) and not qc.requires_grad
    q1, t1 = table.corrected(q[:, 0], t[:, 0])
    assert q1.shape == (V, 4) and torch.equal(q1, want_q[:, 0]) and torch.equal(t1, want_t[:, 0])
    # save / load
    paths = [f"images/view_{i}.png" for i in range(V)]
    table.save(str(tmp_path / "poses.pt"), paths)
    loaded, loaded_paths = pose_table.PoseTable.load(str(tmp_path / "poses.pt"), DEV)
    assert loaded_paths == paths and loaded.steps == table.steps and loaded.num_views == V
    for name in before:
        assert torch.equal(getattr(loaded, name), getattr(table, name)), name
    assert torch.equal(loaded.by_image_path(paths)["images/view_2.png"], table.delta[v])
    with pytest.raises(ValueError, match="image paths"):
        table.save(str(tmp_path / "bad.pt"), paths[:-1])
    with pytest.raises(IndexError):
        table.row(V)


def test_autograd_through_the_rasteriser_and_the_loss_equals_the_direct_calls():
    from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast
    from taichi_3d_gaussian_splatting_amd.synthetic import scene_input, synth, view_pose
    import dataclasses
    H, W = 32, 48
    scene = synth(200, W, H, 0.08, sh_deg=3, seed=0)
    module = Rast(Rast.GaussianPointCloudRasterisationConfig())
    loss_fn = LossFunction(LossFunction.LossFunctionConfig(enable_regularization=False))
    q0, t0 = view_pose(1, 3)
    inp = scene_input(scene, q0, t0, DEV, band=3)
    with torch.no_grad():
        target = module(inp)[0].permute(2, 0, 1).contiguous()
    table = pose_table.PoseTable(3, DEV, pose_table.PoseRefinementConfig(reg=0.5))
    table.delta[1] = torch.tensor([0.01, -0.02, 0.005, 0.03, -0.01, 0.02], device=DEV)
    table.grad.fill_(float("nan"))
    row = table.row(1)
    assert row.is_leaf and row.requires_grad and row.data_ptr() == table.delta[1].data_ptr()
    q_base, t_base = inp.q_pointcloud_camera, inp.t_pointcloud_camera
    q, t = pose_table.compose(q_base, t_base, row)
    assert q.shape == (1, 4) and t.shape == (1, 3) and q.requires_grad and t.requires_grad
    features = inp.point_cloud_features.detach().clone()

    def render(q, t):
        """the loss of the scene under a pose; every render starts from the same bits of the scene"""
        step = dataclasses.replace(inp, point_cloud_features=features.clone(), q_pointcloud_camera=q, t_pointcloud_camera=t)
        return loss_fn(module(step)[0].permute(2, 0, 1), target, clamp_predicted=True)[0]
    L = render(q, t)
    L.backward()
    # the direct calls: the rasteriser's pose gradients, then gs_pose_compose_backward
    ql, tl = pose_table.compose_forward(q_base[None], t_base[None], table.delta[1:2])
    ql, tl = ql[0].requires_grad_(True), tl[0].requires_grad_(True)
    assert torch.equal(ql, q) and torch.equal(tl, t)
    L2 = render(ql, tl)
    L2.backward()
    assert L2.item() == L.item() and L.item() > 0
    want = pose_table.compose_backward(q_base[None], table.delta[1:2], ql.grad[None].contiguous(), tl.grad[None].contiguous(), 0.5)[0]
    assert row.grad is not None and torch.equal(row.grad, want) and bool(want.any())
    assert row.grad.data_ptr() == table.grad[1].data_ptr() and torch.equal(table.grad[1], want)     # it landed in the table
    assert bool(torch.isnan(table.grad[0]).all()) and bool(torch.isnan(table.grad[2]).all())        # and nowhere else
    # an ordinary (6,) leaf gets its gradient the ordinary way, accumulated, with the reg it is given (none)
    plain = pose_table.compose_backward(q_base[None], table.delta[1:2], ql.grad[None].contiguous(), tl.grad[None].contiguous(), 0.0)[0]
    free = table.delta[1].clone().requires_grad_(True)
    # (against the same upstream gradients twice: a forward of the rasteriser normalises the scene's quaternions in place, so a
    # later render is not the bits of an earlier one)
    for _ in range(2):
        qf, tf = pose_table.compose(q_base, t_base, free)
        torch.autograd.backward([qf, tf], [ql.grad, tl.grad])
    assert torch.equal(free.grad, plain + plain)
    qf, tf = pose_table.compose(q_base, t_base, free)
    render(qf, tf).backward()
    assert torch.allclose(free.grad, 3 * plain, rtol=1e-3, atol=1e-5)
    # the gradient points downhill: a small step against it lowers the loss
    with torch.no_grad():
        stepped = (table.delta[1] - 1e-3 * plain / plain.norm()).contiguous()
        qs, ts = pose_table.compose_forward(q_base[None], t_base[None], stepped[None])
        L3 = render(qs[0], ts[0])
    assert L3.item() < L.item()
