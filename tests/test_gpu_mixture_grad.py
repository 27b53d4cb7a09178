"""GPU (-m gpu): gs_mixture_log_density_backward and gs_mixture_fourier_backward (include/gs_mixture_grad.h) against float64
autograd of tests/mixture_ref.py, at every size around a workgroup of rows (CB), an f32 run (RUN) and a query chunk (QC).

Scenes and query lists are those of test_gpu_mixture.py (seeded scenes, a 16^3 grid over [-5, 5]^3 plus the component means,
the lightest row's mean first); sizes are prefixes of the list.  Upstream gradients are seeded: magnitudes uniform in
(0.5, 1.5), random signs, one column for the density and two for the transform.

Bars (nothing here is fitted to the kernel), per group mu, q, log s, alpha and, for the density, x:
  max |out - ref64| <= 4 x max( max |f32 torch autograd - ref64|, 2^-23 max |ref64| )
and for alpha the floor is at least 2^-23 sum_p |g_p| as well: every alpha-gradient is a difference of two sums each bounded by
that.  The f32 autograd runs the queries in slices of at most 512 and lets torch accumulate the slices' gradients.
  drop-one   asserted on the CPU for every case: leaving the last query of the prefix out of the float64 reference moves every
             group by more than 10 x its bar (if not, the query among the last 64 with the largest effect is taken) -- a
             passing case cannot hide a dropped query.  At N = 1 alpha is left out: its gradient is identically zero.
             Two things this assertion cannot be held to as the bars stand, both found on the CPU before any kernel ran:
             (a) alpha's bar has the floor 4 x 2^-23 sum_p |g_p|, which grows with P, while one query moves an alpha-gradient
             by at most about pi_i |g|: from a few hundred queries on no single query reaches 10 such bars (transform, N = 775,
             P = 257: the best of the last 64 reaches 5; at the full list, 1.3).  For THIS assertion alone alpha is held
             against its bar without that floor; the parity check keeps the bar as stated.
             (b) density N = 2, P = 1: the one query is the lighter row's own mean and the other row's share there is 1e-97,
             so mu, q and x are zero to that order, for the reason N = 1, P = 1 is left out.  A group whose float64
             reference is below 1e-30 everywhere is left out of this assertion; at least one group always remains.
Density N = 1, P = 1 is left out: the query is the component's own mean and every gradient but log s is exactly zero."""
import functools
import math

import pytest
import torch

import mixture_grad_ref as GR
import mixture_ref as R
import parity_util as P
import test_gpu_mixture as T
from taichi_3d_gaussian_splatting_amd import _native, mixture, mixture_grad
from taichi_3d_gaussian_splatting_amd.synthetic import synth, view_pose

pytestmark = pytest.mark.gpu
DEV = T.DEV
CB, QC, RUN = mixture_grad.COMPONENTS_PER_WORKGROUP, mixture_grad.QUERIES_PER_CHUNK, mixture_grad.RUN_LENGTH
FULL = T.FULL
P_SIZES = [1, 63, 64, 65, RUN + 1, QC + 1, FULL]
N_SIZES = [1, 2, CB - 1, CB, CB + 1, 3 * CB + 7]
CENTRE = T.CENTRE
SLICE = 512
EPS = 2.0 ** -23
STRUCTURAL_ZERO = 1e-30
dev = T.dev


def count(p, total):
    return total if p == FULL else p


def upstream(kind, n, total):
    return GR.upstream(total, 1 if kind == "density" else 2, seed=7000 + n + (0 if kind == "density" else 1))


def autograd(kind, scene, q, g, dtype, rows=SLICE):
    if kind == "density":
        return GR.autograd_density(*scene, q, g, dtype, rows)
    return GR.autograd_fourier(*scene, q, CENTRE, g, dtype, rows)


def closed(kind, scene, q, g):
    return GR.closed_density(*scene, q, g) if kind == "density" else GR.closed_fourier(*scene, q, CENTRE, g)


def add(a, b):
    """the gradients of two disjoint sets of queries -> of their union (the x rows follow each other)"""
    return {k: (torch.cat([a[k], b[k]]) if k == "x" else a[k] + b[k]) for k in a}


@functools.lru_cache(maxsize=None)
def case(kind, n):
    """queries, upstream gradients, and {P: (ref64, f32)} for every size of the sweep: the gradients of the list's segments
    between the sizes, added up in order, so that the whole sweep costs one pass over the list per dtype"""
    scene = T.scene(n)
    q = T.query_list(scene[0], scene[1], kind)
    g = upstream(kind, n, len(q))
    sizes = sorted({count(p, len(q)) for p in P_SIZES})
    out, lo, acc = {}, 0, None
    for hi in sizes:
        seg = tuple(autograd(kind, scene, q[lo:hi], g[lo:hi], dt) for dt in (torch.float64, torch.float32))
        acc = seg if acc is None else tuple(add(a, s) for a, s in zip(acc, seg))
        out[hi], lo = acc, hi
    return q, g, out


def bars(ref, f32, g, alpha_floor=True):
    out = {}
    for name in ref:
        floor = EPS * float(ref[name].abs().max())
        if name == "alpha" and alpha_floor:
            floor = max(floor, EPS * float(g.abs().sum()))
        out[name] = 4.0 * max(float((f32[name].double() - ref[name]).abs().max()), floor)
    return out


def effect_of(kind, scene, q, g, j):
    """what query j alone adds to each group of the float64 reference (its own row of x for the density)"""
    one = closed(kind, scene, q[j:j + 1], g[j:j + 1])
    return {k: float(v.abs().max()) for k, v in one.items()}


def assert_a_dropped_query_would_show(kind, n, scene, q, g, p, bar, ref):
    """bar: bars(..., alpha_floor=False), see the module's docstring"""
    groups = [k for k in bar if not (n == 1 and k == "alpha") and float(ref[k].abs().max()) > STRUCTURAL_ZERO]
    assert len(groups) >= (1 if p == 1 else len(bar) - 1), (kind, n, p, groups)
    tried = {}
    for j in range(p - 1, max(p - 65, -1), -1):
        tried[j] = effect_of(kind, scene, q, g, j)
        if all(tried[j][k] > 10.0 * bar[k] for k in groups):
            return min(tried[j][k] / bar[k] for k in groups)
    best = max(tried, key=lambda j: min(tried[j][k] / bar[k] for k in groups))
    worst = min(tried[best][k] / bar[k] for k in groups)
    assert worst > 10.0, ("the case cannot show a dropped query: its inputs are wrong", kind, n, p, best, tried[best], bar)
    return worst


def gpu_gradients(kind, scene, q, g, want_x=True):
    s = tuple(dev(a) for a in scene)
    if kind == "density":
        log_p = mixture.log_density(s, dev(q))
        gp, gf, gx = mixture_grad.log_density_backward(s, dev(q), log_p, dev(g.reshape(-1)), want_x=want_x)
        return GR.groups_of(gp.cpu(), gf.cpu(), gx.cpu() if want_x else None), gf.cpu()
    gp, gf = mixture_grad.fourier_backward(s, dev(q), dev(CENTRE), dev(g))
    return GR.groups_of(gp.cpu(), gf.cpu()), gf.cpu()


def check_case(kind, n, p, scene, q, g, ref, f32):
    """-> {group: error / bar}"""
    bar = bars(ref, f32, g)
    shown = assert_a_dropped_query_would_show(kind, n, scene, q, g, p, bars(ref, f32, g, alpha_floor=False), ref)
    out, gf = gpu_gradients(kind, scene, q, g)
    assert gf.dtype == torch.float32 and gf.shape == (n, 56) and bool((gf[:, 8:] == 0).all())
    ratios = {}
    for name in ref:
        assert out[name].shape == ref[name].shape, name
        err = float((out[name].double() - ref[name]).abs().max())
        ratios[name] = err / bar[name]
        print(f"{kind} N={n} P={p} {name}: error {err:.3e}, bar {bar[name]:.3e}, ratio {ratios[name]:.3f} (a dropped query: {shown:.0f} bars)")
    for name in ref:
        assert ratios[name] <= 1.0, (kind, n, p, name, ratios[name])
    return ratios


def sweep_case(kind, n, p):
    q, g, snapshots = case(kind, n)
    p = count(p, len(q))
    ref, f32 = snapshots[p]
    return check_case(kind, n, p, T.scene(n), q[:p], g[:p], ref, f32)


@pytest.mark.parametrize("n,p", [(n, p) for n in N_SIZES for p in P_SIZES if (n, p) != (1, 1)])
def test_log_density_backward_against_float64(n, p):
    sweep_case("density", n, p)


@pytest.mark.parametrize("p", P_SIZES)
@pytest.mark.parametrize("n", N_SIZES)
def test_fourier_backward_against_float64(n, p):
    sweep_case("fourier", n, p)


def chunked_size(n):
    """the smallest P whose query loop is split into at least three chunks with a partial last one"""
    p = 1
    while True:
        chunks, per_chunk = mixture_grad.query_chunks(n, p)
        if chunks >= 3 and p % per_chunk != 0:
            return p
        p += 1


@pytest.mark.parametrize("kind", ["density", "fourier"])
def test_three_query_chunks_with_a_partial_last_one(kind):
    """the reference is the closed form (float64), the yardstick the f32 autograd as everywhere"""
    n = CB + 1
    p = chunked_size(n)
    assert p == 2 * QC + 1 and mixture_grad.query_chunks(n, p) == (3, QC)
    scene = T.scene(n)
    q = T.query_list(scene[0], scene[1], kind)[:p]
    g = upstream(kind, n, p)
    check_case(kind, n, p, scene, q, g, closed(kind, scene, q, g), autograd(kind, scene, q, g, torch.float32))


# ---- rows and queries that take no part ------------------------------------------------------------------------------------------
def same_bits(a, b, what):
    for name in a:
        P.assert_same_bits(a[name].contiguous(), b[name].contiguous(), f"{what}: {name}")


@pytest.mark.parametrize("kind", ["density", "fourier"])
def test_rows_that_take_no_part_get_zero_rows_and_move_no_bit_of_the_others(kind):
    masked, bad, _ = T.special_scene()
    q = T.special_queries(kind)
    g = upstream(kind, 77, len(q))
    a, a_feat = gpu_gradients(kind, bad, q, g)
    b, b_feat = gpu_gradients(kind, masked, q, g)
    same_bits(a, b, kind)
    for name in GR.GROUPS:
        assert bool((a[name][T.SPECIAL] == 0).all()), name
        assert float(a[name].abs().max()) > 0 and bool(torch.isfinite(a[name]).all()), name
    assert bool((a_feat[:, 8:] == 0).all()) and bool((b_feat[:, 8:] == 0).all())
    no_mask = (bad[0][1:].contiguous(), bad[1][1:].contiguous(), None)           # the mask may be absent
    with_mask = (no_mask[0], no_mask[1], torch.zeros(T.CH + 4, dtype=torch.int8))
    same_bits(gpu_gradients(kind, no_mask, q, g)[0], gpu_gradients(kind, with_mask, q, g)[0], kind + " without a mask")


def test_queries_that_contribute_nothing_change_no_bit():
    """g = 0 at a NaN position and at a far one, and a value of -inf under g != 0: the gradients are those of the same call with
    an ordinary point and g = 0 in their places, and their rows of grad_x are zero"""
    n = CB + 1
    scene = T.scene(n)
    p = QC + RUN + 1
    x = T.query_list(scene[0], scene[1], "density")[:p].clone()
    g = upstream("density", n, p).reshape(-1)
    special = [5, RUN, QC]
    plain_g = g.clone()
    plain_g[special] = 0.0
    plain, _ = gpu_gradients("density", scene, x, plain_g)
    odd_x, odd_g = x.clone(), plain_g.clone()
    odd_x[5, 1] = math.nan
    odd_x[RUN] = 1e6 * float(scene[0].abs().max())
    odd_x[QC] = 1e30
    odd_g[QC] = g[QC]
    log_p = mixture.log_density(tuple(dev(a) for a in scene), dev(odd_x)).cpu()
    assert math.isnan(float(log_p[5])) and float(log_p[QC]) == -math.inf and float(log_p[RUN]) < 0
    odd, _ = gpu_gradients("density", scene, odd_x, odd_g)
    same_bits(odd, plain, "density")
    assert bool((odd["x"][special] == 0).all()) and float(odd["x"].abs().max()) > 0
    for name in odd:
        assert bool(torch.isfinite(odd[name]).all()), name
    k = T.query_list(scene[0], scene[1], "fourier")[:p].clone()
    gk = upstream("fourier", n, p)
    gk[special] = 0.0
    plain, _ = gpu_gradients("fourier", scene, k, gk)
    k[5, 0] = math.nan
    k[RUN] = 1e30
    k[QC, 2] = -math.inf
    odd, _ = gpu_gradients("fourier", scene, k, gk)
    same_bits(odd, plain, "fourier")
    for name in odd:
        assert bool(torch.isfinite(odd[name]).all()), name


def test_a_scene_with_no_row_or_no_query():
    pc, feat, _ = T.scene(CB + 1)
    x = T.query_list(pc, feat, "density")[:65]
    g = upstream("density", 1, 65)
    for scene in ((pc, feat, torch.ones(CB + 1, dtype=torch.int8)), (torch.zeros(0, 3), torch.zeros(0, 56), None)):
        for kind, gg in (("density", g), ("fourier", upstream("fourier", 1, 65))):
            out, _ = gpu_gradients(kind, scene, x, gg)
            assert all(bool((v == 0).all()) for v in out.values()), kind
    out, _ = gpu_gradients("density", (pc, feat, None), x[:0], g[:0])
    assert out["x"].shape == (0, 3) and bool((out["mu"] == 0).all())


# ---- determinism, memory, the frame path -------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_the_work_memory_stops_growing():
    n = 3 * CB + 7
    scene = T.scene(n)
    (x, gx, _), (k, gk, _) = case("density", n), case("fourier", n)
    first = gpu_gradients("density", scene, x, gx)[0], gpu_gradients("fourier", scene, k, gk)[0]
    ctx = _native.shared_ctx(torch.device(DEV))
    before = _native.lib().gs_ctx_device_bytes(ctx)
    assert before >= (64 + 80) * n + 32 * len(x)                 # the work memory is the context's and is counted
    again = gpu_gradients("density", scene, x, gx)[0], gpu_gradients("fourier", scene, k, gk)[0]
    same_bits(again[0], first[0], "density")
    same_bits(again[1], first[1], "fourier")
    assert _native.lib().gs_ctx_device_bytes(ctx) == before
    small = gpu_gradients("density", scene, x[:65], gx[:65])[0]  # a smaller call, then the first again: same bits, nothing grows
    same_bits(small, gpu_gradients("density", scene, x[:65], gx[:65])[0], "the smaller call")
    same_bits(gpu_gradients("density", scene, x, gx)[0], first[0], "density after it")
    assert _native.lib().gs_ctx_device_bytes(ctx) == before


def test_backward_calls_between_forward_and_backward_leave_the_rasteriser_gradients_alone():
    s = synth(2000, 128, 96, 0.08, sh_deg=3, seed=0)
    q, t = view_pose(1, 3)
    scene = tuple(dev(a) for a in T.scene(CB + 1))
    x = dev(T.density_case(CB + 1)[0][:QC + 1])
    g = dev(upstream("density", CB + 1, QC + 1).reshape(-1))
    g2 = dev(upstream("fourier", CB + 1, QC + 1))
    log_p = mixture.log_density(scene, x)
    want = mixture_grad.log_density_backward(scene, x, log_p, g), mixture_grad.fourier_backward(scene, x, dev(CENTRE), g2)
    grads = []
    for with_call in (False, True):
        module = P.module()
        inp = P.make_input(s, q, t)
        image = module(inp, keep_frame=True)[0]
        g_image = 2.0 * (image.detach() - 0.5)
        if with_call:                                            # on the operator's own context, whose frame is pending
            ctx = module._ctx_for(torch.device(DEV))
            got = (mixture_grad.log_density_backward(scene, x, log_p, g, ctx=ctx),
                   mixture_grad.fourier_backward(scene, x, dev(CENTRE), g2, ctx=ctx))
        image.backward(g_image)
        grads.append((inp.point_cloud.grad.clone(), inp.point_cloud_features.grad.clone()))
    assert grads[0][1].abs().max() > 0
    P.assert_same_bits(grads[0][0], grads[1][0], "grad_pointcloud")
    P.assert_same_bits(grads[0][1], grads[1][1], "grad_pointcloud_features")
    for a, b in zip(got[0] + got[1], want[0] + want[1]):
        P.assert_same_bits(a, b, "the calls themselves")


# ---- the public path ------------------------------------------------------------------------------------------------------------------
def leaves(n, p):
    pc, feat, mask = T.scene(n)
    x = T.query_list(pc, feat, "density")[:p]
    return dev(pc).requires_grad_(True), dev(feat).requires_grad_(True), dev(mask), dev(x).requires_grad_(True)


def test_log_density_fills_the_gradients_of_its_inputs():
    n, p = CB + 1, QC + 1
    pc, feat, mask, x = leaves(n, p)
    g = dev(upstream("density", n, p).reshape(-1))
    plain = mixture.log_density((pc.detach(), feat.detach(), mask), x.detach())
    out = mixture.log_density((pc, feat, mask), x)
    assert out.requires_grad and not plain.requires_grad
    P.assert_same_bits(out, plain, "the forward's bits")
    (out * g).sum().backward(retain_graph=True)
    want = mixture_grad.log_density_backward((pc, feat, mask), x, plain, g)
    for got, ref, name in zip((pc.grad, feat.grad, x.grad), want, ("point_cloud", "point_cloud_features", "x")):
        assert got.shape == ref.shape and got.dtype == torch.float32
        P.assert_same_bits(got, ref, name)
    assert bool((feat.grad[:, 8:] == 0).all()) and float(feat.grad[:, :8].abs().max()) > 0
    (out * g).sum().backward()                                   # a second backward accumulates
    for got, ref in zip((pc.grad, feat.grad, x.grad), want):
        P.assert_same_bits(got, ref + ref, "accumulated")
    with torch.no_grad():
        P.assert_same_bits(mixture.log_density((pc, feat, mask), x), plain, "under no_grad")
        assert not mixture.log_density((pc, feat, mask), x).requires_grad
    only_x = mixture.log_density((pc.detach(), feat.detach(), mask), x)        # x alone asks for a gradient
    x.grad = None
    (only_x * g).sum().backward()
    P.assert_same_bits(x.grad, want[2], "x alone")


def test_density_and_float64_inputs_backpropagate():
    n, p = CB - 1, 65
    pc, feat, mask, x = leaves(n, p)
    pc64 = pc.detach().double().requires_grad_(True)
    dens = mixture.density((pc64, feat, mask), x)
    dens.sum().backward()
    assert pc64.grad.dtype == torch.float64 and pc64.grad.shape == (n, 3)
    log_p = mixture.log_density((pc.detach(), feat.detach(), mask), x.detach())
    want = mixture_grad.log_density_backward((pc, feat, mask), x, log_p, log_p.exp())
    P.assert_same_bits(pc64.grad.float(), want[0], "through exp")
    P.assert_same_bits(feat.grad, want[1], "through exp")


def test_fourier_fills_the_gradients_of_the_scene():
    n, p = CB + 1, QC + 1
    pc, feat, mask, _ = leaves(n, p)
    k = dev(T.query_list(*T.scene(n)[:2], "fourier")[:p])
    g = dev(upstream("fourier", n, p))
    plain = mixture.fourier((pc.detach(), feat.detach(), mask), k, dev(CENTRE))
    out = mixture.fourier((pc, feat, mask), k, dev(CENTRE))
    assert out.dtype == torch.complex64 and out.requires_grad
    P.assert_same_bits(torch.view_as_real(out), torch.view_as_real(plain), "the forward's bits")
    (torch.view_as_real(out) * g).sum().backward()
    want = mixture_grad.fourier_backward((pc, feat, mask), k, dev(CENTRE), g)
    P.assert_same_bits(pc.grad, want[0], "point_cloud")
    P.assert_same_bits(feat.grad, want[1], "point_cloud_features")
    with pytest.raises(ValueError, match="k requires"):
        mixture.fourier((pc, feat, mask), k.clone().requires_grad_(True), dev(CENTRE))
    vol = mixture.fourier_volume((pc, feat, mask), 4)
    assert vol.requires_grad and mixture.density_volume((pc, feat, mask), 4).requires_grad
    assert not mixture.bounding_box((pc, feat, mask)).requires_grad


def test_a_gradient_step_on_the_point_likelihood_raises_it():
    """300 rows, 400 sample points drawn around the means; the step is small enough that the float64 reference's own step raises
    the sum, and the device's step, taken from the device's gradient, must raise the device's sum"""
    pc, feat, mask = R.make_scene(300, seed=3, log_scale=(-1.0, -0.3))
    gen = torch.Generator().manual_seed(11)
    x = pc[torch.randint(0, 300, (400,), generator=gen)] + 0.3 * torch.randn(400, 3, generator=gen)
    ones = torch.ones(400, 1)
    ref = GR.autograd_density(pc, feat, mask, x, ones)
    step = 1e-4
    before64 = float(R.log_density(pc, feat, mask, x).sum())
    feat64 = feat.double()
    feat64[:, :4] += step * ref["q"]
    feat64[:, 4:7] += step * ref["log_s"]
    feat64[:, 7] += step * ref["alpha"]
    after64 = float(R.log_density(pc.double() + step * ref["mu"], feat64, mask, x, torch.float64).sum())
    assert after64 > before64
    pc_d, feat_d, x_d = dev(pc).requires_grad_(True), dev(feat).requires_grad_(True), dev(x)
    total = mixture.log_density((pc_d, feat_d, dev(mask)), x_d).sum()
    total.backward()
    with torch.no_grad():
        stepped = mixture.log_density((pc_d + step * pc_d.grad, feat_d + step * feat_d.grad, dev(mask)), x_d).sum()
    print(f"sum log p: {float(total.detach()):.4f} -> {float(stepped):.4f} (float64: {before64:.4f} -> {after64:.4f})")
    assert float(stepped) > float(total.detach())
