"""GPU (-m gpu): gs_mixture_log_density and gs_mixture_fourier (include/gs_mixture.h) against the float64 restatement in
tests/mixture_ref.py, at every size around a workgroup of queries (PB) and a chunk of components (CH).

Scenes are seeded: means N(0,1), quaternions NOT normalised (norms in (0.5, 2)), log s uniform in (-3,-1), opacity logits
uniform in (-1,1).  Queries: a 16^3 grid over the box [-BOX, BOX]^3 (sample points for the density, the DFT frequencies of that
box for the transform) plus the component means; the mean of the row of SMALLEST weight comes first, so that every prefix of
the list holds the query that row moves most.  Sizes are prefixes of that list.

Bars (nothing here is fitted to the kernel):
  density    max |out - ref64| <= 4 x max |f32 torch closed form - ref64| over the same queries
  transform  |out - ref64| <= 4 Phi 2^-23 per element, Phi = the case's largest |k.(mu - c)| in float64
  drop-one   asserted on the CPU for every case: leaving the row of smallest weight out of the float64 reference moves some
             output by more than 10 x the bar -- a passing case cannot hide a dropped row.
k = 0 is the second query of the transform list, so it is in every case with P >= 2.  At P = 1 the query is the first mean:
with k = 0 alone Phi is 0 and the bar would be 0, which no f32 sum of N rounded weights meets; that one query has a test of
its own with the bound the weights' roundings give, (N + 2) 2^-24."""
import functools
import math

import pytest
import torch

import mixture_ref as R
import parity_util as P
from taichi_3d_gaussian_splatting_amd import _native, mixture
from taichi_3d_gaussian_splatting_amd.synthetic import synth, view_pose

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PB, CH = mixture.POINTS_PER_WORKGROUP, mixture.COMPONENTS_PER_CHUNK
G = 16
BOX = 5.0
FULL = "grid+means"
P_SIZES = [1, 63, 64, 65, PB + 1, FULL]
N_SIZES = [1, 2, CH - 1, CH, CH + 1, 3 * CH + 7]
BBOX = torch.tensor([[-BOX] * 3, [BOX] * 3])
CENTRE = (BBOX[0] + BBOX[1]) / 2.0


@functools.lru_cache(maxsize=None)
def scene(n):
    return R.make_scene(n, seed=1000 + n)


def lightest(pc, feat, mask=None):
    """index, among the rows that take part, of the row of smallest weight"""
    return int(torch.argmin(R.parameters(pc, feat, mask)[0]))


def query_list(pc, feat, kind):
    j = lightest(pc, feat)
    others = torch.cat([pc[:j], pc[j + 1:]])
    if kind == "density":
        return torch.cat([pc[j:j + 1], R.sample_grid(BBOX, G).reshape(-1, 3), others]).contiguous()
    return torch.cat([pc[j:j + 1], torch.zeros(1, 3), R.frequency_grid(BBOX, G).reshape(-1, 3), others]).contiguous()


@functools.lru_cache(maxsize=None)
def density_case(n):
    """queries, ref64, f32 torch, ref64 without the lightest row: computed once per scene, prefixes serve every P"""
    pc, feat, mask = scene(n)
    x = query_list(pc, feat, "density")
    return (x, R.log_density(pc, feat, mask, x), R.log_density(pc, feat, mask, x, torch.float32).double(),
            R.log_density(pc, feat, mask, x, drop=lightest(pc, feat)))


@functools.lru_cache(maxsize=None)
def fourier_case(n):
    """queries, ref64, per-query largest |phase|, ref64 without the lightest row"""
    pc, feat, mask = scene(n)
    k = query_list(pc, feat, "fourier")
    return (k, R.fourier(pc, feat, mask, k, CENTRE), R.phases(pc, feat, mask, k, CENTRE).abs().amax(1),
            R.fourier(pc, feat, mask, k, CENTRE, drop=lightest(pc, feat)))


def dev(t):
    return None if t is None else t.to(DEV)


def gpu_log_density(pc, feat, mask, x):
    return mixture.log_density((dev(pc), dev(feat), dev(mask)), dev(x)).cpu()


def gpu_fourier(pc, feat, mask, k, centre=CENTRE):
    return mixture.fourier((dev(pc), dev(feat), dev(mask)), dev(k), dev(centre)).cpu()


def count(p, total):
    return total if p == FULL else p


def density_bar(ref, f32, drop):
    bar = 4.0 * float((f32 - ref).abs().max())
    moved = float((drop - ref).abs().max())
    assert moved > 10.0 * bar, ("the case cannot show a dropped row: its inputs are wrong", moved, bar)
    return bar


def fourier_bar(ref, phase, drop):
    bar = 4.0 * float(phase.max()) * 2.0 ** -23
    moved = float((drop - ref).abs().max())
    assert moved > 10.0 * bar, ("the case cannot show a dropped row: its inputs are wrong", moved, bar)
    return bar


@pytest.mark.parametrize("p", P_SIZES)
@pytest.mark.parametrize("n", N_SIZES)
def test_log_density_against_float64(n, p):
    x, ref, f32, drop = density_case(n)
    p = count(p, len(x))
    assert n * p <= 5e8
    bar = density_bar(ref[:p], f32[:p], drop[:p])
    out = gpu_log_density(*scene(n), x[:p])
    assert out.dtype == torch.float32 and out.shape == (p,)
    err = float((out.double() - ref[:p]).abs().max())
    print(f"log_density N={n} P={p}: error {err:.3e}, bar {bar:.3e}, ratio {err / bar:.3f}")
    assert err <= bar, (n, p, err, bar)


@pytest.mark.parametrize("n", N_SIZES)
def test_density_against_float64_by_the_tensor_maximum(n):
    x, ref, f32, _ = density_case(n)
    top = float(ref.exp().max())
    bar = 4.0 * float((f32.exp() - ref.exp()).abs().max()) / top
    pc, feat, mask = scene(n)
    out = mixture.density((dev(pc), dev(feat), dev(mask)), dev(x)).cpu()
    err = float((out.double() - ref.exp()).abs().max()) / top
    print(f"density N={n} P={len(x)}: error / max {err:.3e}, bar {bar:.3e}, ratio {err / bar:.3f}")
    assert err <= bar, (n, err, bar)


@pytest.mark.parametrize("p", P_SIZES)
@pytest.mark.parametrize("n", N_SIZES)
def test_fourier_against_float64(n, p):
    k, ref, phase, drop = fourier_case(n)
    p = count(p, len(k))
    assert n * p <= 5e8
    bar = fourier_bar(ref[:p], phase[:p], drop[:p])
    out = gpu_fourier(*scene(n), k[:p])
    assert out.dtype == torch.complex64 and out.shape == (p,)
    if p >= 2:
        assert bool((k[1] == 0).all()) and abs(complex(ref[1]) - 1.0) < 1e-12          # k = 0 is among the queries, F = 1 there
    err = float((out.to(torch.complex128) - ref[:p]).abs().max())
    print(f"fourier N={n} P={p}: error {err:.3e}, bar {bar:.3e} (Phi {float(phase[:p].max()):.1f}), ratio {err / bar:.3f}")
    assert err <= bar, (n, p, err, bar)


@pytest.mark.parametrize("n", N_SIZES)
def test_the_zero_frequency_alone_is_the_sum_of_the_weights(n):
    """P = 1 with k = 0: every phase is 0, so the value is the f32 sum of N weights each rounded once: within (N + 2) 2^-24 of 1"""
    out = gpu_fourier(*scene(n), torch.zeros(1, 3))
    assert abs(complex(out[0]) - 1.0) <= (n + 2) * 2.0 ** -24, (n, complex(out[0]))
    assert n > 1 or complex(out[0]) == 1.0


# ---- rows that take no part ---------------------------------------------------------------------------------------------------
SPECIAL = [0, 100, CH, CH + 4]


@functools.lru_cache(maxsize=None)
def special_scene():
    """CH + 5 rows, four of them marked for the row cases; (masked, bad, removed): the four masked; the first masked and the others
    unmasked with a NaN position, an infinite log s, q = 0; the four taken out of the arrays"""
    pc, feat, mask = R.make_scene(CH + 5, seed=77)
    masked = (pc, feat, mask.clone())
    masked[2][SPECIAL] = 1
    bpc, bfeat, bmask = pc.clone(), feat.clone(), mask.clone()
    bmask[SPECIAL[0]] = 1
    bpc[SPECIAL[1], 1] = math.nan
    bfeat[SPECIAL[2], 5] = math.inf
    bfeat[SPECIAL[3], :4] = 0.0
    keep = torch.ones(CH + 5, dtype=torch.bool)
    keep[SPECIAL] = False
    return masked, (bpc, bfeat, bmask), (pc[keep].contiguous(), feat[keep].contiguous(), mask[keep].contiguous())


def special_queries(kind):
    pc, feat, mask = special_scene()[2]
    return query_list(pc, feat, kind)


def test_rows_that_take_no_part_leave_the_same_bits_as_masked_rows():
    masked, bad, _ = special_scene()
    assert int(R.takes_part(*bad).sum()) == int(R.takes_part(*masked).sum()) == CH + 1
    x, k = special_queries("density"), special_queries("fourier")
    P.assert_same_bits(gpu_log_density(*bad, x), gpu_log_density(*masked, x), "log_density")
    P.assert_same_bits(torch.view_as_real(gpu_fourier(*bad, k)), torch.view_as_real(gpu_fourier(*masked, k)), "fourier")
    no_mask = (bad[0][1:].contiguous(), bad[1][1:].contiguous(), None)           # the mask may be absent: the three unmasked bad rows
    with_mask = (no_mask[0], no_mask[1], torch.zeros(CH + 4, dtype=torch.int8))
    P.assert_same_bits(gpu_log_density(*no_mask, x), gpu_log_density(*with_mask, x), "log_density without a mask")


def test_rows_appended_behind_the_last_one_change_no_bit():
    """CH + 1 rows and the same with three rows that take no part behind them: two units of the component loop either way"""
    _, _, (pc, feat, mask) = special_scene()
    extra_pc, extra_feat, _ = R.make_scene(3, seed=5)
    extra_pc[0, 0] = math.inf
    extra_feat[1, 7] = math.nan
    longer = (torch.cat([pc, extra_pc]), torch.cat([feat, extra_feat]), torch.cat([mask, torch.tensor([0, 0, 1], dtype=torch.int8)]))
    x, k = special_queries("density"), special_queries("fourier")
    P.assert_same_bits(gpu_log_density(*longer, x), gpu_log_density(pc, feat, mask, x), "log_density")
    P.assert_same_bits(torch.view_as_real(gpu_fourier(*longer, k)), torch.view_as_real(gpu_fourier(pc, feat, mask, k)), "fourier")


def test_taking_masked_rows_out_of_the_arrays_stays_within_the_bar():
    masked, _, removed = special_scene()
    x, k = special_queries("density"), special_queries("fourier")
    j = lightest(*removed)
    ref = R.log_density(*removed, x)
    bar = density_bar(ref, R.log_density(*removed, x, torch.float32).double(), R.log_density(*removed, x, drop=j))
    for s in (masked, removed):
        assert float((gpu_log_density(*s, x).double() - ref).abs().max()) <= bar
    ref = R.fourier(*removed, k, CENTRE)
    bar = fourier_bar(ref, R.phases(*removed, k, CENTRE).abs().amax(1), R.fourier(*removed, k, CENTRE, drop=j))
    for s in (masked, removed):
        assert float((gpu_fourier(*s, k).to(torch.complex128) - ref).abs().max()) <= bar


@pytest.mark.parametrize("n", [1, CH + 1])
def test_a_scene_with_every_row_masked(n):
    pc, feat, _ = scene(n)
    mask = torch.ones(n, dtype=torch.int8)
    x = query_list(pc, feat, "density")[:PB + 1]
    assert bool((gpu_log_density(pc, feat, mask, x) == -math.inf).all())
    out = torch.view_as_real(gpu_fourier(pc, feat, mask, query_list(pc, feat, "fourier")[:PB + 1]))
    assert bool((out == 0).all())
    empty = (torch.zeros(0, 3), torch.zeros(0, 56), None)
    assert bool((gpu_log_density(*empty, x) == -math.inf).all()) and bool((gpu_fourier(*empty, x) == 0).all())
    assert gpu_log_density(pc, feat, mask, x[:0]).shape == (0,) and gpu_fourier(pc, feat, mask, x[:0]).shape == (0,)


def test_far_and_non_finite_queries():
    pc, feat, mask = scene(CH + 1)
    x = query_list(pc, feat, "density")[:PB + 1].clone()
    clean = gpu_log_density(pc, feat, mask, x)
    extent = float(pc.abs().max())
    x[3] = 1e6 * extent
    x[64] = torch.tensor([1e6 * extent, 0.0, -1e6 * extent])
    x[5, 1] = math.nan
    x[PB, 2] = math.inf
    out = gpu_log_density(pc, feat, mask, x)
    assert not math.isnan(float(out[3])) and float(out[3]) < 0 and not math.isnan(float(out[64])) and float(out[64]) < 0
    assert math.isnan(float(out[5])) and math.isnan(float(out[PB]))
    rest = torch.ones(PB + 1, dtype=torch.bool)
    rest[[3, 5, 64, PB]] = False
    P.assert_same_bits(out[rest], clean[rest], "the other queries")
    k = query_list(pc, feat, "fourier")[:PB + 1].clone()
    clean = torch.view_as_real(gpu_fourier(pc, feat, mask, k))
    k[5, 0] = math.nan
    k[PB, 1] = -math.inf
    k[7] = 1e30                                                  # finite: a value, whatever it is, and no NaN elsewhere
    out = torch.view_as_real(gpu_fourier(pc, feat, mask, k))
    assert bool(torch.isnan(out[5]).all()) and bool(torch.isnan(out[PB]).all()) and not bool(torch.isnan(out[7]).any())
    rest[[3, 64]] = True
    rest[7] = False
    P.assert_same_bits(out[rest], clean[rest], "the other frequencies")


# ---- determinism, memory, the frame path -------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_the_work_memory_stops_growing():
    pc, feat, mask = scene(3 * CH + 7)
    x, k = density_case(3 * CH + 7)[0], fourier_case(3 * CH + 7)[0]
    first = gpu_log_density(pc, feat, mask, x), torch.view_as_real(gpu_fourier(pc, feat, mask, k))
    ctx = _native.shared_ctx(torch.device(DEV))
    before = _native.lib().gs_ctx_device_bytes(ctx)
    assert before >= 64 * (3 * CH + 7) + 8 * len(x)              # the work memory is the context's and is counted
    again = gpu_log_density(pc, feat, mask, x), torch.view_as_real(gpu_fourier(pc, feat, mask, k))
    P.assert_same_bits(again[0], first[0], "log_density")
    P.assert_same_bits(again[1], first[1], "fourier")
    assert _native.lib().gs_ctx_device_bytes(ctx) == before
    small = gpu_log_density(pc, feat, mask, x[:65])             # a smaller call, then the first again: same bits, nothing grows
    P.assert_same_bits(small, gpu_log_density(pc, feat, mask, x[:65]))
    P.assert_same_bits(gpu_log_density(pc, feat, mask, x), first[0])
    assert _native.lib().gs_ctx_device_bytes(ctx) == before


def test_a_call_between_forward_and_backward_leaves_the_gradients_alone():
    s = synth(2000, 128, 96, 0.08, sh_deg=3, seed=0)
    q, t = view_pose(1, 3)
    pc, feat, mask = (dev(a) for a in scene(CH + 1))
    x = dev(density_case(CH + 1)[0])
    mixture._bind()
    grads = []
    for with_call in (False, True):
        module = P.module()
        inp = P.make_input(s, q, t)
        image = module(inp, keep_frame=True)[0]
        g = 2.0 * (image.detach() - 0.5)
        if with_call:                                            # on the operator's own context, whose frame is pending
            ctx = module._ctx_for(torch.device(DEV))
            out = torch.empty(len(x), dtype=torch.float32, device=DEV)
            _native.call("gs_mixture_log_density", torch.device(DEV), ctx, pc.data_ptr(), feat.data_ptr(), mask.data_ptr(), len(pc),
                         x.data_ptr(), len(x), out.data_ptr())
            re_im = torch.empty((len(x), 2), dtype=torch.float32, device=DEV)
            _native.call("gs_mixture_fourier", torch.device(DEV), ctx, pc.data_ptr(), feat.data_ptr(), mask.data_ptr(), len(pc),
                         x.data_ptr(), len(x), dev(CENTRE).data_ptr(), re_im.data_ptr())
        image.backward(g)
        grads.append((inp.point_cloud.grad.clone(), inp.point_cloud_features.grad.clone()))
        if with_call:
            P.assert_same_bits(out.cpu(), gpu_log_density(*scene(CH + 1), x.cpu()), "the call itself")
    assert grads[0][1].abs().max() > 0
    P.assert_same_bits(grads[0][0], grads[1][0], "grad_pointcloud")
    P.assert_same_bits(grads[0][1], grads[1][1], "grad_pointcloud_features")


# ---- end to end: both kernels through one FFT -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def consistency_scene():
    pc, feat, mask = R.make_scene(300, seed=3, log_scale=(-1.0, -0.3))
    return pc, feat, mask, R.bounding_box(pc, feat, mask, n_std=4.0)


def test_compare_volume_to_transform_with_the_consistent_convention():
    pc, feat, mask, bbox = consistency_scene()
    report = mixture.compare_volume_to_transform((dev(pc), dev(feat), dev(mask)), G, dev(bbox), consistent=True)
    assert isinstance(report, mixture.MixtureReport) and report.mean_abs_difference.device.type == "cuda"
    diff, cosine = report.as_floats()
    print(f"consistent convention: mean |DFT - analytic| {diff:.3e}, cosine {cosine:.6f}")
    assert cosine >= 0.9999


def test_compare_volume_to_transform_with_the_reference_convention():
    """The two numbers of the float64 restatement, within what the bars above allow them to move.
    Analytic side b: each element within 4 Phi 2^-23.  DFT side a: the density is within e = 4 x the f32 torch error (by the
    tensor maximum) of v, so the normalised volume moves by at most 2 G^3 e / sum(v) in the 1-norm, and every DFT element by
    that much, plus the f32 FFT's own rounding, taken as 3 log2(G^3) 2^-24 |a|_2.  The mean difference is 1-Lipschitz in both
    sides; the cosine of two vectors moves by at most 2 (|da| / |a| + |db| / |b|) in the 2-norm."""
    pc, feat, mask, bbox = consistency_scene()
    a, b, v = R.volume_and_transform(pc, feat, mask, G, bbox, consistent=False)
    want_diff, want_cos = R.compare(a, b)
    x = R.sample_grid(bbox, G).reshape(-1, 3)
    e = 4.0 * float((R.log_density(pc, feat, mask, x, torch.float32).double().exp() - v.reshape(-1)).abs().max())
    norm_a, norm_b = float(a.abs().square().sum().sqrt()), float(b.abs().square().sum().sqrt())
    da = 2.0 * G ** 3 * e / float(v.sum()) + 3.0 * math.log2(G ** 3) * 2.0 ** -24 * norm_a
    k = R.frequency_grid(bbox, G).reshape(-1, 3)
    db = 4.0 * float(R.phases(pc, feat, mask, k, (bbox[0] + bbox[1]) / 2.0).abs().max()) * 2.0 ** -23
    tol_diff, tol_cos = da + db, 2.0 * G ** 1.5 * (da / norm_a + db / norm_b)
    for fn in (mixture.compare_volume_to_transform, mixture.ft_grab_scene):
        diff, cosine = fn((dev(pc), dev(feat), dev(mask)), G, dev(bbox)).as_floats()
        print(f"reference convention: mean difference {diff:.6e} (float64 {want_diff:.6e}, tolerance {tol_diff:.2e}), "
              f"cosine {cosine:.6f} (float64 {want_cos:.6f}, tolerance {tol_cos:.2e})")
        assert abs(diff - want_diff) <= tol_diff
        assert abs(cosine - want_cos) <= tol_cos
    assert mixture.ft_grab_scene is mixture.compare_volume_to_transform


def test_bounding_box_and_volumes_on_the_device():
    pc, feat, mask, _ = consistency_scene()
    s = (dev(pc), dev(feat), dev(mask))
    box = mixture.bounding_box(s)
    assert box.device.type == "cuda" and torch.equal(box.cpu(), R.bounding_box(pc, feat, mask))
    vol, ft = mixture.density_volume(s, 8), mixture.fourier_volume(s, 8)
    assert vol.shape == (8, 8, 8) and vol.dtype == torch.float32 and ft.shape == (8, 8, 8) and ft.dtype == torch.complex64
    want = R.log_density(pc, feat, mask, R.sample_grid(box.cpu(), 8).reshape(-1, 3)).exp().reshape(8, 8, 8)
    assert float((vol.cpu().double() - want).abs().max()) <= 1e-4 * float(want.max())
