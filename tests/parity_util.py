"""Shared helpers of the parity and gradient tests: the scenes, the operator and its input, the CPU oracle on the same
inputs, the bars and the comparisons of every product.  Nothing here touches the GPU at import."""
import os

import numpy as np
import torch

import torch_ref
from oracle import oracle
from taichi_3d_gaussian_splatting_amd import CameraInfo, GaussianPointCloudRasterisation
from taichi_3d_gaussian_splatting_amd.synthetic import scene_input, synth, view_pose

Rast = GaussianPointCloudRasterisation
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INT_EXPORTS = ["point_id_in_camera_list", "num_overlap_tiles", "accumulated_num_overlap_tiles", "sort_key",
               "point_offset_with_sort_key", "tile_points_start", "tile_points_end", "point_in_camera_mask"]
FLOAT_EXPORTS = ["point_uv", "point_in_camera", "point_uv_conic_and_rescale", "point_alpha_after_activation",
                 "point_color", "point_radii"]


UNIT_FACTORS = dict(grad_color_factor=1.0, grad_high_order_color_factor=1.0, grad_s_factor=1.0, grad_q_factor=1.0,
                    grad_alpha_factor=1.0)


def module(partial=False, strict=False, depth=False, hook=None, ctrl=None, **factors):
    """The operator with allow_partial_tiles, backward_reference_order, differentiable_depth and any grad factors set"""
    cfg = Rast.GaussianPointCloudRasterisationConfig()
    cfg.allow_partial_tiles = bool(partial)
    cfg.backward_reference_order = bool(strict)
    cfg.differentiable_depth = bool(depth)
    for k, v in factors.items():
        setattr(cfg, k, v)
    return Rast(cfg, backward_valid_point_hook=hook, controller_accumulators=ctrl)


def make_input(scene, q, t, band=3, requires_grad=True, pose=False):
    """requires_grad: of the points and their features; pose: of q_pointcloud_camera and t_pointcloud_camera"""
    return scene_input(scene, q, t, DEV, band, requires_grad, pose)


def run_oracle(scene, q, t, cfg=None):
    return oracle.forward(scene.point_cloud, scene.point_cloud_features, scene.point_invalid_mask,
                          scene.point_object_id, q, t, scene.camera_intrinsics, scene.height, scene.width, cfg)


def oracle_frame(scene, q, t, partial):
    """-> (Forward, features_after) of the oracle with its default config, for a frame that blends something"""
    f, feat_after = run_oracle(scene, q, t, oracle.default_config(allow_partial_tiles=int(partial)))
    assert f.K > 0
    return f, feat_after


def bits(x):
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return a.view(np.uint8) if a.dtype != np.bool_ else a


def assert_same_bits(a, b, what=None):
    assert np.array_equal(bits(a), bits(b)), what


IMAGE_TOL = 2e-6      # max |a - ref| / max |ref| of the blended images (fused multiply-adds, shared weight alpha*T)


def assert_forward_parity(module, inp, outs, f, feat_after, rgb_only=False):
    """Bit-exact on every integer array and on every per-point f32 array of the forward (uv, conic, colour, radii ...,
    which decide every index); the blended images (sums of up to thousands of terms) within IMAGE_TOL, fifty times
    tighter than the 1e-4 bar; accumulated alpha (1 - T) bit-exact again because T follows the reference sequence."""
    image, depth, count = outs
    fr = module.last_frame
    assert fr.n_points_in_camera == f.M, (fr.n_points_in_camera, f.M)
    assert fr.n_keys == f.K, (fr.n_keys, f.K)
    for name in INT_EXPORTS:
        got = fr.export(name).cpu().numpy()
        assert np.array_equal(got, getattr(f, name)), f"{name} differs"
    for name in FLOAT_EXPORTS:
        got = fr.export(name).cpu().numpy()
        ref = getattr(f, name)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), \
            f"{name}: not bit-exact, max abs diff {np.abs(got - ref).max() if ref.size else 0}"
    # in-place quaternion normalisation, RAST:264-266
    assert np.array_equal(inp.point_cloud_features.detach().cpu().numpy().view(np.uint32), feat_after.view(np.uint32))
    e = rel_err(image.detach().cpu().numpy(), f.rasterized_image)
    assert e < IMAGE_TOL, ("image", e)
    acc = module.last_forward_outputs["pixel_accumulated_alpha"].cpu().numpy() if not rgb_only else None
    if acc is not None:
        assert np.array_equal(acc.view(np.uint32), f.pixel_accumulated_alpha.view(np.uint32)), "pixel_accumulated_alpha"
        assert np.array_equal(module.last_forward_outputs["pixel_offset_of_last_effective_point"].cpu().numpy(),
                              f.pixel_offset_of_last_effective_point), "pixel_offset_of_last_effective_point"
    if not rgb_only:
        assert np.array_equal(count.cpu().numpy(), f.pixel_valid_point_count), "pixel_valid_point_count"
        e = rel_err(depth.detach().cpu().numpy(), f.rasterized_depth)
        assert e < IMAGE_TOL, ("depth", e)


def rel_err(a, ref):
    """max |a-ref| / max|ref|  (the 1e-4 'relative fp32' bar of BASELINE.md section 4)."""
    scale = float(np.abs(ref).max())
    if scale == 0.0:
        return float(np.abs(a).max())
    return float(np.abs(a - ref).max()) / scale


GRAD_TOL = 1e-4          # tensor-level: max |a - ref| / max |ref| per column group
# Per-element bar: |a - ref| <= ELEM_RTOL * |ref| + ELEM_FLOOR * S.  S is the oracle's "summed" magnitude of the
# element (gso_backward_ex): the reference's own expressions for the element with every product replaced by its
# absolute value all the way down -- sum over the loop-1 contributions (RAST:674-696) of the un-cancelled size of each
# contribution (colour*T against w/(1-alpha) in d alpha, a*dx against b*dy in Sigma^-1 d, the terms of Sigma^-1 d d^T Sigma^-1),
# through |loop-2 Jacobian| and the grad factor.  That is the quantity a float evaluation can be accurate relative to
# (the componentwise forward-error bound): an element is a sum of up to ~1e4 signed terms, each itself a difference,
# and the reference adds them with unordered f32 atomics.  The floor covers, per product: hardware-exp alpha (2e-6
# relative), the T recurrence drifting by an ulp per step over a pixel's list (~6e-7 rms over 100 steps), and f32
# summation of n <= 1e4 terms (sqrt(n) * 2^-24 ~ 6e-6 worst case, measured 1.7e-6): 5e-6 in all.  Measured at
# BASELINE configs 2 and 3 (profiles/r02_parity_margins.json): no element uses more than a third of this bar.
ELEM_RTOL = 2e-5         # five times tighter than the 1e-4 of BASELINE.md
ELEM_FLOOR = 5e-6
GROUPS = [(0, 4, "q"), (4, 7, "s"), (7, 8, "opacity"), (8, 56, "sh")]


def elem_margins(a, ref, summed):
    """Per-element statistics of one column group: the worst and 99.9th-percentile use of the per-element bar
    (1.0 = at the bar), the same for the error relative to |ref| over well-conditioned elements (S <= 10 |ref|), and for
    the error relative to S over all elements."""
    a, ref, summed = a.astype(np.float64).ravel(), ref.astype(np.float64).ravel(), summed.astype(np.float64).ravel()
    err = np.abs(a - ref)
    live = summed > 0
    if not live.any():
        return dict(elements=0, bar_use_max=float(err.max()) if err.size else 0.0, bar_use_p999=0.0, rel_max=0.0, rel_p999=0.0,
                    of_summed_max=0.0, of_summed_p999=0.0, outside_live_max_abs=float(err.max()) if err.size else 0.0)
    use = err[live] / (ELEM_RTOL * np.abs(ref[live]) + ELEM_FLOOR * summed[live])
    well = live & (summed <= 10.0 * np.abs(ref))
    rel = err[well] / np.abs(ref[well]) if well.any() else np.zeros(1)
    ofs = err[live] / summed[live]
    q = lambda x: float(np.quantile(x, 0.999))
    return dict(elements=int(live.sum()), bar_use_max=float(use.max()), bar_use_p999=q(use),
                well_conditioned_elements=int(well.sum()), rel_max=float(rel.max()), rel_p999=q(rel),
                of_summed_max=float(ofs.max()), of_summed_p999=q(ofs),
                outside_live_max_abs=float(err[~live].max()) if (~live).any() else 0.0)


def backward_margins(gp, gf, b):
    """{group: elem_margins} for the two returned gradients against an oracle.backward(..., want_summed=True) result."""
    out = {"xyz": elem_margins(gp, b["grad_pointcloud"], b["summed_pointcloud"])}
    for lo, hi, name in GROUPS:
        out[name] = elem_margins(gf[:, lo:hi], b["grad_pointcloud_features"][:, lo:hi], b["summed_pointcloud_features"][:, lo:hi])
    return out


def assert_backward_parity(module, inp, g_image, f, band, extras=None, cfg=None, tensor_tol=GRAD_TOL):
    b = oracle.backward(f, g_image, band, cfg, want_summed=True)
    gp = inp.point_cloud.grad.cpu().numpy()
    gf = inp.point_cloud_features.grad.cpu().numpy()
    assert rel_err(gp, b["grad_pointcloud"]) < tensor_tol, ("xyz", rel_err(gp, b["grad_pointcloud"]))
    for lo, hi, name in GROUPS:
        e = rel_err(gf[:, lo:hi], b["grad_pointcloud_features"][:, lo:hi])
        assert e < tensor_tol, (name, e)
    # every element on its own: within ELEM_RTOL of its value plus ELEM_FLOOR of the magnitude summed to produce it;
    # where nothing was summed (rows outside the frustum, masked SH bands, pixels-free splats) exactly zero
    margins = backward_margins(gp, gf, b)
    for name, m in margins.items():
        assert m["bar_use_max"] <= 1.0, (name, m)
        assert m["outside_live_max_abs"] == 0.0, (name, m)
    # rows outside the frustum are exactly zero
    out = np.setdiff1d(np.arange(f.N), f.point_id_in_camera_list)
    assert not gp[out].any() and not gf[out].any()
    if extras is not None:
        assert rel_err(extras["grad_viewspace"].cpu().numpy(), b["grad_viewspace"]) < GRAD_TOL
        assert rel_err(extras["magnitude_grad_viewspace"].cpu().numpy(), b["magnitude_grad_viewspace"]) < GRAD_TOL
        assert rel_err(extras["magnitude_grad_viewspace_on_image"].cpu().numpy(), b["magnitude_grad_viewspace_on_image"]) < GRAD_TOL
        assert np.array_equal(extras["num_affected_pixels"].cpu().numpy(), b["num_affected_pixels"]), "num_affected_pixels"
    b["margins"] = margins
    return b


def assert_pose_gradient_parity(scene, q, t, partial, gq, gt, g_image=None, g_depth=None, g_alpha=None, per_element=True, use=None):
    """grad_q (K,4) and grad_t (K,3) against torch_ref.pose_gradients for the given upstreams: GRAD_TOL of the tensor maximum;
    per element within ELEM_RTOL of its value plus ELEM_FLOOR of the summed per-point magnitudes; rows no visible point depends
    on exactly zero.  -> the reference's (grad_q, grad_t).  use: a dict that receives, before anything is asserted, what q and t
    use of the tensor bar and of the per-element bar (1.0 = at the bar)"""
    f, feat_after = oracle_frame(scene, q, t, partial)
    rq, rt, sq, st = torch_ref.pose_gradients(scene, q, t, f, feat_after, g_image, g_depth, g_alpha)
    if use is not None:
        for name, a, ref, summed in (("q", gq, rq, sq), ("t", gt, rt, st)):
            err = np.abs(a.astype(np.float64) - ref)
            bar = ELEM_RTOL * np.abs(ref) + ELEM_FLOOR * summed
            use[name] = float(err.max() / max(np.abs(ref).max(), 1e-300) / GRAD_TOL)
            use[name + " element"] = float((err / np.maximum(bar, 1e-300))[bar > 0].max()) if (bar > 0).any() else 0.0
    for name, a, ref, summed in (("q", gq, rq, sq), ("t", gt, rt, st)):
        assert a.shape == ref.shape, name
        scale = np.abs(ref).max()
        assert scale > 0, name
        err = np.abs(a.astype(np.float64) - ref)
        assert err.max() / scale < GRAD_TOL, (name, err.max() / scale, a, ref)
        if per_element:
            bar = ELEM_RTOL * np.abs(ref) + ELEM_FLOOR * summed
            assert np.all(err <= bar), (name, (err / np.maximum(bar, 1e-300)).max(), a, ref)
        assert not a[summed == 0].any(), name          # rows no touched point depends on: exact zeros
    return rq, rt


def random_target(scene, seed):
    """A target image of the scene's size, uniform in 0..1 -> (H,W,3) f32"""
    return np.random.default_rng(seed).uniform(0, 1, (scene.height, scene.width, 3)).astype(np.float32)


def assert_oracle_matches_autograd(s, q, t, target, partial):
    """The two references against each other on the CPU: the oracle's image against torch_ref.render's in float64 (atol 2e-5),
    and its analytic backward of the upstream 2 (image - target), all grad factors 1, against float64 autograd (2e-4 of the
    tensor maximum per column group, and of the view-space gradient) -> {what: error} as measured"""
    cfg = oracle.default_config(allow_partial_tiles=int(partial), **UNIT_FACTORS)
    f, feat_after = run_oracle(s, q, t, cfg)
    assert f.K > 0 and f.pixel_valid_point_count.max() >= 3
    pc = torch.tensor(s.point_cloud, dtype=torch.float64, requires_grad=True)
    ft = torch.tensor(feat_after, dtype=torch.float64, requires_grad=True)
    img, _, _, aux = torch_ref.render(pc, ft, q, t, s.camera_intrinsics, s.height, s.width, f)
    # forward agreement first (f32 oracle vs f64 restatement)
    errors = {"image": float(np.abs(img.detach().numpy() - f.rasterized_image).max())}
    assert np.allclose(img.detach().numpy(), f.rasterized_image, atol=2e-5), errors
    g_img = 2.0 * (f.rasterized_image.astype(np.float64) - target)
    img.backward(torch.tensor(g_img))
    b = oracle.backward(f, g_img.astype(np.float32), color_max_sh_band=3, cfg=cfg)

    def close(a, ref, name):
        scale = np.abs(ref).max() + 1e-12
        errors[name] = err = float(np.abs(a - ref).max() / scale)
        assert err < 2e-4, f"{name}: max err / max|ref| = {err:.3e}"

    close(b["grad_pointcloud"], pc.grad.numpy(), "xyz")
    gf = ft.grad.numpy()
    close(b["grad_pointcloud_features"][:, 0:4], gf[:, 0:4], "q")
    close(b["grad_pointcloud_features"][:, 4:7], gf[:, 4:7], "s")
    close(b["grad_pointcloud_features"][:, 7], gf[:, 7], "opacity")
    close(b["grad_pointcloud_features"][:, 8:], gf[:, 8:], "sh")
    ids = f.point_id_in_camera_list
    close(b["grad_viewspace"][ids], aux["uv"].grad.numpy(), "viewspace")
    return errors


# ---- gradients of the depth and accumulated-alpha outputs against float64 (test_gpu_depth_alpha_grad.py, test_gpu_cameras.py) ----
def upstream(shape, seed, positive=False):
    rng = np.random.default_rng(seed)
    g = rng.uniform(0, 1, shape) if positive else rng.normal(0, 1, shape)
    return torch.tensor(g.astype(np.float32), device=DEV)


UPSTREAM_SEEDS = {"image": 0, "depth": 17, "alpha": 34}


def run_outputs(module, inp, which, seed=0, retain=False, positive=False):
    """forward, then backward of sum(g_k * output_k) over the outputs named in `which` ("image", "depth", "alpha"); the
    upstream of each output depends on its name only; -> ({name: upstream (H,W[,3]) f32 numpy}, the outputs)"""
    outs = module(inp, return_accumulated_alpha=True)
    named = {"image": outs[0], "depth": outs[1], "alpha": outs[3]}
    tensors, grads, ups = [], [], {}
    for name in which:
        g = upstream(named[name].shape, seed + UPSTREAM_SEEDS[name], positive)
        tensors.append(named[name])
        grads.append(g)
        ups[name] = g.cpu().numpy()
    torch.autograd.backward(tensors, grads, retain_graph=retain)
    return ups, outs


def check_point_gradients(gp, gf, ref_p, ref_f, ids):
    """Point gradients against a float64 reference: GRAD_TOL of the maximum of each column group (exact zeros where the group's
    reference is all zero), and exact zeros on the rows outside the frustum -> {group: max |a - ref| / max |ref|}"""
    errors = {}
    for name, a, ref in [("xyz", gp, ref_p)] + [(n, gf[:, lo:hi], ref_f[:, lo:hi]) for lo, hi, n in GROUPS]:
        scale = np.abs(ref).max()
        err = np.abs(a.astype(np.float64) - ref)
        if scale == 0:
            assert not a.any(), name
            continue
        errors[name] = float(err.max() / scale)
        assert err.max() / scale < GRAD_TOL, (name, err.max() / scale)
    out = np.setdiff1d(np.arange(gp.shape[0]), ids)                # rows outside the frustum: exact zeros
    assert not gp[out].any() and not gf[out].any()
    return errors


def float64_point_gradients(scene, q, t, partial, ups):
    """-> (grad_pointcloud, grad_features) of the float64 reference for the upstreams `ups`, and the in-camera ids"""
    f, feat_after = oracle_frame(scene, q, t, partial)
    g = [ups.get(k) for k in ("image", "depth", "alpha")]
    g = [None if x is None else x.astype(np.float64) for x in g]
    tp, tf = torch_ref.point_gradients(scene, q, t, f, feat_after, *g)
    return tp, tf, f.point_id_in_camera_list


# ---- scenes ---------------------------------------------------------------------------------------------------------
def tiny_pose():
    """The pose of tiny_case: its quaternion is deliberately not unit -> (q (1,4), t (1,3))"""
    ang = 0.05
    q = np.array([[0.02, np.sin(ang / 2), -0.01, np.cos(ang / 2)]], np.float32)
    t = np.array([[0.03, -0.02, 0.1]], np.float32)
    return q, t


def tiny_case(seed, n, sigma0, width=32, height=None):
    """A scene small enough for torch_ref, under tiny_pose() -> (scene, q, t, partial)"""
    height = width if height is None else height
    s = synth(n, width, height, sigma0, sh_deg=3, seed=seed)
    q, t = tiny_pose()
    return s, q, t, int(width % 16 != 0 or height % 16 != 0)


def multi_object_case(seed, n_objects, n=64, sigma0=0.5, width=32, height=32, ids=None, empty_last=False):
    """tiny_case with n_objects poses, each the tiny_case pose perturbed by N(0, 0.01) -> (scene, q, t, partial).  ids: the
    object of every point (default: drawn uniformly).  empty_last: the last object's points lie behind the camera, so no
    visible point depends on its row"""
    s, q, t, partial = tiny_case(seed, n, sigma0, width, height)
    rng = np.random.default_rng(seed + 7)
    drawn = rng.integers(0, n_objects, n).astype(np.int32)
    s.point_object_id[:] = drawn if ids is None else np.asarray(ids, np.int32)
    q = np.repeat(q, n_objects, 0) + rng.normal(0, 0.01, (n_objects, 4)).astype(np.float32)
    t = np.repeat(t, n_objects, 0) + rng.normal(0, 0.01, (n_objects, 3)).astype(np.float32)
    if empty_last:
        t[-1] = [0.0, 0.0, 50.0]
    return s, q.astype(np.float32), t.astype(np.float32), partial


# Multi-object frames past one wave (64 in-camera points) and one block (256) of k_pose_points, still small enough for the
# pixel-loop reference: 700 points at 48x48 (3 blocks) and 1200 at 64x64 (5 blocks), every point in camera unless empty_last.
# k_pose_points counts touched points only (a point hidden everywhere takes no slot), so the two layouts that must fill a wave's
# 64 and a block's 256 record slots put the rows that cover most pixels under the unperturbed pose first: the same scene in another row order.
# name -> (frame, n_objects, ids(n) or None for random, empty_last, touched rows first)
POSE_FRAMES = {700: (700, 0.15, 48), 1200: (1200, 0.1, 64)}
POSE_LAYOUTS = {
    "random3_empty_last": (700, 3, None, True, False),                        # several waves and blocks per object; a zero row
    "random3": (1200, 3, None, False, False),
    "random300": (700, 300, None, False, False),                              # more than 256 objects: records at stride 256
    "one_point_per_object": (700, 700, lambda n: np.arange(n), False, True),  # block 0 holds 256 distinct ids: every record slot
    "modulo64": (1200, 64, lambda n: np.arange(n) % 64, False, True),         # a wave holds 64 distinct ids: its last slot
    "contiguous100": (1200, 12, lambda n: np.arange(n) // 100, False, False), # an object straddles every block edge
}


def affected_pixels(f):
    """(M) int: num_affected_pixels of the in-camera entries of an oracle Forward (it does not depend on the upstream)"""
    cfg = oracle.default_config(allow_partial_tiles=int(f.W % 16 != 0 or f.H % 16 != 0))
    return oracle.backward(f, np.ones((f.H, f.W, 3), np.float32), 3, cfg)["num_affected_pixels"]


def pose_layout_case(name):
    """An entry of POSE_LAYOUTS -> (scene, q, t, partial)"""
    n, n_objects, ids, empty_last, touched_first = POSE_LAYOUTS[name]
    _, sigma0, width = POSE_FRAMES[n]
    s, q, t, partial = multi_object_case(n, n_objects, n, sigma0, width, width, None if ids is None else ids(n), empty_last)
    if touched_first:       # rows by falling pixel count under the unperturbed pose: the first ones stay touched under any of the poses
        f, _ = oracle_frame(*tiny_case(n, n, sigma0, width))
        pixels = np.zeros(n, np.int64)
        pixels[f.point_id_in_camera_list] = affected_pixels(f)
        order = np.argsort(-pixels, kind="stable")
        s.point_cloud[:], s.point_cloud_features[:] = s.point_cloud[order], s.point_cloud_features[order]
    return s, q, t, partial


def pose_reduction_shape(object_of_entry, touched):
    """How k_pose_points sees a frame: object_of_entry (M) the object id of every in-camera entry, touched (M) bool (its per-splat
    count is not zero) -> blocks, the largest number of distinct touched ids in a wave (64 entries) and in a block (256), the
    number of objects with a touched point, and of objects with touched points in more than one block."""
    o = np.where(touched, object_of_entry, -1)
    distinct = lambda size: [np.unique(c[c >= 0]) for c in (o[i:i + size] for i in range(0, o.size, size))]
    per_block = distinct(256)
    blocks_of = np.bincount(np.concatenate(per_block).astype(np.int64)) if o.size else np.zeros(0, np.int64)
    return dict(blocks=len(per_block), per_wave=max(len(u) for u in distinct(64)), per_block=max(len(u) for u in per_block),
                objects=int((blocks_of > 0).sum()), objects_in_several_blocks=int((blocks_of > 1).sum()))


LARGE_FRAME = (1, 300000, 0.01, 256, 256)    # tiny_case arguments: more than 262 144 points in camera, past the second trip
                                              # of k_pose_reduce's block loop (1024 x 256) and of k_rows_scatter's (256 x 1024)


# the scenes of the float64 gradient comparisons: the four of test_oracle_autograd and three of the soak
SCENES = [("tiny", (0, 48, 0.25, 32, 32)), ("tiny", (1, 64, 0.6, 32, 32)), ("tiny", (2, 24, 1.2, 32, 32)),
          ("tiny", (3, 56, 0.5, 41, 27)), ("soak", 29), ("soak", 54), ("soak", 182)]


def scene_case(kind, arg):
    """An entry of SCENES -> (scene, q, t, partial)"""
    if kind == "tiny":
        return tiny_case(*arg)
    c = soak_case(arg)
    return c["scene"], c["q"], c["t"], c["partial"]


def dense_corner_scene():
    """26000 splats at 208x160 with 6000 translucent ones piled on a corner region: lists of thousands of entries there, a few
    hundred elsewhere"""
    rng = np.random.default_rng(88)
    s = synth(26000, 208, 160, 0.02, sh_deg=3, seed=88)
    s.point_cloud[:6000, 0] = rng.uniform(-0.9, -0.4, 6000).astype(np.float32) * s.point_cloud[:6000, 2] / 1.2
    s.point_cloud[:6000, 1] = rng.uniform(-0.7, -0.3, 6000).astype(np.float32) * s.point_cloud[:6000, 2] / 1.2
    s.point_cloud_features[:6000, 4:7] = np.log(rng.uniform(0.05, 0.15, (6000, 3))).astype(np.float32)
    s.point_cloud_features[:6000, 7] = rng.uniform(-5.0, -2.5, 6000).astype(np.float32)
    return s


def block_edges_scene(width, height, sigma0):
    """3 * 256 + 1 rows for the edges of the binning's block scans and reductions: rows 256..511 lie behind the camera, so a
    block with no in-camera point sits between two populated ones (and the last block holds one row); row 600 is one faint
    splat far larger than the image, whose box is every tile; the image size is no multiple of 16 (partial edge tiles)"""
    n = 3 * 256 + 1
    s = synth(n, width, height, sigma0, sh_deg=3, seed=n)
    s.point_cloud[256:512, 2] *= -1.0
    s.point_cloud[600, :2] *= 0.1                              # near the optical axis
    s.point_cloud_features[600, 4:7] = np.log(3.0)
    s.point_cloud_features[600, 7] = -3.0                      # faint: everything behind it still counts
    return s


def default_heavy_policy():
    """False when the suite runs under one of the library's diagnostic switches, which replace the default policy of heavy
    tiles and segments that some tests assert"""
    return not any(k in os.environ for k in ("GS_BWD_SPLIT_HEAVY", "GS_BWD_SEGMENTS", "GS_BWD_HEAVY_X2"))


# ---- the randomised scenes of tools/parity_soak.py (also the source of the two seeds kept in the suite) ------------
def soak_case(seed):
    """Seeded scene + pose + config of the parity soak: image sizes 16..640 (half of them not multiples of 16),
    30..50 000 Gaussians, two decades of splat scale, a non-unit pose quaternion, optional invalid rows, SH band 0..3."""
    rng = np.random.default_rng(seed)
    partial = bool(rng.integers(0, 2))
    W = int(rng.integers(1, 40)) * 16 + (int(rng.integers(1, 16)) if partial else 0)
    H = int(rng.integers(1, 30)) * 16 + (int(rng.integers(1, 16)) if partial else 0)
    n = int(10 ** rng.uniform(1.5, 4.7))
    sigma0 = float(10 ** rng.uniform(-2.3, -0.2))
    band = int(rng.integers(0, 4))
    s = synth(n, W, H, sigma0, sh_deg=3, seed=seed)
    if rng.random() < 0.3:
        s.point_invalid_mask[rng.random(n) < 0.2] = 1
    ang = rng.normal(0, 0.15, 3)
    q = np.array([[ang[0], ang[1], ang[2], 1.0]], np.float32) * float(rng.uniform(0.5, 2.0))    # deliberately not unit
    t = rng.normal(0, 0.3, (1, 3)).astype(np.float32)
    return dict(scene=s, q=q, t=t, band=band, partial=partial, rng=rng, W=W, H=H, n=n, sigma0=sigma0)


# ---- frames built from projected records, and frames whose predicted sizes did not hold -----------------------------------
# (tests/test_oracle_stages_host.py, test_gpu_records_frames.py, test_gpu_sizing_redo.py)
RECORD_COUNTS = (1, 255, 256, 257, 513)      # one record; a block of k_boxes_from_records / records-mode k_keygen less one, full, plus one; two blocks plus one
SHARD_CUTS = (0, 1, 300, 300, 1500)          # a single-row shard, an empty shard in the middle
RASTER_EXPORTS = ("sort_key", "point_offset_with_sort_key", "tile_points_start", "tile_points_end", "num_overlap_tiles")


def records_scene():
    """1500 points at 96x64, all in camera under view_pose(): the scene of the block-tail and shard cases"""
    return synth(1500, 96, 64, 0.08, seed=7)


def clustered_cut_scene():
    """3000 clustered points at 64x64: the oracle gives 4 lists over 512 entries, the longest 1030 (cut records, heavy tiles)"""
    from taichi_3d_gaussian_splatting_amd.synthetic import synth_clustered
    return synth_clustered(3000, 64, 64, 0.05, sh_deg=3, seed=4)


def giant_scene(n, width, height, giants=4):
    """synth(n, width, height, 0.05, seed=3) whose first `giants` splats are faint and far larger than the image: the box of each
    is every tile"""
    s = synth(n, width, height, 0.05, seed=3)
    s.point_cloud_features[:giants, 4:7] = np.log(3.0)
    s.point_cloud_features[:giants, 7] = -3.0                  # faint: everything behind them still counts
    return s


def shard_of(scene, lo, hi):
    """Rows lo..hi of a scene (views of its arrays)"""
    import copy
    sub = copy.copy(scene)
    sub.point_cloud, sub.point_cloud_features = scene.point_cloud[lo:hi], scene.point_cloud_features[lo:hi]
    sub.point_invalid_mask, sub.point_object_id = scene.point_invalid_mask[lo:hi], scene.point_object_id[lo:hi]
    return sub


def only_points(scene, ids):
    """The scene with every row but `ids` marked invalid (a copy of the mask; the other arrays are shared)"""
    import copy
    sub = copy.copy(scene)
    sub.point_invalid_mask = np.ones_like(scene.point_invalid_mask)
    sub.point_invalid_mask[np.asarray(ids, np.int64)] = 0
    return sub


def oracle_config(partial=False, **kw):
    return oracle.default_config(allow_partial_tiles=int(bool(partial)), **kw)


FORWARD_PRODUCTS = ("rasterized_image", "rasterized_depth", "pixel_accumulated_alpha", "pixel_offset_of_last_effective_point",
                    "pixel_valid_point_count")


class Run(dict):
    """The products of one forward + backward, by name, as attributes"""
    __getattr__ = dict.__getitem__


def run_monolithic(mod, scene, q, t, band, g_fn):
    """Forward and backward of the operator `mod` -> Run: the five forward products, the raster exports, both gradients, the
    frame's sizing; all numpy but `inp`, `outs`, `g` and `frame`"""
    inp = make_input(scene, q, t, band)
    image, depth, count = mod(inp)
    fr = mod.last_frame
    r = Run(inp=inp, frame=fr, sizing=fr.sizing, outs=(image, depth, count), sort_key_bits=fr.sort_key_bits, n_keys=fr.n_keys,
            n_points_in_camera=fr.n_points_in_camera)
    lo = mod.last_forward_outputs
    for name, x in zip(FORWARD_PRODUCTS, (image, depth, lo["pixel_accumulated_alpha"], lo["pixel_offset_of_last_effective_point"], count)):
        r[name] = x.detach().cpu().numpy().copy()
    for name in RASTER_EXPORTS:
        r[name] = fr.export(name).cpu().numpy()
    r["g"] = g_fn(image.detach())
    image.backward(r["g"])
    r["grad_pointcloud"] = inp.point_cloud.grad.cpu().numpy().copy()
    r["grad_pointcloud_features"] = inp.point_cloud_features.grad.cpu().numpy().copy()
    return r


def run_staged(st, scene, cuts, q, t, band, g_fn, records_prefix=None, second_backward=False):
    """project_shard of every shard lo..hi of `cuts` -> forward_projected of the concatenated records -> backward_projected ->
    backward_shard of every shard, on the StagedRasteriser `st` -> Run with run_monolithic's names plus the staged path's own:
    the magnitude image, the (N,2) / (N) / (M) extras put side by side in shard order, the global ids of the records, the (M,12)
    sums as the library scales them and the opacity of every record.
    records_prefix = (whole_scene, m): forward_projected gets the first m records of whole_scene's projection instead, which
    must be the bits of `scene`'s own records (scene = whole_scene with every other point invalid)."""
    shards, ids_all = [], []
    if records_prefix is not None:                                    # (first, and kept: a frame slot of its own to the end)
        rec_whole, _, fr_whole = st.project_shard(make_input(records_prefix[0], q, t, band, requires_grad=False))
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sinp = make_input(shard_of(scene, lo, hi), q, t, band, requires_grad=False)
        rec, ids, frame = st.project_shard(sinp)
        assert rec.shape == (frame.n_points_in_camera, 16) and ids.shape == (frame.n_points_in_camera,)
        assert bool((ids[1:] > ids[:-1]).all())
        shards.append((sinp, rec, frame))
        ids_all.append(ids.cpu().numpy().astype(np.int64) + lo)
    records = torch.cat([sh[1] for sh in shards]).contiguous()        # shard-major = ascending global point id
    if records_prefix is not None:
        m = records_prefix[1]
        assert records.shape[0] == m
        assert_same_bits(rec_whole[:m], records, "the first m records of the whole scene")
        records = rec_whole[:m].contiguous()
    outs, rframe = st.forward_projected(records, shards[0][0].camera_info)
    r = Run(frame=rframe, sizing=rframe.sizing, sort_key_bits=rframe.sort_key_bits, n_keys=rframe.n_keys,
            n_points_in_camera=rframe.n_points_in_camera, ids=np.concatenate(ids_all), records=records.cpu().numpy())
    assert rframe.n_points_in_camera == records.shape[0]
    for name in FORWARD_PRODUCTS:
        r[name] = getattr(outs, name).cpu().numpy().copy()
    for name in RASTER_EXPORTS:
        r[name] = rframe.export(name).cpu().numpy()
    r["point_alpha_after_activation"] = rframe.export("point_alpha_after_activation").cpu().numpy()
    r["g"] = g_fn(outs.rasterized_image)
    sums, mag_img = st.backward_projected(rframe, outs, r["g"], want_magnitude_image=True)
    assert sums.shape == (records.shape[0], 12)
    r["heavy_tiles"] = rframe.heavy_tiles()
    if second_backward:                                               # through the same kept frame: the same bits again
        sums2, mag2 = st.backward_projected(rframe, outs, r["g"], want_magnitude_image=True)
        assert_same_bits(sums2, sums, "sums of a second backward")
        assert_same_bits(mag2, mag_img, "magnitude image of a second backward")
    r["sums"], r["magnitude_grad_viewspace_on_image"] = sums.cpu().numpy(), mag_img.cpu().numpy()
    parts, off = [], 0
    for sinp, rec, frame in shards:
        m = rec.shape[0]
        parts.append(st.backward_shard(frame, sinp, sums[off:off + m].contiguous(), want_extras=True))
        off += m
    assert off == records.shape[0]
    cat = lambda name: torch.cat([getattr(p, name) for p in parts]).cpu().numpy()
    for name in ("grad_pointcloud", "grad_pointcloud_features", "grad_viewspace", "magnitude_grad_viewspace", "num_affected_pixels"):
        r[name] = cat(name)
    r["shard_frames"] = [sh[2] for sh in shards] + ([fr_whole] if records_prefix is not None else [])
    return r


FRAME_PRODUCTS = FORWARD_PRODUCTS + RASTER_EXPORTS + ("grad_pointcloud", "grad_pointcloud_features")


def assert_same_frame(a, b, what=""):
    """Two Runs agree bit for bit in the forward products, the raster exports and both gradients"""
    for name in FRAME_PRODUCTS:
        assert a[name].shape == b[name].shape, (what, name, a[name].shape, b[name].shape)
        assert_same_bits(a[name], b[name], (what, name))


def assert_staged_equals_monolithic(staged, mono, hook, extras):
    """run_staged against run_monolithic on the same points, bit for bit: assert_same_frame, and the staged path's magnitude image
    and extras against what the operator's hook delivered (`hook`: the BackwardValidPointHookInput, per in-camera point) and
    against the operator's last_backward_extras (`extras`: per point of the scene)"""
    assert staged.n_keys == mono.n_keys and staged.n_points_in_camera == mono.n_points_in_camera
    assert_same_frame(staged, mono, "staged against monolithic")
    ids = staged.ids
    assert np.array_equal(ids, hook.point_id_in_camera_list.cpu().numpy())
    assert_same_bits(staged.magnitude_grad_viewspace_on_image, hook.magnitude_grad_viewspace_on_image, "magnitude image")
    assert_same_bits(staged.grad_viewspace[ids], hook.grad_viewspace, "hook grad_viewspace")
    assert_same_bits(staged.magnitude_grad_viewspace[ids], hook.magnitude_grad_viewspace, "hook magnitude_grad_viewspace")
    assert_same_bits(staged.num_affected_pixels, hook.num_affected_pixels, "hook num_affected_pixels")
    assert_same_bits(staged.num_overlap_tiles, hook.num_overlap_tiles, "hook num_overlap_tiles")
    assert_same_bits(staged.grad_viewspace, extras["grad_viewspace"], "grad_viewspace of every point")
    assert_same_bits(staged.magnitude_grad_viewspace, extras["magnitude_grad_viewspace"], "magnitude_grad_viewspace of every point")
    assert_same_bits(staged.num_affected_pixels, extras["num_affected_pixels"], "num_affected_pixels")


def leave_stale_frames(st, scene, q, t, n_frames, band=3):
    """What a StagedRasteriser's frame slots hold after other work: the dense `scene` projected, rendered from its records and
    back-propagated in n_frames kept raster frames, then everything released -- the next n_frames + 1 frames of `st` get buffers
    whose tile arrays, cut records and flags are that scene's, not fresh zeros"""
    sinp = make_input(scene, q, t, band, requires_grad=False)
    rec, ids, pframe = st.project_shard(sinp)
    assert rec.shape[0] > 0
    kept = []
    for _ in range(n_frames):
        outs, rframe = st.forward_projected(rec.contiguous(), sinp.camera_info)
        assert rframe.n_keys > 0
        sums, _ = st.backward_projected(rframe, outs, 2.0 * (outs.rasterized_image - 0.5), want_magnitude_image=True)
        kept.append(rframe)
    st.backward_shard(pframe, sinp, sums)
    torch.cuda.synchronize()
    for fr in kept + [pframe]:
        fr.release()


SUM_GROUPS = [(0, 2, "uv"), (2, 5, "cov"), (5, 8, "colour"), (8, 9, "opacity"), (9, 10, "magnitude")]


def sums_in_reference_scaling(sums, alpha):
    """(M,12) sums of backward_projected -> float64 in the scaling of oracle.backward_sums: loop 1 of the library leaves the
    per-splat factors to the per-point kernel (k_backward.hip: opacity on columns 0, 1 and 9, opacity / 2 on 2..4,
    (1 - opacity) opacity on 8).  Column 10 (the pixel count, integer bits) and 11 (the depth column, not written without a depth
    upstream) are left out: zeros"""
    s = np.asarray(sums).astype(np.float64)
    a = np.asarray(alpha).astype(np.float64)[:, None]
    s[:, [0, 1, 9]] *= a
    s[:, 2:5] *= 0.5 * a
    s[:, 8:9] *= (1.0 - a) * a
    s[:, 10:12] = 0.0
    return s


def assert_sums_parity(sums, alpha, f, g_image):
    """backward_projected's (M,12) sums against oracle.backward_sums of the oracle frame `f` (of the same records): GRAD_TOL on
    rel_err per column group, the pixel counts exactly -> the worst rel_err"""
    ref, _ = oracle.backward_sums(f, g_image)
    assert ref.shape == np.asarray(sums).shape
    got = sums_in_reference_scaling(sums, alpha)
    assert np.array_equal(np.ascontiguousarray(sums[:, 10]).view(np.int32), np.ascontiguousarray(ref[:, 10]).view(np.int32)), "pixel counts"
    worst = 0.0
    for lo, hi, name in SUM_GROUPS:
        e = rel_err(got[:, lo:hi], ref[:, lo:hi].astype(np.float64))
        print(f"sums against oracle.backward_sums, {name}: max |a - ref| / max |ref| = {e:.3g} (bar {GRAD_TOL})")
        assert np.abs(ref[:, lo:hi]).max() > 0, name
        assert e < GRAD_TOL, (name, e)
        worst = max(worst, e)
    return worst
