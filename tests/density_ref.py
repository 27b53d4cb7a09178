"""Restatement of the reference's adaptive density control (CTRL = taichi_3d_gaussian_splatting/
GaussianPointAdaptiveController.py, GP3D = taichi_3d_gaussian_splatting/GaussianPoint3D.py) in torch, line by line,
as the oracle of tests/test_gpu_density.py and the baseline of tools/bench_densify.py.

The two Taichi kernels of CTRL:10-42 are restated too; GaussianPoint3D.sample()'s ti.random() is replaced by the
Philox4x32-10 stream libgsrast draws from (counter = (destination row, call index, 0 clone / 1 original, 0), key =
the 64-bit seed), so that sampled positions are comparable.  Runs on any device; the tests run it on the CPU, where
every f32 operation is IEEE-rounded."""
import numpy as np
import torch

PHILOX_M = (0xD2511F53, 0xCD9E8D57)
PHILOX_W = (0x9E3779B9, 0xBB67AE85)
MASK32 = 0xFFFFFFFF


def philox4x32_10_numpy(ctr, key):
    """ctr: (..., 4) uint32, key: (2,) uint32 -> (..., 4) uint32 (Random123 philox4x32, 10 rounds)."""
    c = [np.asarray(ctr, np.uint64)[..., i] for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(PHILOX_W[0])) & np.uint64(MASK32), (k1 + np.uint64(PHILOX_W[1])) & np.uint64(MASK32)
        p0, p1 = np.uint64(PHILOX_M[0]) * c[0], np.uint64(PHILOX_M[1]) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & np.uint64(MASK32), (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & np.uint64(MASK32)]
    return np.stack(c, -1).astype(np.uint32)


def philox4x32_10_torch(ctr, key):
    """The same on int64 tensors holding uint32 values (int64 products wrap modulo 2^64, which keeps both halves)."""
    c = [ctr[..., i] for i in range(4)]
    k0, k1 = int(key[0]), int(key[1])
    for r in range(10):
        if r:
            k0, k1 = (k0 + PHILOX_W[0]) & MASK32, (k1 + PHILOX_W[1]) & MASK32
        p0, p1 = c[0] * PHILOX_M[0], c[2] * PHILOX_M[1]
        c = [((p1 >> 32) & MASK32) ^ c[1] ^ k0, p1 & MASK32, ((p0 >> 32) & MASK32) ^ c[3] ^ k1, p0 & MASK32]
    return torch.stack(c, -1)


def seed_key(seed):
    return (seed & MASK32, (seed >> 32) & MASK32)


def rotation_matrix(q):
    """GP3D:31-49 on (n,4) xyzw, not normalised."""
    x, y, z, w = q.unbind(-1)
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    return torch.stack([torch.stack([1 - 2 * (yy + zz), 2 * (xy - wz), 2 * (xz + wy)], -1),
                        torch.stack([2 * (xy + wz), 1 - 2 * (xx + zz), 2 * (yz - wx)], -1),
                        torch.stack([2 * (xz - wy), 2 * (yz + wx), 1 - 2 * (xx + yy)], -1)], -2)


def sample_from_point(pos, feat, rows, call_index, which, seed):
    """CTRL:27-42 / GP3D:391-406 with the Philox stream: pos (n,3), feat (n,56), rows (n,) destination rows."""
    n = rows.shape[0]
    ctr = torch.stack([rows.to(torch.int64), torch.full((n,), call_index, dtype=torch.int64, device=rows.device),
                       torch.full((n,), which, dtype=torch.int64, device=rows.device), torch.zeros(n, dtype=torch.int64, device=rows.device)], -1)
    u = ((philox4x32_10_torch(ctr, seed_key(seed)) >> 8) + 1).to(torch.float32) * 2.0 ** -24
    u1, u2, u3, u4 = u.unbind(-1)
    two_pi = float(np.float32(2 * 3.141592653589))
    z1 = torch.sqrt(-2 * torch.log(u1)) * torch.cos(two_pi * u2)              # GP3D:91-94
    z2 = torch.sqrt(-2 * torch.log(u1)) * torch.sin(two_pi * u2)
    z3 = torch.sqrt(-2 * torch.log(u3)) * torch.cos(two_pi * u4)
    base = torch.stack([z1, z2, z3], -1)
    RS = rotation_matrix(feat[:, 0:4]) * torch.exp(feat[:, 4:7])[:, None, :]
    return pos + (RS * base[:, None, :]).sum(-1)


def ellipsoid_offset(feat):
    """CTRL:10-25 / GP3D:376-388, the base-axis choice as written."""
    s = feat[:, 4:7]
    base = torch.zeros_like(s)
    axis = torch.zeros(s.shape[0], dtype=torch.int64, device=s.device)
    axis[(s[:, 0] < s[:, 1]) & (s[:, 1] > s[:, 2])] = 1
    axis[~((s[:, 0] < s[:, 1]) & (s[:, 1] > s[:, 2])) & (s[:, 0] < s[:, 2]) & (s[:, 1] < s[:, 2])] = 2
    base[torch.arange(s.shape[0], device=s.device), axis] = 1
    v = (rotation_matrix(feat[:, 0:4]) @ base[:, :, None])[:, :, 0]
    e = torch.exp(s)
    rc, ra = e.max(-1).values, e.min(-1).values
    return torch.sqrt(rc ** 2 - ra ** 2)[:, None] * v


def find_densify_points(pc, feat, mask, acc, ids, npix, depth, mag, remove_floaters, cfg):
    """CTRL:170-265.  acc: dict of the six accumulators by their reference names.  Returns the densify info and the masks."""
    point_id_list = torch.arange(pc.shape[0], device=pc.device)
    ids = ids.long()
    average_num_affect_pixels = acc["accumulated_num_pixels"] / acc["accumulated_num_in_camera"]            # :181
    average_num_affect_pixels[torch.isnan(average_num_affect_pixels)] = 0                                 # :182
    floater_mask = torch.zeros_like(point_id_list, dtype=torch.bool)
    floater_mask_in_camera = torch.zeros_like(ids, dtype=torch.bool)
    floater_point_id = torch.empty(0, dtype=torch.int64, device=pc.device)
    if remove_floaters:                                                                                    # :191
        floater_mask_in_camera = (npix > cfg.floater_near_camrea_num_pixels_threshold) & (depth < cfg.floater_depth_threshold)
        floater_point_id = ids[floater_mask_in_camera]
        floater_mask[floater_point_id] = True
        floater_mask = floater_mask & (mask == 0)                                                          # :199
    point_alpha = feat[:, 7]
    nan_mask = torch.isnan(feat).any(dim=1)                                                                # :203
    transparent_point_mask = ((point_alpha < cfg.transparent_alpha_threshold) | nan_mask) & (mask == 0) & (~floater_mask)
    transparent_point_id = point_id_list[transparent_point_mask]
    will_be_remove_mask = floater_mask | transparent_point_mask
    in_camera_will_be_remove_mask = floater_mask_in_camera | transparent_point_mask[ids]                   # :213
    in_camera_to_densify_mask = mag > cfg.densification_view_space_position_gradients_threshold            # :217
    in_camera_to_densify_mask &= ~in_camera_will_be_remove_mask
    num_to_densify_by_viewspace = int(in_camera_to_densify_mask.sum())
    in_camera_to_densify_mask |= (mag / npix > cfg.densification_view_avg_space_position_gradients_threshold)   # :221
    in_camera_to_densify_mask &= ~in_camera_will_be_remove_mask
    num_to_densify = int(in_camera_to_densify_mask.sum())
    single_frame_densify_point_id = ids[in_camera_to_densify_mask]
    single_frame_densify_point_mask = torch.zeros_like(point_id_list, dtype=torch.bool)
    single_frame_densify_point_mask[single_frame_densify_point_id] = True
    nic = acc["accumulated_num_in_camera"]
    mf = acc["accumulated_view_space_position_gradients"] / nic                                            # :230
    mf[torch.isnan(mf)] = 0
    multi_frame_densify_mask = mf > cfg.densification_multi_frame_view_space_position_gradients_threshold
    mfa = acc["accumulated_view_space_position_gradients_avg"] / nic                                       # :235
    mfa[torch.isnan(mfa)] = 0
    multi_frame_densify_mask |= (mfa / average_num_affect_pixels > cfg.densification_multi_frame_view_pixel_avg_space_position_gradients_threshold)
    mfn = acc["accumulated_position_gradients_norm"] / nic                                                 # :240, no NaN fill
    multi_frame_densify_mask |= (mfn > cfg.densification_multi_frame_position_gradients_threshold)
    to_densify_mask = (single_frame_densify_point_mask | multi_frame_densify_mask) & (~will_be_remove_mask)   # :243
    to_densify_mask &= mask == 0        # libgsrast: valid rows only (a no-op in the reference's wiring, see k_density.hip)
    densify_point_id = point_id_list[to_densify_mask]
    densify_point_position_before_optimization = pc[densify_point_id].clone()                             # :248
    densify_point_grad_position = acc["accumulated_position_gradients"][densify_point_id] / nic[densify_point_id].unsqueeze(-1)
    densify_point_grad_position[torch.isnan(densify_point_grad_position)] = 0                              # :251
    densify_size_reduction_factor = torch.zeros_like(densify_point_id, dtype=torch.float32)
    over_reconstructed_mask = acc["accumulated_num_pixels"][to_densify_mask] > cfg.under_reconstructed_num_pixels_threshold
    densify_size_reduction_factor[over_reconstructed_mask] = float(np.float32(np.log(cfg.gaussian_split_factor_phi)))
    return dict(floater_point_id=floater_point_id, transparent_point_id=transparent_point_id, densify_point_id=densify_point_id,
                densify_point_position_before_optimization=densify_point_position_before_optimization,
                densify_size_reduction_factor=densify_size_reduction_factor.unsqueeze(-1),
                densify_point_grad_position=densify_point_grad_position,
                floater_mask=floater_mask, transparent_mask=transparent_point_mask, densify_mask=to_densify_mask,
                num_to_densify=num_to_densify, num_to_densify_by_viewspace=num_to_densify_by_viewspace)


def add_densify_points(pc, feat, mask, obj, info, cfg, seed, call_index):
    """CTRL:290-353, in place on pc / feat / mask / obj.  Returns the counts and the fill rows."""
    total_valid_points_before_densify = int(mask.shape[0] - mask.sum())
    num_transparent_points = info["transparent_point_id"].shape[0]
    mask[info["transparent_point_id"]] = 1
    num_floaters_points = info["floater_point_id"].shape[0]
    mask[info["floater_point_id"]] = 1
    num_of_densify_points = info["densify_point_id"].shape[0]
    invalid_point_id_to_fill = torch.where(mask == 1)[0][:num_of_densify_points]                          # :299
    num_fillable_densify_points = 0
    num_over_reconstructed = num_under_reconstructed = 0
    if num_of_densify_points > 0:
        nf = num_fillable_densify_points = min(num_of_densify_points, invalid_point_id_to_fill.shape[0])
        factor = info["densify_size_reduction_factor"][:nf]
        pc[invalid_point_id_to_fill] = info["densify_point_position_before_optimization"][:nf]
        feat[invalid_point_id_to_fill] = feat[info["densify_point_id"][:nf]]
        obj[invalid_point_id_to_fill] = obj[info["densify_point_id"][:nf]]
        feat[invalid_point_id_to_fill, 4:7] -= factor
        over_reconstructed_mask = (factor > 1e-6).reshape(-1)
        under_reconstructed_mask = ~over_reconstructed_mask
        num_over_reconstructed = int(over_reconstructed_mask.sum())
        num_under_reconstructed = nf - num_over_reconstructed
        densify_point_id = info["densify_point_id"][:nf]
        feat[densify_point_id, 4:7] -= factor
        if cfg.enable_ellipsoid_offset:                                                                     # :322
            point_offset = ellipsoid_offset(feat[densify_point_id])
            pc[invalid_point_id_to_fill] += point_offset
            pc[densify_point_id] -= point_offset
        if cfg.enable_sample_from_point:                                                                    # :329
            over_id = densify_point_id[over_reconstructed_mask]
            over_fill = invalid_point_id_to_fill[over_reconstructed_mask]
            pc[over_fill] = sample_from_point(pc[over_id], feat[over_id], over_fill, call_index, 0, seed)
            pc[over_id] = sample_from_point(pc[over_id], feat[over_id], over_id, call_index, 1, seed)
            under_fill = invalid_point_id_to_fill[under_reconstructed_mask]
            under_grad = info["densify_point_grad_position"][:nf][under_reconstructed_mask]
            pc[under_fill] += under_grad * cfg.under_reconstructed_move_factor
        mask[invalid_point_id_to_fill] = 0
    total_valid_points_after_densify = int(mask.shape[0] - mask.sum())
    assert total_valid_points_after_densify == (total_valid_points_before_densify - num_transparent_points - num_floaters_points
                                                + num_fillable_densify_points)                               # :346
    return dict(floaters=num_floaters_points, transparent=num_transparent_points, densify=num_of_densify_points,
                fillable=num_fillable_densify_points, over=num_over_reconstructed, under=num_under_reconstructed,
                valid_before=total_valid_points_before_densify, valid_after=total_valid_points_after_densify,
                fill_point_id=invalid_point_id_to_fill[:num_fillable_densify_points])


ACCUMULATORS = (("accumulated_num_in_camera", torch.int32, ()), ("accumulated_num_pixels", torch.int32, ()),
                ("accumulated_view_space_position_gradients", torch.float32, ()),
                ("accumulated_view_space_position_gradients_avg", torch.float32, ()),
                ("accumulated_position_gradients", torch.float32, (3,)), ("accumulated_position_gradients_norm", torch.float32, ()))


class ReferenceController:
    """CTRL:130-168 around find_densify_points / add_densify_points: the counter and the schedule, update()'s six
    accumulations in f32 as the reference does them, refinement() with the apply's call index, the accumulator reset and
    reset_alpha.  The scene and the accumulators are plain attributes (pc, feat, mask, obj; acc), edited in place as the
    reference edits its maintained parameters, so that a caller may also replace them between two steps."""

    def __init__(self, cfg, pc, feat, mask, obj, seed=0):
        self.cfg, self.seed = cfg, seed
        self.pc, self.feat, self.mask, self.obj = pc, feat, mask, obj
        self.iteration_counter = -1                                                                         # CTRL:109
        self.refinement_calls = 0
        self.info = None
        self.reset()

    def reset(self):                                                                                        # CTRL:114-125, 154-165
        n = self.pc.shape[0]
        self.acc = {name: torch.zeros((n,) + shape, dtype=dtype, device=self.pc.device) for name, dtype, shape in ACCUMULATORS}

    def is_densify_iteration(self):                                                                         # CTRL:142-144, 150-152
        return (self.iteration_counter >= self.cfg.num_iterations_warm_up
                and self.iteration_counter % self.cfg.num_iterations_densify == 0)

    def update(self, payload):
        """payload: point_id_in_camera_list, num_affected_pixels, magnitude_grad_viewspace, point_depth and
        grad_point_in_camera of the reference's BackwardValidPointHookInput.  -> the densify info on a densify iteration"""
        self.iteration_counter += 1                                                                         # :131
        ids = payload.point_id_in_camera_list.long()
        a = self.acc
        a["accumulated_num_in_camera"][ids] += 1                                                            # :133
        a["accumulated_num_pixels"][ids] += payload.num_affected_pixels                                     # :134
        grad_viewspace_norm = payload.magnitude_grad_viewspace
        a["accumulated_view_space_position_gradients"][ids] += grad_viewspace_norm                          # :136
        avg_grad_viewspace_norm = grad_viewspace_norm / payload.num_affected_pixels                         # :137
        avg_grad_viewspace_norm[torch.isnan(avg_grad_viewspace_norm)] = 0                                   # :138
        a["accumulated_view_space_position_gradients_avg"][ids] += avg_grad_viewspace_norm                  # :139
        a["accumulated_position_gradients"][ids] += payload.grad_point_in_camera                            # :140
        a["accumulated_position_gradients_norm"][ids] += payload.grad_point_in_camera.norm(dim=1)           # :141
        if not self.is_densify_iteration():
            return None
        remove_floaters = self.iteration_counter > self.cfg.iteration_start_remove_floater                  # :191
        self.info = find_densify_points(self.pc, self.feat, self.mask, a, payload.point_id_in_camera_list,
                                        payload.num_affected_pixels, payload.point_depth, payload.magnitude_grad_viewspace,
                                        remove_floaters, self.cfg)
        return self.info

    def refinement(self):
        """-> None during the warm-up, else dict(counts=the apply's counts or None, info=its densify info or None,
        reset_alpha=whether CTRL:166 fired, rows_lowered=the rows whose alpha it lowered)"""
        if self.iteration_counter < self.cfg.num_iterations_warm_up:                                        # :150
            return None
        counts = info = None
        if self.iteration_counter % self.cfg.num_iterations_densify == 0:                                   # :152
            assert self.info is not None                                                                    # :291
            info, self.info = self.info, None
            counts = add_densify_points(self.pc, self.feat, self.mask, self.obj, info, self.cfg, self.seed, self.refinement_calls)
            self.refinement_calls += 1
            self.reset()
        reset_alpha = self.iteration_counter % self.cfg.num_iterations_reset_alpha == 0                     # :166
        lowered = 0
        if reset_alpha:
            lowered = int((self.feat[:, 7] > self.cfg.reset_alpha_value).sum())
            self.feat[:, 7] = torch.clamp(self.feat[:, 7], max=self.cfg.reset_alpha_value)                  # :355-358
        return dict(counts=counts, info=info, reset_alpha=reset_alpha, rows_lowered=lowered)
