"""GPU (-m gpu): frames built from projected records (gs_forward_projected) where they leave the path of a gs_forward frame.

Such a frame runs k_boxes_from_records (which clears the tile arrays itself, in a grid-stride loop), k_keygen without block offsets
(256 consecutive records per block, the last block a tail) and every backward without k_project's largest-tile-count word, so that
k_sum_rows looks for giant points itself.  Every case here checks two things: the staged chain project_shard -> forward_projected
-> backward_projected -> backward_shard against the monolithic operator on the same points, bit for bit in every product both
have (forward outputs, raster exports, gradients, the magnitude image and the hook's extras); and the monolithic operator against
the CPU oracle at the bars of parity_util.  That the oracle's own staged halves agree with its monolithic ones is
test_oracle_stages_host.py.

Before the frame under test the same StagedRasteriser renders and back-propagates another, denser scene of the same image size in
as many kept frames as the case will use and releases them (parity_util.leave_stale_frames): the buffers of the frame under test
then hold that scene's tile arrays, cut records and flags, not fresh zeros."""
import numpy as np
import pytest
import torch

from taichi_3d_gaussian_splatting_amd.stages import StagedRasteriser
from taichi_3d_gaussian_splatting_amd.synthetic import synth, synth_clustered, view_pose

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import parity_util
    return parity_util


def _case(P, scene, cuts, q, t, dense, partial=False, band=3, records_prefix=None, second_backward=False, seed=0):
    """The two checks of this file on `scene` cut into shards at `cuts` -> (operator, its Run, the staged Run, oracle Forward)"""
    H, W = scene.height, scene.width
    assert (dense.height, dense.width) == (H, W)
    target = torch.tensor(np.random.default_rng(seed).uniform(0, 1, (H, W, 3)).astype(np.float32), device=P.DEV)
    g_fn = lambda image: 2.0 * (image - target)
    hooked = []
    mod = P.module(partial, hook=hooked.append)
    mono = P.run_monolithic(mod, scene, q, t, band, g_fn)
    ocfg = P.oracle_config(partial)
    f, feat_after = P.run_oracle(scene, q, t, ocfg)
    assert f.K > 0
    P.assert_forward_parity(mod, mono.inp, mono.outs, f, feat_after)
    P.assert_backward_parity(mod, mono.inp, mono.g.cpu().numpy(), f, band, mod.last_backward_extras, ocfg)
    st = StagedRasteriser(mod.config)
    P.leave_stale_frames(st, dense, q, t, n_frames=len(cuts) + 1)
    staged = P.run_staged(st, scene, cuts, q, t, band, g_fn, records_prefix, second_backward)
    assert len(hooked) == 1
    P.assert_staged_equals_monolithic(staged, mono, hooked[0], mod.last_backward_extras)
    return mod, mono, staged, f


def _first_records_case(P, whole, m, dense, **kw):
    """forward_projected of the first m records of `whole` against the operator on `whole` with every other point invalid"""
    q, t = view_pose()
    fw, _ = P.run_oracle(whole, q, t)
    assert fw.M >= m
    masked = P.only_points(whole, fw.point_id_in_camera_list[:m])
    n = whole.point_cloud.shape[0]
    mod, mono, staged, f = _case(P, masked, (0, n), q, t, dense, records_prefix=(whole, m), **kw)
    assert f.M == m and staged.records.shape == (m, 16)
    return mod, mono, staged, f


@pytest.mark.parametrize("m,n_keys", zip((1, 255, 256, 257, 513), (2, 502, 504, 505, 995)))
def test_block_tails_of_a_records_frame(P, m, n_keys):
    """m records = less than a block of k_boxes_from_records and of the records-mode k_keygen (mine = min(256, M - first)), a
    block less one, exactly one, one more, two and one more."""
    assert m in P.RECORD_COUNTS
    mod, mono, staged, f = _first_records_case(P, P.records_scene(), m, synth(5000, 96, 64, 0.12, seed=91))
    assert staged.n_keys == f.K == n_keys, (staged.n_keys, f.K)


@pytest.mark.parametrize("m", [1, 3])
def test_few_records_on_many_tiles(P, m):
    """One block of 256 threads clears the tile arrays of 1000 tiles (more than 3000 words: several trips of the clearing loop)
    over what a dense frame left there; a tile word it missed shows in the tile ranges, which are all but a few empty here."""
    whole = synth(3000, 640, 400, 0.05, seed=3)
    mod, mono, staged, f = _first_records_case(P, whole, m, synth(9000, 640, 400, 0.05, seed=91))
    assert staged.tile_points_start.shape == (1000,) and staged.n_keys == f.K
    assert np.array_equal(staged.tile_points_start, f.tile_points_start), "tile_points_start against the oracle"
    assert np.array_equal(staged.tile_points_end, f.tile_points_end), "tile_points_end against the oracle"
    assert ((f.tile_points_end - f.tile_points_start) == 0).sum() >= 1000 - f.K


def _seven(n):
    return tuple(int(x) for x in np.linspace(0, n, 8).astype(int))


@pytest.mark.parametrize("cuts", ["one_row_and_empty", "seven"])
@pytest.mark.parametrize("objects", [1, 3])
def test_records_of_shards(P, cuts, objects):
    """Records of several owners side by side: an empty shard in the middle and a single-row shard, then seven near-equal shards
    (blocks of 256 records straddle owners); with three objects under three poses the owners' records mix objects."""
    cuts = P.SHARD_CUTS if cuts == "one_row_and_empty" else _seven(1500)
    dense = synth(5000, 96, 64, 0.12, seed=91)
    if objects == 1:
        s = P.records_scene()
        q, t = view_pose()
    else:
        s, q, t, partial = P.multi_object_case(7, objects, n=1500, sigma0=0.08, width=96, height=64)
        assert not partial and len(np.unique(s.point_object_id)) == objects
    mod, mono, staged, f = _case(P, s, cuts, q, t, dense, seed=1)
    sizes = [fr.n_points for fr in staged.shard_frames]
    assert sizes == [hi - lo for lo, hi in zip(cuts[:-1], cuts[1:])] and f.M > 1024


def test_partial_tiles_on_a_records_frame(P):
    """250x203 with allow_partial_tiles on both paths: edge tiles that lie partly outside the image"""
    s = synth(4000, 250, 203, 0.08, seed=250)
    q, t = view_pose()
    mod, mono, staged, f = _case(P, s, (0, 1333, 2666, 4000), q, t, synth(8000, 250, 203, 0.08, seed=91), partial=True, seed=2)
    assert staged.tile_points_start.shape == (16 * 13,)


@pytest.mark.parametrize("wpt", [None, "2", "1"])
def test_cut_lists_and_heavy_tiles_on_a_records_frame(P, wpt, monkeypatch):
    """Lists over 512 entries at 64x64: the forward of a kept records frame stores cut records, its backward shares the heavy
    tiles among four waves and walks them in segments -- with 4, 2 and 1 waves per ordinary tile (GS_BWD_WAVES_PER_TILE, read by
    every call) -- and a second backward through the same frame repeats the first one's bits."""
    if wpt is not None:
        monkeypatch.setenv("GS_BWD_WAVES_PER_TILE", wpt)
    s = P.clustered_cut_scene()
    q, t = view_pose()
    mod, mono, staged, f = _case(P, s, (0, 3000), q, t, synth_clustered(6000, 64, 64, 0.05, sh_deg=3, seed=9), second_backward=True, seed=3)
    lens = staged.tile_points_end - staged.tile_points_start
    assert (lens > 512).any() and lens.max() == 1030, lens.max()
    if P.default_heavy_policy():
        assert staged.heavy_tiles > 0


@pytest.mark.parametrize("n,w,h,rows_per_pair", [(3000, 640, 400, 4), (2000, 1536, 1024, 1)])
def test_giant_points_without_the_projection_hint(P, n, w, h, rows_per_pair):
    """Four faint splats whose box is every tile: more than SUM_ROWS_GIANT = 1024 (point, tile) rows each, at four rows per pair
    (1000 tiles) and at one (6144 tiles).  A records frame has no largest-tile-count word from k_project, so k_sum_rows finds
    them by looking at every point."""
    s = P.giant_scene(n, w, h)
    q, t = view_pose()
    mod, mono, staged, f = _case(P, s, (0, n), q, t, synth(3 * n, w, h, 0.05, seed=91), seed=4)
    rows = staged.num_overlap_tiles.astype(np.int64) * rows_per_pair
    assert rows.max() > 1024 and (rows > 1024).sum() >= 3, (rows.max(), (rows > 1024).sum())
    assert staged.num_overlap_tiles.max() == (w // 16) * (h // 16)


@pytest.mark.parametrize("which", ["first_513_records", "shards"])
def test_sums_of_backward_projected_against_the_oracle(P, which):
    """backward_projected's (M,12) per-splat sums, put into the reference's scaling, against oracle.backward_sums: GRAD_TOL on
    max |a - ref| / max |ref| per column group (uv, Sigma', colour, opacity, magnitude), the pixel counts exactly.
    Measured worst group: 2.1e-7 (colour) on the first 513 records, 1.3e-7 (uv) on the shards' records."""
    dense = synth(5000, 96, 64, 0.12, seed=91)
    if which == "shards":
        mod, mono, staged, f = _case(P, P.records_scene(), P.SHARD_CUTS, *view_pose(), dense, seed=1)
    else:
        mod, mono, staged, f = _first_records_case(P, P.records_scene(), 513, dense)
    worst = P.assert_sums_parity(staged.sums, staged.point_alpha_after_activation, f, mono.g.cpu().numpy())
    print(f"{which}: M = {f.M}, K = {f.K}, worst column group {worst:.3g} of the bar's {P.GRAD_TOL}")
