"""CPU: the references that the records-frame tests (test_gpu_records_frames.py) compare against agree with each other.  The oracle
has the staged path's four halves of its own (pack_records, forward_from_projected, backward_sums, backward_points); the GPU
tests compare the staged path with the monolithic operator and the monolithic operator with oracle.forward / oracle.backward, so
what ties the two is shown here: a frame rendered from the first m records is the frame of the scene with every other point
invalid, the records of shards put side by side are the records of the whole, and the two backward halves chained are the
backward."""
import numpy as np
import pytest

import parity_util as P
from oracle import oracle
from taichi_3d_gaussian_splatting_amd.synthetic import view_pose

RASTER = ("sort_key", "point_offset_with_sort_key", "tile_points_start", "tile_points_end", "num_overlap_tiles") + P.FORWARD_PRODUCTS


@pytest.fixture(scope="module")
def whole():
    s = P.records_scene()
    q, t = view_pose()
    f, feat_after = P.run_oracle(s, q, t)
    assert f.M == 1500                                  # every point in camera: record i is point i
    return s, q, t, f, oracle.pack_records(f)


@pytest.mark.parametrize("m,n_keys", zip(P.RECORD_COUNTS, (2, 502, 504, 505, 995)))
def test_frame_from_the_first_m_records_is_the_frame_of_those_points(whole, m, n_keys):
    s, q, t, f, records = whole
    fr = oracle.forward_from_projected(records[:m], s.height, s.width)
    fm, _ = P.run_oracle(P.only_points(s, f.point_id_in_camera_list[:m]), q, t)
    assert fr.M == fm.M == m and fr.K == fm.K == n_keys, (fr.M, fm.M, fr.K, fm.K)
    P.assert_same_bits(oracle.pack_records(fm), records[:m], "records of the masked scene")
    for name in RASTER:
        a, b = getattr(fr, name), getattr(fm, name)
        assert a.shape == b.shape and a.dtype == b.dtype, name
        P.assert_same_bits(a, b, name)


def test_records_of_shards_side_by_side_are_the_records_of_the_whole(whole):
    s, q, t, f, records = whole
    parts = []
    for lo, hi in zip(P.SHARD_CUTS[:-1], P.SHARD_CUTS[1:]):
        fs, _ = P.run_oracle(P.shard_of(s, lo, hi), q, t)
        assert fs.M == hi - lo
        parts.append(oracle.pack_records(fs))
    assert [p.shape[0] for p in parts] == [1, 299, 0, 1200]
    P.assert_same_bits(np.concatenate(parts), records, "concatenated records")


def test_backward_sums_then_backward_points_is_the_backward(whole):
    s, q, t, f, records = whole
    g = (2.0 * (f.rasterized_image - np.random.default_rng(1).uniform(0, 1, f.rasterized_image.shape))).astype(np.float32)
    ref = oracle.backward(f, g, 3)
    sums, mag_img = oracle.backward_sums(f, g)
    assert sums.shape == (f.M, 12) and np.abs(sums[:, :10]).max() > 0
    got = oracle.backward_points(f, sums, 3)
    got["magnitude_grad_viewspace_on_image"] = mag_img
    for name in ("grad_pointcloud", "grad_pointcloud_features", "grad_viewspace", "magnitude_grad_viewspace",
                 "magnitude_grad_viewspace_on_image", "num_affected_pixels"):
        assert got[name].shape == ref[name].shape, name
        P.assert_same_bits(got[name], ref[name], name)
    # and from the frame rendered from the records (what a renderer that owns no points holds): the same sums
    fr = oracle.forward_from_projected(records, s.height, s.width)
    sums_r, mag_r = oracle.backward_sums(fr, g)
    P.assert_same_bits(sums_r, sums, "sums of the records frame")
    P.assert_same_bits(mag_r, mag_img, "magnitude image of the records frame")
