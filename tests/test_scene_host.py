"""CPU: GaussianPointCloudScene -- the constructor's state, the torch half of initialize() against the reference's formulas
(GaussianPointCloudScene.py:85-127) restated here in float64, files, and the refusal to initialise without a GPU."""
import numpy as np
import pytest
import torch

import knn_ref
from knn_ref import logit_bar
from taichi_3d_gaussian_splatting_amd import GaussianPointCloudScene as Scene, scene_io
from taichi_3d_gaussian_splatting_amd.GaussianPointCloudScene import initial_features

Config = Scene.PointCloudSceneConfig
C0 = 0.28209479177387814


def test_config_has_the_references_fields_and_defaults():
    import dataclasses
    got = {f.name: f.default for f in dataclasses.fields(Config)}
    assert got == dict(num_of_features=56, max_num_points_ratio=None, add_sphere=False, sphere_radius_factor=4.0,
                       num_points_sphere=10000, max_initial_covariance=None, initial_alpha=-2.0, initial_covariance_ratio=1.0)


def test_constructor_state_with_preallocated_rows():
    x = knn_ref.uniform(101, seed=1)
    scene = Scene(x, Config(max_num_points_ratio=1.5))
    total = int(101 * 1.5)
    assert {k: (tuple(v.shape), v.dtype) for k, v in scene.named_parameters()} == {
        "point_cloud": ((total, 3), torch.float32), "point_cloud_features": ((total, 56), torch.float32)}
    assert {k: (tuple(v.shape), v.dtype) for k, v in scene.named_buffers()} == {
        "point_invalid_mask": ((total,), torch.int8), "point_object_id": ((total,), torch.int32)}
    assert scene.point_invalid_mask.tolist() == [0] * 101 + [1] * (total - 101)
    assert scene.point_cloud.detach()[:101].numpy().tobytes() == x.tobytes() and not scene.point_cloud.detach()[101:].any()
    assert not scene.point_cloud_features.detach().any() and not scene.point_object_id.any()
    pc, ft = scene()
    assert pc is scene.point_cloud and ft is scene.point_cloud_features
    # features given: padded alike; no ratio: no extra rows
    feats = torch.ones(101, 56)
    scene = Scene(torch.from_numpy(x), Config(max_num_points_ratio=2.0), point_cloud_features=feats)
    assert scene.point_cloud_features.shape == (202, 56) and (scene.point_cloud_features.detach()[:101] == 1).all()
    assert not scene.point_cloud_features.detach()[101:].any()
    assert Scene(x, Config()).point_cloud.shape == (101, 3)
    with pytest.raises(AssertionError):
        Scene(x, Config(max_num_points_ratio=1.0))


@pytest.mark.parametrize("colours", [False, True])
@pytest.mark.parametrize("ratio,largest", [(1.0, None), (0.5, 0.02)])
def test_initial_features_are_the_references_formulas(colours, ratio, largest):
    rng = np.random.default_rng(3)
    x = knn_ref.uniform(600, seed=2)
    x[9] = x[10] = x[12] = x[8]                          # four valid copies of one point: all three distances zero, the lower clip
    mask = (np.arange(600) % 4 == 3).astype(np.int8)
    valid = mask == 0
    mean64 = knn_ref.mean_distance(x, 3, mask)[valid]
    assert mean64.min() == 0.0
    rgb = rng.uniform(-10, 300, (int(valid.sum()), 3)) if colours else None
    before = torch.from_numpy(rng.normal(size=(600, 56)).astype(np.float32))
    ft = before.clone()
    cfg = Config(initial_covariance_ratio=ratio, max_initial_covariance=largest, initial_alpha=-1.25)
    torch.manual_seed(0)
    initial_features(ft, torch.from_numpy(mask), torch.from_numpy(knn_ref.mean_distance(x, 3, mask, np.float32)[valid]), cfg, rgb)
    got = ft.numpy().astype(np.float64)
    # columns 4:7: log(clip(mean * ratio, 1e-6, max)) on valid rows (float64 here, f32 there: a few 2^-24 on values of size <= 14)
    want = np.log(np.clip(mean64 * ratio, 1e-6, largest))
    assert np.abs(got[valid, 4:7] - want[:, None]).max() < 4e-6
    assert (got[valid, 4:7].min(axis=1) == got[valid, 4:7].max(axis=1)).all()
    assert np.abs(got[valid, 4].min() - np.log(1e-6)) < 4e-6
    if largest is not None:
        assert abs(got[valid, 4].max() - np.log(largest)) < 4e-6 and (mean64 * ratio > largest).any()
    assert (ft[~valid, 4:7] == before[~valid, 4:7]).all()
    # every row: unit quaternion, alpha, SH
    assert np.abs(np.linalg.norm(got[:, 0:4], axis=1) - 1).max() < 1e-6 and (got[:, 0:4] >= 0).all()
    assert len(np.unique(got[:, 0])) > 500
    assert (got[:, 7] == -1.25).all()
    dc = (8, 24, 40)
    rest = [c for c in range(8, 56) if c not in dc]
    assert not got[:, rest].any()
    assert (got[~valid][:, dc] == 1).all()
    if not colours:
        assert (got[:, dc] == 1).all()
    else:
        c = np.clip(rgb / 255.0, 0.0, 0.99)
        with np.errstate(divide="ignore"):
            want = np.log(c / (1.0 - c)) / C0
        fin = np.isfinite(want)                          # a colour clamped to 0: logit = -inf in both
        assert (np.isneginf(got[valid][:, dc]) == ~fin).all() and (~fin).any()
        assert (np.abs(got[valid][:, dc][fin] - want[fin]) <= logit_bar(c, want)[fin]).all()


def _trained_file(tmp_path, n=50):
    rng = np.random.default_rng(4)
    pc, ft = rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 56)).astype(np.float32)
    path = str(tmp_path / "trained.parquet")
    scene_io.save_parquet(path, pc, ft)
    return path, pc, ft


def test_a_file_with_features_round_trips_on_the_cpu(tmp_path):
    path, pc, ft = _trained_file(tmp_path)
    scene = Scene.from_parquet(path, Config(max_num_points_ratio=1.5), device="cpu")
    assert scene.point_cloud.device.type == "cpu" and scene.point_cloud.shape == (75, 3)
    assert scene.point_cloud.detach()[:50].numpy().tobytes() == pc.tobytes()
    assert scene.point_cloud_features.detach()[:50].numpy().tobytes() == ft.tobytes()
    assert scene.point_invalid_mask.tolist() == [0] * 50 + [1] * 25
    again = str(tmp_path / "again.parquet")
    scene.to_parquet(again)
    pc2, ft2 = scene_io.load_parquet(again)
    assert pc2.tobytes() == pc.tobytes() and ft2.tobytes() == ft.tobytes()
    ply = str(tmp_path / "scene.ply")
    scene.to_ply(ply)
    pc3, ft3 = scene_io.load_inria_ply(ply, normalise_rotation=False)
    assert pc3.tobytes() == pc.tobytes() and ft3.tobytes() == ft.tobytes()
    assert Scene.from_parquet(path, device="cpu").point_cloud.shape == (50, 3)         # the default configuration


def _bare_file(tmp_path, colours=True):
    import pandas as pd
    rng = np.random.default_rng(5)
    df = pd.DataFrame(rng.normal(size=(40, 3)).astype(np.float32), columns=["x", "y", "z"])
    if colours:
        for i, c in enumerate("rgb"):
            df[c] = rng.integers(0, 256, 40).astype(np.uint8)
    path = str(tmp_path / ("bare_rgb.parquet" if colours else "bare.parquet"))
    df.to_parquet(path)
    return path, df


def test_a_bare_cloud_is_read_but_not_initialised_without_a_gpu(tmp_path):
    path, df = _bare_file(tmp_path)
    pc, ft, rgb = scene_io.load_parquet_columns(path)
    assert ft is None and pc.dtype == np.float32 and pc.tobytes() == df[["x", "y", "z"]].to_numpy().tobytes()
    assert rgb.shape == (40, 3) and (rgb == df[["r", "g", "b"]].to_numpy()).all()
    assert scene_io.load_parquet_columns(_bare_file(tmp_path, colours=False)[0])[2] is None
    with pytest.raises(ValueError, match="holds no trained features"):                 # as before
        scene_io.load_parquet(path)
    with pytest.raises(RuntimeError, match="GPU"):
        Scene.from_parquet(path, Config(), device="cpu")
    scene = Scene(pc, Config())
    with pytest.raises(RuntimeError, match=r"GPU.*move the module"):
        scene.initialize()
    assert not scene.point_cloud_features.detach().any()                               # refused before anything was written
    trained = _trained_file(tmp_path)[0]
    assert scene_io.load_parquet_columns(trained)[1].shape == (50, 56) and scene_io.load_parquet_columns(trained)[2] is None


def test_sphere_points():
    from taichi_3d_gaussian_splatting_amd.GaussianPointCloudScene import _add_sphere
    pc = np.array([[0, 0, 0], [2, 1, 0], [-2, 0.5, 0.25]], np.float32)
    rgb = np.zeros((3, 3), np.float32)
    out, colours = _add_sphere(pc, rgb, 4.0, 200)
    assert out.dtype == np.float32 and out.shape == (203, 3) and out[:3].tobytes() == pc.tobytes()
    assert np.allclose(np.linalg.norm(out[3:], axis=1), 4.0 * 2.0, rtol=1e-6)          # half the largest extent (4) times the factor
    assert colours.shape == (203, 3) and (colours[3:] == 127).all()
    assert _add_sphere(pc, None, 4.0, 5)[1] is None
    assert "GaussianPointCloudScene" in __import__("taichi_3d_gaussian_splatting_amd").__dict__
