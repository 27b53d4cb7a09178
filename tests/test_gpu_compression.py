"""GPU (-m gpu): compressed scene files end to end (compression.py on vq.py's k-means): a 3000-row scene whose higher-band SH
coefficients are 24 planted prototypes plus noise (the generator's own are independent draws, incompressible by construction),
32 codes, 5 iterations, then save, load, decode and render.

The picture of the decoded scene is held against that of the same scene compressed by a float64 k-means written in torch here
(same initial rows, same codec): its PSNR against the original may fall short of the float64 one by a margin only, because
near-ties may resolve differently in f32.  profiles/vq_margins.json records both PSNRs as measured on the GPU and the margin:
twice the observed gap, at least 0.1 dB."""
import dataclasses
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast
from taichi_3d_gaussian_splatting_amd import compression, scene_io, vq
from taichi_3d_gaussian_splatting_amd.compose import SceneComposition
from taichi_3d_gaussian_splatting_amd.GaussianPointCloudScene import GaussianPointCloudScene
from taichi_3d_gaussian_splatting_amd.synthetic import scene_input, synth, view_pose

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGINS = os.path.join(ROOT, "profiles", "vq_margins.json")
REST = list(compression.REST_COLUMNS)
CODES, ITERS, SEED = 32, 5, 0


def planted_scene():
    s = synth(3000, 96, 64, 0.05)
    rng = np.random.default_rng(0)
    prototypes = rng.normal(0.0, 0.3, (24, 45))
    ft = s.point_cloud_features.copy()
    ft[:, REST] = (prototypes[rng.integers(0, 24, 3000)] + rng.normal(0.0, 0.01, (3000, 45))).astype(np.float32)
    return dataclasses.replace(s, point_cloud_features=ft)


def holder(s):
    return SimpleNamespace(point_cloud=torch.tensor(s.point_cloud, device=DEV), point_cloud_features=torch.tensor(s.point_cloud_features, device=DEV),
                           point_invalid_mask=torch.tensor(s.point_invalid_mask, device=DEV))


def render(s, point_cloud=None, features=None):
    q, t = view_pose(0)
    if point_cloud is not None:
        s = dataclasses.replace(s, point_cloud=np.asarray(point_cloud.cpu()), point_cloud_features=np.asarray(features.cpu()))
    with torch.no_grad():
        return Rast(Rast.GaussianPointCloudRasterisationConfig())(scene_input(s, q, t, DEV))[0]


def psnr(a, b):
    return float(10 * torch.log10(1.0 / torch.mean((torch.clamp(a, 0, 1) - torch.clamp(b, 0, 1)).double() ** 2)))


def float64_kmeans(x, rows, iters):
    """Lloyd's iterations in float64 torch operations from the centroids x[rows] -> (codebook float32, labels)"""
    x = x.double()
    codebook = x[rows].clone()
    for _ in range(iters):
        labels = torch.cdist(x, codebook).argmin(1)
        sums = torch.zeros_like(codebook).index_add_(0, labels, x)
        counts = torch.bincount(labels, minlength=codebook.shape[0])
        codebook = torch.where(counts[:, None] > 0, sums / counts.clamp_min(1)[:, None], codebook)
    return codebook.float(), torch.cdist(x, codebook).argmin(1)


def psnr_pair(s, compressed):
    """-> (PSNR of the package's compressed scene, PSNR of the float64 k-means' one), both decoded and against the original"""
    original = render(s)
    x = torch.tensor(s.point_cloud_features[:, REST], device=DEV)
    codebook, labels = float64_kmeans(x, vq.initial_rows(3000, CODES, SEED).to(DEV), ITERS)
    reference = compression.encode(s.point_cloud, s.point_cloud_features, labels, codebook)
    return psnr(render(s, *compressed.decode()), original), psnr(render(s, *reference.decode()), original)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("compression")
    s = planted_scene()
    compressed = compression.compress(holder(s), codes=CODES, iters=ITERS, seed=SEED)
    path, parquet = str(tmp / "scene.npz"), str(tmp / "scene.parquet")
    compressed.save(path)
    scene_io.save_parquet(parquet, s.point_cloud, s.point_cloud_features)
    return SimpleNamespace(s=s, compressed=compressed, path=path, parquet=parquet, loaded=compression.load(path))


def test_file_shapes_sizes_and_decoded_values(case):
    c, s = case.loaded, case.s
    for name in compression.KEYS[1:]:
        assert np.array_equal(getattr(c, name), getattr(case.compressed, name)), name
    assert c.xyz.shape == (3000, 3) and c.q.shape == (3000, 4) and c.sh_index.shape == (3000,) and c.sh_index.dtype == np.uint8
    assert c.codebook.shape == (CODES, 45) and c.codebook.dtype == np.float16
    assert os.path.getsize(case.path) < os.path.getsize(case.parquet) / 4
    assert np.bincount(c.sh_index, minlength=CODES).min() > 0       # no code is empty
    pc, ft = c.decode()
    pc, ft = pc.numpy(), ft.numpy()
    assert np.array_equal(pc, s.point_cloud)
    cols = [0, 1, 2, 3, 4, 5, 6, 7, 8, 24, 40]
    x = s.point_cloud_features[:, cols].astype(np.float64)
    assert np.all(np.abs(ft[:, cols] - x) <= np.maximum(2.0 ** -11 * np.abs(x), 2.0 ** -25))
    assert np.array_equal(ft[:, REST], c.codebook.astype(np.float32)[c.sh_index])
    assert len(case.compressed.history) == ITERS + 1 and case.compressed.history[-1] < case.compressed.history[0]


def test_picture_quality_reaches_the_float64_k_means(case):
    recorded = json.load(open(MARGINS))
    assert recorded["margin_db"] == pytest.approx(max(0.1, 2.0 * max(recorded["psnr_float64_db"] - recorded["psnr_hip_db"], 0.0)))
    got, want = psnr_pair(case.s, case.compressed)
    print(f"PSNR of decoded against original: package {got:.4f} dB, float64 k-means {want:.4f} dB, margin {recorded['margin_db']} dB")
    assert got >= want - recorded["margin_db"]
    assert np.isfinite(got) and np.isfinite(want)


def test_a_non_finite_sh_coefficient_is_refused(case):
    h = holder(case.s)
    h.point_cloud_features[5, 30] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        compression.compress(h, codes=8, iters=1)
    h.point_invalid_mask[5] = 1                                     # an invalid row is not kept, so it does not matter
    assert len(compression.compress(h, codes=8, iters=1)) == 2999


def test_visibility_weights_see_what_the_camera_sees(case):
    s = case.s
    pc, ft = s.point_cloud.copy(), s.point_cloud_features.copy()
    pc[0], pc[1] = [0.0, 0.0, -5.0], [0.0, 0.0, 1.5]               # behind the camera; in front of everything, in the middle
    ft[1, 4:7], ft[1, 7] = np.log(0.05), 4.0
    q, t = view_pose(0)
    info = scene_input(s, q, t, DEV).camera_info
    h = holder(dataclasses.replace(s, point_cloud=pc, point_cloud_features=ft))
    w = compression.visibility_weights(h, (torch.tensor(q), torch.tensor(t), info))
    assert w.shape == (3000,) and w.dtype == torch.float32 and bool(torch.isfinite(w).all()) and float(w.min()) >= 0.0
    assert float(w[0]) == 0.0 and float(w[1]) > 1.0
    two = compression.visibility_weights(h, (torch.tensor(np.concatenate([q, q])), torch.tensor(np.concatenate([t, t])), [info, info]))
    assert torch.allclose(two, w + w, rtol=1e-4, atol=1e-6)        # f32 sums over pixels, whose order the channels' backward does not fix
    weighted = compression.compress(h, codes=CODES, iters=2, weights="visibility", poses=(torch.tensor(q), torch.tensor(t), info))
    assert len(weighted) == 3000 and weighted.codebook.shape == (CODES, 45)
    with pytest.raises(ValueError, match="poses"):
        compression.compress(h, weights="visibility")


def test_compressed_files_load_wherever_scenes_do(case):
    pc, ft = case.loaded.decode()
    want = render(case.s, pc, ft)
    scene = GaussianPointCloudScene.from_compressed(case.path, device=DEV)
    assert torch.equal(scene.point_cloud.detach().cpu(), pc) and torch.equal(scene.point_cloud_features.detach().cpu(), ft)
    composition = SceneComposition([case.path], device=DEV)
    q, t = view_pose(0)
    info = scene_input(case.s, q, t, DEV).camera_info
    for sc in (scene, composition.scene):
        with torch.no_grad():
            got = Rast(Rast.GaussianPointCloudRasterisationConfig())(Rast.GaussianPointCloudRasterisationInput(
                point_cloud=sc.point_cloud, point_cloud_features=sc.point_cloud_features, point_object_id=sc.point_object_id,
                point_invalid_mask=sc.point_invalid_mask, camera_info=info, q_pointcloud_camera=torch.tensor(q, device=DEV),
                t_pointcloud_camera=torch.tensor(t, device=DEV), color_max_sh_band=3))[0]
        assert torch.equal(got, want)
    again = str(case.path)[:-4] + "_again.npz"
    written = scene.to_compressed(again, codes=CODES, iters=1)
    assert len(written) == 3000 and len(compression.load(again)) == 3000
