"""GPU (-m gpu): the sparse gradient exchange between two processes sharing cuda:0, collectives over gloo (a one-GPU box has no
second card and RCCL needs one per rank).  Rank r renders view r of the scene of tests/test_gpu_multiprocess.py, packs the rows
its backward touched and calls distributed.sparse_reduce_point_gradients; a second backward of the same view is reduced with the
dense all_reduce_point_gradients.

Both ranks must hold the same union and the same bits.  With two ranks a + b is commutative, so on the union rows the merged
gradient equals the all-reduced one under == everywhere and bit for bit wherever the value is not a signed zero (the dense sum
adds +0.0 for a rank that does not list the row, which turns a -0.0 into +0.0); outside the union the all-reduced gradient is
zero."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_gpu_multiprocess import N_PTS, ROOT, _free_port, _grad_of_image, _input, _scene

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, out_dir, backend="gloo", own_device=False):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank if own_device else 0), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    from taichi_3d_gaussian_splatting_amd import GaussianPointCloudRasterisation as Rast
    from taichi_3d_gaussian_splatting_amd import distributed as gsd
    from taichi_3d_gaussian_splatting_amd.synthetic import view_pose
    gsd.init_from_env(backend)
    dev = torch.device("cuda", rank if own_device else 0)
    torch.cuda.set_device(dev)
    s = _scene()
    module = Rast(Rast.GaussianPointCloudRasterisationConfig())
    module.track_touched_rows = True
    q, t = view_pose(rank, world)

    def backward():
        inp = _input(s, 0, N_PTS, dev, q, t, requires_grad=True)       # fresh parameters: the forward normalises the quaternions in place
        img = module(inp)[0]
        img.backward(_grad_of_image(img.detach()))
        return inp.point_cloud.grad, inp.point_cloud_features.grad

    gp, gf = backward()
    local = module.last_touched_rows
    m_gp, m_gf, union, stats = gsd.sparse_reduce_point_gradients(gp, gf, local, zero=True)
    assert stats["collectives"] == 2 and 0 < stats["bytes_sent"] < stats["bytes_dense"] == 236 * N_PTS, stats
    assert stats["rows_local"] == int(local.count.item()) and int(stats["rows_union"].item()) == int(union.count.item())
    assert gsd._flat_base(m_gp, m_gf) is not None and union.n_points == N_PTS
    # a second backward of the same view on fresh parameters (the same bits), reduced densely
    d_gp, d_gf = backward()
    assert torch.equal(d_gp, gp) and torch.equal(d_gf, gf)
    assert gsd.all_reduce_point_gradients(d_gp, d_gf) in (1, 2)
    np.save(os.path.join(out_dir, f"union_{rank}.npy"), union.tensor().cpu().numpy())
    np.save(os.path.join(out_dir, f"local_{rank}.npy"), local.tensor().cpu().numpy())
    for name, x in (("m_gp", m_gp), ("m_gf", m_gf), ("d_gp", d_gp), ("d_gf", d_gf)):
        np.save(os.path.join(out_dir, f"{name}_{rank}.npy"), x.cpu().numpy())
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_sparse_exchange(tmp_path):
    _two_ranks(tmp_path, "gloo", False)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: the same exchange with one card per rank over RCCL (backend nccl)")
def test_two_ranks_on_two_gpus_sparse_exchange_over_rccl(tmp_path):
    _two_ranks(tmp_path, "nccl", True)


def _two_ranks(tmp_path, backend, own_device):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), backend, own_device), nprocs=world, join=True)
    load = lambda name, r: np.load(tmp_path / f"{name}_{r}.npy")
    union = load("union", 0)
    locals_ = [load("local", r) for r in range(world)]
    assert np.array_equal(union, load("union", 1))
    assert np.array_equal(union, np.union1d(locals_[0], locals_[1])) and 0 < union.size < N_PTS
    assert np.setdiff1d(locals_[0], locals_[1]).size > 0 and np.intersect1d(locals_[0], locals_[1]).size > 0
    out = np.setdiff1d(np.arange(N_PTS), union)
    for name in ("gp", "gf"):
        m0, m1, d0 = load("m_" + name, 0), load("m_" + name, 1), load("d_" + name, 0)
        assert np.array_equal(m0.view(np.uint32), m1.view(np.uint32))           # both ranks: the same bits, on every row (zero=True)
        assert (m0[union] == d0[union]).all()
        signed_zero = (m0[union] == 0)
        assert np.array_equal(m0[union].view(np.uint32)[~signed_zero], d0[union].view(np.uint32)[~signed_zero])
        assert not d0[out].view(np.uint32).any() and not m0[out].view(np.uint32).any()
        assert m0[union].any()
