"""GPU (-m gpu): the sort's first radix pass inside k_keygen (k_binning.hip) against the three-kernel pass it replaces.

With 8 or more depth bits in the key, digit 0 is the low byte of the depth code -- the same for all pairs of a point -- and k_keygen
stores every pair where a stable pass over that digit would have put it, from the [digit][block] pair counts the per-point kernel
leaves, for scenes of up to 4096 blocks of 256 rows.  GS_SORT_FIRST_PASS=0 (read on every call) keeps the full-pass loop.  Every case renders the same inputs on fresh contexts
with the switch on and off and asks for the same bits in the forward products, the raster exports, the scan of the tile counts and
both gradients; the fresh on-run also meets the oracle at the bars of parity_util.  Which path a frame took is read from the
library's own launch counts: k_sort_hist runs ceil(key bits / 8) times on the full-pass loop and once less on the fused path, so no
case can pass by silently taking the other one."""
import ctypes as C

import numpy as np
import pytest
import torch

from taichi_3d_gaussian_splatting_amd import _native
from taichi_3d_gaussian_splatting_amd.stages import StagedRasteriser
from taichi_3d_gaussian_splatting_amd.synthetic import synth, view_pose

pytestmark = pytest.mark.gpu

WIDE_SCALE = 2.0e8          # of test_sort_keys_wider_than_32_bits: depth codes of 31 bits
SWITCH = "GS_SORT_FIRST_PASS"


@pytest.fixture(scope="module")
def P():
    import parity_util
    return parity_util


def _g(image):
    return 2.0 * (image - 0.5)


def _bits_for(x):
    return max(int(x).bit_length(), 1)


def _counted(owner, fn):
    """fn() with the library's profiler on k_sort_hist alone -> (fn's result, launches of k_sort_hist)"""
    L = _native.lib()
    names = L.gs_kernel_names().decode().split(",")
    kid = names.index("k_sort_hist")
    ctx = owner._ctx_for(torch.device("cuda:0"))
    _native.check(L.gs_profile_enable(ctx, C.c_uint64(1 << kid)), "gs_profile_enable")
    r = fn()
    torch.cuda.synchronize()
    ms, cnt = (C.c_double * len(names))(), (C.c_int64 * len(names))()
    _native.check(L.gs_profile_read(ctx, ms, cnt, len(names), 1), "gs_profile_read")
    _native.check(L.gs_profile_enable(ctx, C.c_uint64(0)), "gs_profile_enable")
    return r, int(cnt[kid])


def _passes(key_bits, depth_bits, fused):
    """k_sort_hist launches of one binning"""
    return (key_bits + 7) // 8 - (1 if fused and depth_bits >= 8 else 0)


def _tile_bits(scene):
    T = ((scene.width + 15) // 16) * ((scene.height + 15) // 16)
    return _bits_for(max(T - 1, 1))


def _codes(r):
    """depth codes of the frame's pairs, from the reference's 64-bit (tile << 32) + code keys"""
    return (r.sort_key.astype(np.int64) & 0xFFFFFFFF)


def _render(P, monkeypatch, switch, scene, cfg=None, band=3, mod=None, voided=None, capped=False):
    """One forward + backward with the switch set -> Run (+ accumulated_num_overlap_tiles), with the launch count checked: a frame
    has one binning at its own key width, and one that was queued twice another before it, on predicted sizes that did not hold,
    with `voided` depth bits; capped: the scene has more blocks of rows than the fused path is taken for"""
    monkeypatch.setenv(SWITCH, switch)
    mod = mod or P.module(**(cfg or {}))
    r, launches = _counted(mod, lambda: P.run_monolithic(mod, scene, *view_pose(), band, _g))
    r["accumulated_num_overlap_tiles"] = r.frame.export("accumulated_num_overlap_tiles").cpu().numpy()
    r["mod"] = mod
    tb = _tile_bits(scene)
    attempts = [(r.sort_key_bits, r.sort_key_bits - tb)] if r.n_keys > 0 else []
    assert (voided is not None) == (r.sizing == "redone"), r.sizing
    if voided is not None:
        attempts.append((voided + tb, voided))
    want = sum(_passes(kb, db, switch == "1" and not capped) for kb, db in attempts)
    assert launches == want, (switch, launches, want, attempts)
    return r


def _same(P, a, b, what):
    P.assert_same_frame(a, b, what)
    P.assert_same_bits(a.accumulated_num_overlap_tiles, b.accumulated_num_overlap_tiles, (what, "accumulated_num_overlap_tiles"))
    assert a.sort_key_bits == b.sort_key_bits and a.n_keys == b.n_keys and a.sizing == b.sizing, what


def _on_off(P, monkeypatch, scene, cfg=None, oracle=True):
    """The scene on two fresh contexts, switch on and off: the same bits, and the on-run against the oracle -> (on, off)"""
    on = _render(P, monkeypatch, "1", scene, cfg)
    off = _render(P, monkeypatch, "0", scene, cfg)
    assert on.sizing == off.sizing == "exact"
    _same(P, on, off, "switch on against off")
    if oracle:
        ocfg = P.oracle_config(scene.width % 16 != 0 or scene.height % 16 != 0, **(cfg or {}))
        f, feat_after = P.run_oracle(scene, *view_pose(), ocfg)
        P.assert_forward_parity(on.mod, on.inp, on.outs, f, feat_after)
    return on, off


def _set_depth(s, rows, z):
    """Rows `rows` of the scene at depth z (scalar or array) with their image position kept"""
    rows = np.asarray(rows)
    z = np.broadcast_to(np.asarray(z, np.float64), rows.shape)
    old = s.point_cloud[rows, 2].astype(np.float64)
    s.point_cloud[rows, 0] = (s.point_cloud[rows, 0] * z / old).astype(np.float32)
    s.point_cloud[rows, 1] = (s.point_cloud[rows, 1] * z / old).astype(np.float32)
    s.point_cloud[rows, 2] = z.astype(np.float32)


def _depth_of_code(c, scale=100.0):
    """A depth whose code i32(depth * scale) is c: the middle of the code's interval"""
    return (np.asarray(c, np.float64) + 0.5) / scale


def test_blocks_shared_low_bytes_and_equal_codes(P, monkeypatch):
    """Three k_project blocks, the last one partial (700 rows), the middle one with no point in camera, a few rows masked; codes of
    8 to 10 bits; within a block and across blocks points whose codes share the low byte and differ above it (c, c + 256, c + 512),
    and runs of points with one code, whose pairs must stay in point order"""
    s = synth(700, 64, 48, 0.1, sh_deg=3, seed=700)
    s.point_cloud[256:512, 2] *= -1.0
    s.point_invalid_mask[[3, 130, 255, 520, 699]] = 1
    c = 210
    for base in (10, 100, 530, 650):                      # rows of block 0 and of block 2
        _set_depth(s, [base, base + 1, base + 2], _depth_of_code([c + 512, c, c + 256]))
    same = [20, 21, 22, 60, 200, 540, 541, 690]           # one code in two waves of block 0 and in block 2
    _set_depth(s, same, _depth_of_code(c + 256))
    s.point_cloud_features[same, 4:7] = np.log(0.5)       # a few tiles each
    on, off = _on_off(P, monkeypatch, s)
    codes = _codes(on)
    assert on.sort_key_bits - _tile_bits(s) >= 9 and codes.max() >= 256
    for k in (c, c + 256, c + 512):
        assert (codes == k).any(), k
    # the points of one code, as the pairs of the tile that has most of them list them: ascending in-camera offset
    keys, counts = np.unique(on.sort_key[codes == c + 256], return_counts=True)
    v = on.point_offset_with_sort_key[on.sort_key == keys[counts.argmax()]]
    assert v.size >= 3 and bool((np.diff(v) > 0).all()), v
    assert on.n_points_in_camera < 700 - 256


def test_one_box_over_every_tile_and_empty_boxes(P, monkeypatch):
    """One faint splat whose box is all 340 tiles of a 320x272 image among small ones -- one owner across two trips of the pair loop --
    and in-camera points right of the image whose box is empty"""
    s = P.giant_scene(600, 320, 272, 1)
    s.point_cloud[0] = [0.0, 0.0, 2.0]                     # on the optical axis, near
    fx = 0.6 * 320
    rows = np.array([5, 300, 599])
    s.point_cloud[rows, 0] = ((320 + 30 - 160) * s.point_cloud[rows, 2].astype(np.float64) / fx).astype(np.float32)
    s.point_cloud_features[rows, 4:7] = np.log(0.005)
    on, off = _on_off(P, monkeypatch, s)
    n = on.num_overlap_tiles
    assert n.max() == 340 and (n == 0).sum() >= 3, (n.max(), (n == 0).sum())
    assert on.sort_key_bits - _tile_bits(s) >= 8


@pytest.mark.parametrize("depth_bits,band", [(7, (1.0, 1.25)), (8, (1.5, 2.5)), (9, (3.0, 5.0))])
def test_depth_field_of_7_8_and_9_bits(P, monkeypatch, depth_bits, band):
    """Depths in a narrow band: the largest code below 128 (digit 0 holds a tile bit: the full-pass loop, whatever the switch says),
    in [128, 255] and in [256, 511]"""
    s = synth(500, 96, 64, 0.03, sh_deg=3, seed=depth_bits)
    _set_depth(s, np.arange(500), np.random.default_rng(depth_bits).uniform(band[0], band[1], 500))
    on, off = _on_off(P, monkeypatch, s)
    codes = _codes(on)
    assert 1 << (depth_bits - 1) <= codes.max() < 1 << depth_bits, codes.max()
    assert on.sort_key_bits - _tile_bits(s) == depth_bits


def test_keys_wider_than_32_bits(P, monkeypatch):
    s = synth(3000, 160, 96, 0.08, sh_deg=3, seed=4)
    on, off = _on_off(P, monkeypatch, s, cfg=dict(depth_to_sort_key_scale=WIDE_SCALE))
    assert on.sort_key_bits > 32
    assert int(on.sort_key.max() & 0xFFFFFFFF) > 2 ** 30


def test_exact_predicted_and_redone_frames_of_one_context(P, monkeypatch):
    """Frame 1 sized exactly, frame 2 on a prediction that holds, frame 3 with more pairs than the prediction has room for: queued
    twice, both times from the digit table k_project left once"""
    X, Y = synth(2000, 128, 96, 0.08, seed=53), synth(7000, 128, 96, 0.08, seed=54)
    runs = {}
    for switch in ("1", "0"):
        mod = P.module()
        x1 = _render(P, monkeypatch, switch, X, mod=mod)
        x2 = _render(P, monkeypatch, switch, X, mod=mod)
        assert (x1.sizing, x2.sizing) == ("exact", "predicted")
        mc = int(_codes(x2).max())
        y = _render(P, monkeypatch, switch, Y, mod=mod, voided=_bits_for(mc + mc // 4))      # the key width predicted (run_forward_tail)
        assert y.sizing == "redone" and y.n_keys > x2.n_keys + x2.n_keys // 4 + 4096, (y.sizing, x2.n_keys, y.n_keys)
        runs[switch] = (x1, x2, y)
    for a, b, what in zip(runs["1"], runs["0"], ("exact", "predicted", "redone")):
        _same(P, a, b, what + " frame, switch on against off")
    fresh = _render(P, monkeypatch, "1", Y)
    P.assert_same_frame(runs["1"][2], fresh, "the redone frame against a fresh context")
    P.assert_same_frame(runs["1"][1], runs["1"][0], "the predicted frame against the exact one")


def test_frame_with_no_pairs_then_an_ordinary_one(P, monkeypatch):
    X = synth(2000, 128, 96, 0.08, seed=53)
    behind = synth(2000, 128, 96, 0.08, seed=53)
    behind.point_cloud[:, 2] -= 50.0
    runs = {}
    for switch in ("1", "0"):
        mod = P.module()
        e = _render(P, monkeypatch, switch, behind, mod=mod)
        assert e.n_keys == 0 and e.n_points_in_camera == 0 and not e.rasterized_image.any()
        # (4096 pairs and one depth bit are what a context that has seen no pair predicts: the first attempt takes the full-pass loop)
        runs[switch] = (e, _render(P, monkeypatch, switch, X, mod=mod, voided=1))
        assert runs[switch][1].n_keys > 4096
    for a, b, what in zip(runs["1"], runs["0"], ("empty", "ordinary")):
        _same(P, a, b, what + " frame, switch on against off")
    P.assert_same_frame(runs["1"][1], _render(P, monkeypatch, "1", X), "after the empty frame against a fresh context")


def test_records_from_elsewhere(P, monkeypatch):
    """gs_forward_projected: k_boxes_from_records leaves the digit table, k_keygen's blocks are 256 consecutive records (no block
    offsets); 600 records are three blocks, the last one partial"""
    s = synth(600, 96, 64, 0.08, seed=7)
    runs = {}
    for switch in ("1", "0"):
        monkeypatch.setenv(SWITCH, switch)
        st = StagedRasteriser()
        r, launches = _counted(st, lambda: P.run_staged(st, s, (0, 600), *view_pose(), 3, _g))
        assert r.n_points_in_camera == 600 and r.sizing == "exact"
        db = r.sort_key_bits - _tile_bits(s)
        assert db >= 8 and launches == _passes(r.sort_key_bits, db, switch == "1"), (db, launches)
        runs[switch] = r
    on, off = runs["1"], runs["0"]
    P.assert_same_frame(on, off, "records frame, switch on against off")
    P.assert_same_bits(on.sums, off.sums, "sums")
    mono = _render(P, monkeypatch, "1", s)
    P.assert_same_frame(on, mono, "records frame against gs_forward")
    f, _ = P.run_oracle(s, *view_pose(), P.oracle_config())
    for name in P.RASTER_EXPORTS:
        assert np.array_equal(on[name], getattr(f, name)), name


MAX_BLOCKS = 4096           # gs_api.hip: GS_FIRST_PASS_MAX_BLOCKS, blocks of 256 rows up to which k_keygen does the first pass


@pytest.mark.parametrize("blocks", [MAX_BLOCKS, MAX_BLOCKS + 1])
def test_block_count_at_the_cap_and_one_past_it(P, monkeypatch, blocks):
    """2000 points followed by invalid rows up to `blocks` blocks of 256, the last block holding one row: at the cap k_keygen does the
    first pass, one block further the three-kernel pass runs whatever the switch says; the same bits either way"""
    import copy
    base = synth(2000, 128, 96, 0.08, seed=53)
    n = (blocks - 1) * 256 + 1
    s = copy.copy(base)
    s.point_cloud = np.zeros((n, 3), np.float32)
    s.point_cloud_features = np.zeros((n, 56), np.float32)
    s.point_invalid_mask = np.ones(n, np.int8)
    s.point_object_id = np.zeros(n, np.int32)
    s.point_cloud[:2000], s.point_cloud_features[:2000], s.point_invalid_mask[:2000] = base.point_cloud, base.point_cloud_features, 0
    capped = blocks > MAX_BLOCKS
    on = _render(P, monkeypatch, "1", s, capped=capped)
    off = _render(P, monkeypatch, "0", s)
    _same(P, on, off, "switch on against off")
    small = _render(P, monkeypatch, "1", base)
    for name in P.FORWARD_PRODUCTS + P.RASTER_EXPORTS:
        P.assert_same_bits(on[name], small[name], ("against the 2000 rows alone", name))
    assert on.sort_key_bits - _tile_bits(s) >= 8 and on.n_keys > 0
