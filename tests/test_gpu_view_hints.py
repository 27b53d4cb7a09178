"""GPU (-m gpu): the view table of a context (include/gs_view_hints.h; csrc/gs_common.h "the view table").

A context keeps the backward's tile order per view, keyed on the device by the pose of object 0, and dispatches the next forward
blend of a view in the order the view's own last backward left.  That is scheduling only: every setting of GS_VIEW_HINTS must
give the same bits, forward and backward, and whatever a slot holds must be a permutation of the tiles (an order that is none
would silently drop tiles).  Shapes: 64x48 (12 tiles) and 80x64 (20 tiles), 2000 points, poses 2 degrees apart.  Unset, the
switch gives images of fewer than 4096 tiles one slot (no order can help a launch the chip holds at once), so the tests of the
table's contents ask for their slots by number."""
import ctypes as C

import numpy as np
import pytest
import torch

from taichi_3d_gaussian_splatting_amd import _native
from taichi_3d_gaussian_splatting_amd.synthetic import synth, view_pose

pytestmark = pytest.mark.gpu

SWITCH = "GS_VIEW_HINTS"
DEFAULT_SLOTS = 64                                    # what an unset switch gives from 4096 tiles on; below, one slot and no lookup
SLOTS = "64"                                          # an explicit count holds at every size: the small shapes get their table with it
POSES = [view_pose(v, 8) for v in (2, 3, 4)]          # neighbours: 2 degrees apart
ROUNDS = 3
PRODUCTS = ("image", "depth", "alpha", "last", "count", "grad_pointcloud", "grad_pointcloud_features")


@pytest.fixture(scope="module")
def P():
    import parity_util
    return parity_util


def _read(ctx, frame=None, slot=-1):
    """gs_view_hints_read -> dict(S, T, keys (S,7), filled (S), order (T) of `slot` or None, frame_slots (read, write) or None)"""
    L = _native.lib()
    fn = L.gs_view_hints_read
    I32P = C.POINTER(C.c_int32)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, I32P, I32P, C.POINTER(C.c_float), I32P, C.c_int32, I32P, C.c_int32, I32P]
    fn.restype = C.c_int
    S, T = C.c_int32(), C.c_int32()
    rc = fn(ctx, None, -1, C.byref(S), C.byref(T), None, None, 0, None, 0, None)
    assert rc == 0, L.gs_last_error()
    S, T = S.value, T.value
    keys, filled = np.zeros((max(S, 1), 7), np.float32), np.zeros(max(S, 1), np.int32)
    order = np.full(max(T, 1), -1, np.int32)
    slots = np.zeros(2, np.int32)
    rc = fn(ctx, frame.handle if frame is not None else None, slot, None, None, keys.ctypes.data_as(C.POINTER(C.c_float)),
            filled.ctypes.data_as(I32P), S, order.ctypes.data_as(I32P), T, slots.ctypes.data_as(I32P))
    assert rc == 0, L.gs_last_error()
    return dict(S=S, T=T, keys=keys[:S], filled=filled[:S], order=order[:T] if slot >= 0 else None,
                frame_slots=(int(slots[0]), int(slots[1])) if frame is not None else None)


def _ctx(mod):
    return mod._ctx_for(torch.device("cuda:0"))


def _assert_slots_valid(ctx, extra=()):
    """Every filled slot (and every slot of `extra`) holds a permutation of the tiles."""
    tab = _read(ctx)
    for slot in list(np.flatnonzero(tab["filled"])) + list(extra):
        order = _read(ctx, slot=int(slot))["order"]
        assert np.array_equal(np.sort(order), np.arange(tab["T"])), (slot, order)
    return tab


def _scene(width, height, seed=31):
    return synth(2000, width, height, 0.08, sh_deg=3, seed=seed)


def _step(P, mod, scene, pose, backward=True):
    """One forward (+ backward of a fixed upstream gradient) -> (products by name as numpy, the forward's frame)"""
    q, t = pose
    if not backward:
        with torch.no_grad():
            image, depth, count = mod(P.make_input(scene, q, t, requires_grad=False))
        inp = None
    else:
        inp = P.make_input(scene, q, t)
        image, depth, count = mod(inp)
    frame = mod.last_frame
    lo = mod.last_forward_outputs
    r = dict(image=image, depth=depth, alpha=lo["pixel_accumulated_alpha"], last=lo["pixel_offset_of_last_effective_point"], count=count)
    r = {k: v.detach().cpu().numpy().copy() for k, v in r.items()}
    if backward:
        image.backward(2.0 * (image.detach() - 0.25))
        r["grad_pointcloud"] = inp.point_cloud.grad.cpu().numpy().copy()
        r["grad_pointcloud_features"] = inp.point_cloud_features.grad.cpu().numpy().copy()
    return r, frame


def _same(P, a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        P.assert_same_bits(a[k], b[k], (what, k))


def _cycle(P, monkeypatch, setting, scene, rounds=ROUNDS, check=None):
    """rounds x POSES of forward + backward on a fresh context under GS_VIEW_HINTS=setting (None: unset) -> (steps, module)"""
    if setting is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, setting)
    mod = P.module()
    steps = []
    for r in range(rounds):
        for v, pose in enumerate(POSES):
            got, frame = _step(P, mod, scene, pose)
            steps.append(got)
            if check:
                check(mod, r, v, frame)
    return steps, mod


@pytest.fixture(scope="module")
def hint_free(P):
    """The three poses at 64x48 with no hint at all, one round: what every other setting must reproduce, round after round."""
    mp = pytest.MonkeyPatch()
    try:
        steps, _ = _cycle(P, mp, "0", _scene(64, 48), rounds=1)
    finally:
        mp.undo()
    return steps


def test_every_setting_gives_the_same_bits(P, monkeypatch, hint_free):
    scene = _scene(64, 48)
    for setting in (None, SLOTS, "1", "0"):
        steps, mod = _cycle(P, monkeypatch, setting, scene)
        assert len(steps) == ROUNDS * len(POSES)
        for i, got in enumerate(steps):
            assert set(got) == set(PRODUCTS)
            _same(P, got, hint_free[i % len(POSES)], (setting, i))
        tab = _read(_ctx(mod))
        assert (tab["S"], tab["T"]) == {None: (1, 12), SLOTS: (64, 12), "1": (1, 12), "0": (0, 0)}[setting]
        if setting in (None, "1"):                         # one slot: every pose matches it, no frame looks its pose up
            assert _read(_ctx(mod), mod.last_frame)["frame_slots"] == (-2, -2) and _assert_slots_valid(_ctx(mod))["filled"].all()


def test_table_contents(P, monkeypatch):
    seen = {}

    def check(mod, r, v, frame):
        ctx = _ctx(mod)
        slots = _read(ctx, frame)["frame_slots"]
        if r == 0:
            assert slots == (v - 1, v), (v, slots)      # reads the nearest view seen so far (none at first), fills the lowest unfilled slot
            seen[v] = slots[1]
        else:
            assert slots == (seen[v], seen[v]), (r, v, slots)                                   # its own pose's slot, read and written
        if r == 0 and v == len(POSES) - 1:
            tab = _assert_slots_valid(ctx)
            assert tab["S"] == DEFAULT_SLOTS and tab["T"] == 12
            assert list(np.flatnonzero(tab["filled"])) == [0, 1, 2]
            for w, (q, t) in enumerate(POSES):
                P.assert_same_bits(tab["keys"][w], np.concatenate([q[0], t[0]]).astype(np.float32), w)

    _, mod = _cycle(P, monkeypatch, SLOTS, _scene(64, 48), rounds=2, check=check)
    assert len(set(seen.values())) == len(POSES)                                                # neighbours 2 degrees apart: different slots
    tab = _assert_slots_valid(_ctx(mod))
    assert list(np.flatnonzero(tab["filled"])) == [0, 1, 2]                                     # the same pose reuses its slot


def test_a_drifting_pose_keeps_its_slot(P, monkeypatch):
    """A pose that moves as pose optimisation moves it (0.02 degrees, 1e-3 of the scene's unit) is the same view; the key follows it."""
    monkeypatch.setenv(SWITCH, SLOTS)
    mod, scene = P.module(), _scene(64, 48)
    for pose in POSES:
        _step(P, mod, scene, pose)
    a = np.deg2rad(-3.0 + 0.02)                                                                 # POSES[0] = view 2 of 8 is -3 degrees about y
    q = np.array([[0.0, np.sin(a / 2), 0.0, np.cos(a / 2)]], np.float32)
    t = np.array([[1e-3, 0.0, -1e-3]], np.float32)
    _, frame = _step(P, mod, scene, (q, t))
    assert _read(_ctx(mod), frame)["frame_slots"] == (0, 0)
    tab = _assert_slots_valid(_ctx(mod))
    assert list(np.flatnonzero(tab["filled"])) == [0, 1, 2]
    P.assert_same_bits(tab["keys"][0], np.concatenate([q[0], t[0]]), "the key follows the pose")


def test_eviction(P, monkeypatch, hint_free):
    def check(mod, r, v, frame):
        tab = _assert_slots_valid(_ctx(mod))
        assert tab["S"] == 2
        slots = _read(_ctx(mod), frame)["frame_slots"]
        assert 0 <= slots[1] < 2 and -1 <= slots[0] < 2
        seen.append(slots[1])

    seen = []
    steps, mod = _cycle(P, monkeypatch, "2", _scene(64, 48), check=check)
    for i, got in enumerate(steps):
        _same(P, got, hint_free[i % len(POSES)], i)
    assert _read(_ctx(mod))["filled"].all()
    assert seen == [0, 1, 0, 1, 0, 1, 0, 1, 0]             # two unfilled slots, then the cursor's round robin: it moves when a slot is filled


def test_tile_grid_change(P, monkeypatch):
    monkeypatch.setenv(SWITCH, SLOTS)
    scenes = {12: _scene(64, 48), 20: _scene(80, 64)}
    fresh = {T: _step(P, P.module(), s, POSES[0])[0] for T, s in scenes.items()}
    mod = P.module()
    for T in (12, 20, 12):
        got, frame = _step(P, mod, scenes[T], POSES[0])
        tab = _read(_ctx(mod), frame)
        assert tab["T"] == T and tab["frame_slots"] == (-1, 0), (T, tab["frame_slots"])        # emptied: nothing to read, slot 0 to fill
        _same(P, got, fresh[T], T)
        got, frame = _step(P, mod, scenes[T], POSES[0])                                         # and the second frame of the grid finds the first
        assert _read(_ctx(mod), frame)["frame_slots"] == (0, 0)
        _same(P, got, fresh[T], T)
        assert list(np.flatnonzero(_assert_slots_valid(_ctx(mod))["filled"])) == [0]


def test_two_frames_in_flight(P, monkeypatch):
    monkeypatch.setenv(SWITCH, SLOTS)
    scene = _scene(64, 48)
    single = [_step(P, P.module(), scene, pose)[0] for pose in POSES[:2]]
    mod = P.module()
    _step(P, mod, scene, POSES[2])                                                              # something to read
    inps = [P.make_input(scene, *pose) for pose in POSES[:2]]
    images = [mod(inp)[0] for inp in inps]                                                      # forward A, forward B, both kept
    for k in (1, 0):                                                                            # backward B, backward A
        images[k].backward(2.0 * (images[k].detach() - 0.25))
    for k in (0, 1):
        P.assert_same_bits(images[k], single[k]["image"], k)
        P.assert_same_bits(inps[k].point_cloud.grad, single[k]["grad_pointcloud"], k)
        P.assert_same_bits(inps[k].point_cloud_features.grad, single[k]["grad_pointcloud_features"], k)
    tab = _assert_slots_valid(_ctx(mod))
    assert 2 <= tab["filled"].sum() <= 3                    # A and B both found slot 1 unfilled: they may share it


def test_corner_frames(P, monkeypatch):
    monkeypatch.setenv(SWITCH, SLOTS)
    scene = _scene(64, 48)
    fresh = _step(P, P.module(), scene, POSES[0])[0]
    # no point in camera: K = 0, k_tile_order is not launched
    mod = P.module()
    behind = _scene(64, 48)
    behind.point_cloud[:, 2] = -behind.point_cloud[:, 2]
    got, frame = _step(P, mod, behind, POSES[1])
    assert frame.n_keys == 0 and not got["image"].any()
    assert not _read(_ctx(mod))["filled"].any()
    _same(P, _step(P, mod, scene, POSES[0])[0], fresh, "after an empty frame")
    before = _assert_slots_valid(_ctx(mod))
    assert list(np.flatnonzero(before["filled"])) == [0]
    order_before = _read(_ctx(mod), slot=0)["order"]
    # no_grad: reads a slot, fills none
    got, frame = _step(P, mod, scene, POSES[1], backward=False)
    assert _read(_ctx(mod), frame)["frame_slots"][0] == 0
    for k in got:
        P.assert_same_bits(got[k], _step(P, P.module(), scene, POSES[1], backward=False)[0][k], k)
    after = _assert_slots_valid(_ctx(mod))
    assert np.array_equal(after["filled"], before["filled"]) and np.array_equal(P.bits(after["keys"][0]), P.bits(before["keys"][0]))
    assert np.array_equal(_read(_ctx(mod), slot=0)["order"], order_before)
    _same(P, _step(P, mod, scene, POSES[0])[0], fresh, "after a no_grad frame")


def test_frames_from_records(P, monkeypatch):
    """gs_forward_projected: no pose to key the frame by.  Its backward's order goes to the slot behind the keyed ones, its forward
    reads whichever slot was written last; the image is what it is without any hint."""
    from taichi_3d_gaussian_splatting_amd.stages import StagedRasteriser
    scene = P.records_scene()                                                                  # 96x64: 24 tiles
    q, t = view_pose()

    def render(setting):
        if setting is None:
            monkeypatch.delenv(SWITCH, raising=False)
        else:
            monkeypatch.setenv(SWITCH, setting)
        st = StagedRasteriser(P.module().config)
        inp = P.make_input(scene, q, t, requires_grad=False)
        rec, ids, shard = st.project_shard(inp)
        runs = []
        for _ in range(2):                                                                      # the second forward reads the first backward's order
            outs, frame = st.forward_projected(rec.contiguous(), inp.camera_info)
            sums, _mag = st.backward_projected(frame, outs, 2.0 * (outs.rasterized_image - 0.25))
            runs.append(dict(image=outs.rasterized_image.cpu().numpy().copy(), count=outs.pixel_valid_point_count.cpu().numpy().copy(),
                             last=outs.pixel_offset_of_last_effective_point.cpu().numpy().copy(), sums=sums.cpu().numpy().copy()))
            slots = _read(st._ctx_for(torch.device("cuda:0")), frame)["frame_slots"]
            assert slots == (-2, -2)
        return runs, st

    ref, _ = render("0")
    _same(P, ref[0], ref[1], "hint-free, twice")
    for setting in (SLOTS, "1", None):
        runs, st = render(setting)
        for r in runs:
            _same(P, r, ref[0], setting)
        ctx = st._ctx_for(torch.device("cuda:0"))
        tab = _read(ctx)
        assert tab["T"] == 24
        if setting == SLOTS:
            assert not tab["filled"].any()
            _assert_slots_valid(ctx, extra=[tab["S"]])
        else:
            assert tab["filled"].all()
            _assert_slots_valid(ctx)


def test_more_tiles_than_the_order_kernel_stages(P, monkeypatch):
    """2080x1024 = 8320 tiles: above the 8192 up to which k_tile_order keeps its work values in registers and puts the order
    together in LDS, so it loads in two rounds and stores tile by tile, to the frame and to the slot."""
    scene = synth(3000, 2080, 1024, 0.02, sh_deg=3, seed=33)
    pose = POSES[1]
    monkeypatch.setenv(SWITCH, "0")
    ref, _ = _step(P, P.module(), scene, pose)
    monkeypatch.delenv(SWITCH, raising=False)                  # unset: at this size the table has its 64 slots
    mod = P.module()
    first, _ = _step(P, mod, scene, pose)
    tab = _assert_slots_valid(_ctx(mod))
    assert tab["S"] == DEFAULT_SLOTS and tab["T"] == 8320 and list(np.flatnonzero(tab["filled"])) == [0]
    second, frame = _step(P, mod, scene, pose)
    assert _read(_ctx(mod), frame)["frame_slots"] == (0, 0)
    _same(P, first, ref, "first")
    _same(P, second, ref, "second")


def test_heavy_tiles_present(P, monkeypatch):
    """A clustered scene whose backward splits heavy tiles: they stand at the head of the stored order, and the next forward of the
    view, dispatched in that order, gives the hint-free bits."""
    scene = P.clustered_cut_scene()                                                             # 64x64: 16 tiles
    pose = view_pose()
    monkeypatch.setenv(SWITCH, "0")
    ref, _ = _step(P, P.module(), scene, pose)
    monkeypatch.setenv(SWITCH, SLOTS)
    mod = P.module()
    first, frame = _step(P, mod, scene, pose)
    n_heavy = frame.heavy_tiles()
    assert 0 < n_heavy < 16
    order = _read(_ctx(mod), slot=0)["order"]
    assert np.array_equal(np.sort(order), np.arange(16))
    # tile_work counts (splat, quadrant) evaluations, at most four per list entry: a heavy tile has at least twice the mean work, so
    # its list is longer than half the mean number of evaluations per tile / 4 -- and in this scene the heavy tiles are the longest lists
    length = (frame.export("tile_points_end") - frame.export("tile_points_start")).cpu().numpy()
    assert set(order[:n_heavy]) == set(np.argsort(-length, kind="stable")[:n_heavy]), (order, length)
    second, frame2 = _step(P, mod, scene, pose)
    assert _read(_ctx(mod), frame2)["frame_slots"] == (0, 0)
    _same(P, first, ref, "first")
    _same(P, second, ref, "second, in its own heavy-first order")
