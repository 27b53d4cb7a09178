"""GPU (-m gpu): the three calls of include/gs_mcmc.h against tests/mcmc_ref.py, the header restated in numpy.

Sizes: one row, around one wave (63, 64, 65), around one block (255, 256, 257) and several blocks with a partial last one (1500).
Every scene of five rows or more mixes valid, free (mask 1) and mask-2 rows; a scene of one row is one valid row.
Past 1024 blocks (MC.N_LARGE = 1025 x 256 + 3 rows, where the one-block kernels give a thread two block sums, and the sizes around
1024 x 256) and where the sampler's draws land on a prefix: the scenes of tests/mcmc_cases.py, whose conditions
tests/test_mcmc_ref_host.py asserts on the CPU.  On the host the large noise case takes 2 s (two float64 references), the large
regulariser case 0.6 s, each large relocation case 0.6 s to 1.3 s and 0.6 s for its moment tensors."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mcmc_cases as MC
import mcmc_ref
from mcmc_cases import MASK_PATTERN

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 255, 256, 257, 1500]
DEV = "cuda:0"
_scenes = {}


def make_scene(n, seed=0, dead_share=0.1):
    """-> dict of numpy arrays pc, ft, mask, obj (cached: never edited)"""
    key = (n, seed, dead_share)
    if key not in _scenes:
        rng = np.random.default_rng(1000 * seed + n)
        ft = rng.normal(0.0, 0.6, (n, 56)).astype(np.float32)
        ft[:, 4:7] = rng.normal(-3.0, 0.5, (n, 3)).astype(np.float32)
        ft[:, 7] = rng.normal(0.0, 3.0, n).astype(np.float32)
        dead = rng.random(n) < dead_share
        ft[dead, 7] = rng.uniform(-9.0, -5.4, int(dead.sum())).astype(np.float32)
        _scenes[key] = dict(pc=rng.normal(0.0, 1.0, (n, 3)).astype(np.float32), ft=ft,
                            mask=np.array([MASK_PATTERN[i % 10] for i in range(n)], np.int8),
                            obj=rng.integers(0, 5, n).astype(np.int32))
    return _scenes[key]


def on_device(s, **replace):
    s = dict(s, **replace)
    return SimpleNamespace(point_cloud=torch.tensor(s["pc"], device=DEV), point_cloud_features=torch.tensor(s["ft"], device=DEV),
                           point_invalid_mask=torch.tensor(s["mask"], device=DEV), point_object_id=torch.tensor(s["obj"], device=DEV))


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({4: np.uint32, 1: np.uint8, 8: np.uint64}[a.dtype.itemsize])


# ---- noise -------------------------------------------------------------------------------------------------------------
# The gate closes fast: at opacity 0.5 it is 3e-22, and above 0.875 its exponent is clamped and it is 6e-39, below the smallest
# normal f32.  At a training run's noise_scale (noise_lr x position lr = 5e5 x 1.6e-4 = 80) the products Sigma_ij v_j of such rows
# are subnormal, where an f32 carries fewer than 24 bits and no relative bound can hold.  So the float64 comparison runs twice
# over every row: at LARGE, where every product of every row is a normal number, and at 80, where the bound is asserted on the
# rows whose products are all normal (the others are covered at LARGE by the same code) and everything else is asserted on all.
NOISE = dict(noise_scale=80.0, seed=0x1234567890ABCDEF, step=17)
LARGE = 1e12
SMALLEST_NORMAL = 2.0 ** -126


def noise_scene(n):
    s = make_scene(n)
    ft = s["ft"].copy()
    if n > 20:
        ft[5, 7] = 10.0                 # an opaque row: the gate closes
        ft[7, 5] = np.nan               # a NaN log-scale: the row must stay
    return dict(s, ft=ft)


def delta_from_zero(s, scale, step=NOISE["step"], seed=NOISE["seed"]):
    """the call on the scene moved to the origin: the result IS the delta, with no rounding of the addition"""
    from taichi_3d_gaussian_splatting_amd import mcmc
    dev = on_device(s, pc=np.zeros_like(s["pc"]))
    mcmc.inject_noise(dev, scale, step, seed=seed)
    return dev.point_cloud.cpu().numpy()


@pytest.mark.parametrize("n", SIZES + [MC.N_LARGE])
def test_noise_against_float64(n):
    from taichi_3d_gaussian_splatting_amd import mcmc
    s = noise_scene(n)
    for scale in (LARGE, NOISE["noise_scale"]):
        delta, magnitude, moves, smallest = mcmc_ref.noise(s["ft"], s["mask"], scale, NOISE["seed"], NOISE["step"], with_smallest_term=True)
        got = delta_from_zero(s, scale)
        assert (bits(got[~moves]) == 0).all()
        normal = moves & (smallest >= SMALLEST_NORMAL)
        if scale == LARGE:
            assert np.array_equal(normal, moves)                                # every moving row is compared
        err = np.abs(got.astype(np.float64) - delta)
        worst = np.max(err[normal] / magnitude[normal]) if normal.any() else 0.0
        print(f"noise n={n} scale={scale:g}: {int(normal.sum())} of {int(moves.sum())} moving rows, largest |delta - ref| / magnitude = {worst:.3g} (bar 2e-5)")
        assert (err[normal] <= 2e-5 * magnitude[normal]).all()
        assert (np.abs(got) <= 1.001 * magnitude + 1e-44).all()                 # and no row moves further than its terms allow
    if n > 20:
        assert s["mask"][5] == 0 and s["mask"][7] == 0
        assert moves[5] and np.abs(got[5]).max() < 1e-30
        assert not moves[7]
    # the scene's own positions: x + delta in one f32 addition; every row that is not valid keeps every bit, the features too
    dev = on_device(s)
    mcmc.inject_noise(dev, NOISE["noise_scale"], NOISE["step"], seed=NOISE["seed"])
    want = np.where(moves[:, None], s["pc"] + got, s["pc"])
    assert np.array_equal(bits(dev.point_cloud), bits(want))
    assert np.array_equal(bits(dev.point_cloud_features), bits(s["ft"])) and np.array_equal(bits(dev.point_invalid_mask), bits(s["mask"]))
    if n >= 63:
        assert (bits(want) != bits(s["pc"])).any()
    # the same call from the same state
    again = on_device(s)
    mcmc.inject_noise(again, NOISE["noise_scale"], NOISE["step"], seed=NOISE["seed"])
    assert np.array_equal(bits(again.point_cloud), bits(dev.point_cloud))


def test_noise_depends_on_the_row_alone_and_on_the_step():
    s = noise_scene(1500)
    whole = delta_from_zero(s, LARGE)
    part = delta_from_zero({k: v[:257] for k, v in s.items()}, LARGE)
    assert np.array_equal(bits(whole)[:257], bits(part))
    moved = (whole != 0).any(1)
    assert moved.sum() > 800
    other = delta_from_zero(s, LARGE, step=NOISE["step"] + 1)
    assert (bits(other)[moved] != bits(whole)[moved]).any(1).all()
    seeded = delta_from_zero(s, LARGE, seed=NOISE["seed"] + 1)
    assert (bits(seeded)[moved] != bits(whole)[moved]).any(1).all()
    # and with 1026 blocks behind the 257 rows
    s = noise_scene(MC.N_LARGE)
    whole = delta_from_zero(s, LARGE)
    part = delta_from_zero({k: v[:257] for k, v in s.items()}, LARGE)
    assert np.array_equal(bits(whole)[:257], bits(part))
    assert (whole[MC.N_FULL:] != 0).any() and (whole != 0).any(1).sum() > 150_000


# ---- regulariser -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, upstream", [(n, upstream) for n in SIZES for upstream in (None, 0.37)] + [(MC.N_LARGE, 0.37)])
def test_regulariser_against_float64(n, upstream):
    """MC.N_LARGE: 157 442 valid rows in 1026 blocks, so each thread of k_mcmc_reg_total sums two partials (0.6 s on the host)"""
    from taichi_3d_gaussian_splatting_amd import mcmc
    s = make_scene(n)
    assert n != MC.N_LARGE or (MC.per_thread(n) == 2 and (s["mask"] == 0).sum() == 157_442)
    lo, ls = 0.01, 0.02
    value, added = mcmc_ref.regulariser(s["ft"], s["mask"], lo, ls, 1.0 if upstream is None else upstream)
    dev = on_device(s)
    up = None if upstream is None else torch.tensor(upstream, device=DEV)
    zero = torch.zeros_like(dev.point_cloud_features)
    out = mcmc.add_regulariser_grad(dev, lo, ls, grad=zero, upstream=up).cpu().numpy().astype(np.float64)
    assert out[2] == value[2] == (s["mask"] == 0).sum()
    assert (np.abs(out[:2] - value[:2]) <= 1e-6 * np.abs(value[:2])).all()           # each term within 1e-6 of itself
    term = zero.cpu().numpy()                                       # 0 + term is the term
    valid = s["mask"] == 0
    ulps = mcmc_ref.ulp_distance_f32(term[valid][:, 4:8], added[valid][:, 4:8])
    print(f"regulariser n={n}: gradient within {ulps.max():.2f} f32 ulp (bar 4)")
    assert ulps.max() <= 4.0
    assert (bits(term[~valid]) == 0).all() and (bits(term[:, :4]) == 0).all() and (bits(term[:, 8:]) == 0).all()
    # += onto a gradient that is there: one f32 addition per element of the four columns, nothing else touched
    rng = np.random.default_rng(n)
    before = rng.normal(0.0, 1e-4, s["ft"].shape).astype(np.float32)
    grad = torch.tensor(before, device=DEV)
    again = mcmc.add_regulariser_grad(dev, lo, ls, grad=grad, upstream=up)
    assert np.array_equal(bits(again), bits(out.astype(np.float32)))
    want = before.copy()
    want[:, 4:8] = before[:, 4:8] + term[:, 4:8]
    assert np.array_equal(bits(grad), bits(want))
    assert np.array_equal(bits(dev.point_cloud_features), bits(s["ft"]))
    # the value alone
    alone = mcmc.add_regulariser_grad(dev, lo, ls, with_grad=False)
    assert np.array_equal(bits(alone), bits(again))


def test_regulariser_without_a_valid_row_and_through_the_parameter_grad():
    from taichi_3d_gaussian_splatting_amd import mcmc
    s = make_scene(257)
    dev = on_device(s, mask=np.where(s["mask"] == 0, 2, s["mask"]).astype(np.int8))
    before = np.random.default_rng(0).normal(0.0, 1.0, s["ft"].shape).astype(np.float32)
    grad = torch.tensor(before, device=DEV)
    out = mcmc.add_regulariser_grad(dev, 0.01, 0.02, grad=grad)
    assert (bits(out) == 0).all() and np.array_equal(bits(grad), bits(before))
    # the default target is the parameter's .grad, and there must be one
    dev = on_device(s)
    dev.point_cloud_features.requires_grad_(True)
    with pytest.raises(ValueError, match="no .grad"):
        mcmc.add_regulariser_grad(dev, 0.01, 0.02)
    dev.point_cloud_features.grad = torch.zeros_like(dev.point_cloud_features)
    mcmc.add_regulariser_grad(dev, 0.01, 0.02)
    assert float(dev.point_cloud_features.grad[:, 4:8].abs().sum()) > 0


# ---- relocate ----------------------------------------------------------------------------------------------------------
def run_relocate(s, moments=True, call_index=0, seed=3, ref=None, **settings):
    """-> (got: dict of numpy arrays after the call, ref: mcmc_ref.relocate's (or `ref`, the same computed before), moments before)"""
    from taichi_3d_gaussian_splatting_amd import mcmc
    dev = on_device(s)
    n = s["pc"].shape[0]
    rng = np.random.default_rng(7)
    mom = [rng.normal(0.0, 1.0, shape).astype(np.float32) + 3.0 for shape in ((n, 56), (n, 56), (n, 3), (n, 3))]
    optimizers = (None, None)
    if moments:
        t = [torch.tensor(m, device=DEV) for m in mom]
        optimizers = (SimpleNamespace(params=[dev.point_cloud_features], state=[dict(exp_avg=t[0], exp_avg_sq=t[1])]),
                      SimpleNamespace(params=[dev.point_cloud], state=[dict(exp_avg=t[2], exp_avg_sq=t[3])]))
    config = mcmc.MCMCConfig(seed=seed, **{k: v for k, v in settings.items() if k != "grow_permille"})
    if "grow_permille" in settings:
        config.grow_factor = 1.0 + settings["grow_permille"] / 1000.0
        assert config.grow_permille == settings["grow_permille"]
    plan = mcmc.MCMCPlan(n, DEV)
    for name in ("source_of", "dest_row", "multiplicity"):
        getattr(plan, name).fill_(-7)                               # what the call does not write stays
    counts = mcmc.relocate(dev, config, optimizers, call_index, plan)
    got = dict(counts=[int(x) for x in counts.cpu()], dest_row=plan.dest_row.cpu().numpy(), source_of=plan.source_of.cpu().numpy(),
               multiplicity=plan.multiplicity.cpu().numpy(), pc=dev.point_cloud.cpu().numpy(), ft=dev.point_cloud_features.cpu().numpy(),
               mask=dev.point_invalid_mask.cpu().numpy(), obj=dev.point_object_id.cpu().numpy(),
               moments=[x.cpu().numpy() for x in t] if moments else None)
    if ref is None:
        ref = mcmc_ref.relocate(s["pc"], s["ft"], s["mask"], s["obj"], seed, call_index, n_max=config.n_max, grow_permille=config.grow_permille,
                                cap_max=config.cap_max, min_logit=mcmc_ref.min_opacity_logit(config.min_opacity))
    return got, ref, mom


def check_relocate(s, got, ref, mom):
    n = s["pc"].shape[0]
    D = ref["counts"][5]
    assert got["counts"] == ref["counts"], (dict(zip(mcmc_ref.COUNTS, got["counts"])), dict(zip(mcmc_ref.COUNTS, ref["counts"])))
    assert got["dest_row"][:D].tolist() == ref["dest_row"] and got["source_of"][:D].tolist() == ref["source_of"]
    assert (got["dest_row"][D:] == -7).all() and (got["source_of"][D:] == -7).all()
    if D:
        assert np.array_equal(got["multiplicity"], ref["multiplicity"])
    else:
        assert (got["multiplicity"] == -7).all()
    touched = ref["touched"]
    assert touched.sum() == D + ref["counts"][6]
    assert np.array_equal(got["mask"], ref["mask"]) and np.array_equal(got["obj"], ref["object_id"])
    assert np.array_equal(bits(got["pc"]), bits(ref["point_cloud"]))
    keep = [0, 1, 2, 3] + list(range(8, 56))
    assert np.array_equal(bits(got["ft"][:, keep]), bits(ref["features64"][:, keep].astype(np.float32)))
    assert np.array_equal(bits(got["ft"][~touched]), bits(s["ft"][~touched]))
    if touched.any():
        ulps = mcmc_ref.ulp_distance_f32(got["ft"][touched][:, 4:8], ref["features64"][touched][:, 4:8])
        print(f"relocate n={n}: D={D}, sources={ref['counts'][6]}, largest multiplicity={ref['multiplicity'].max()}, "
              f"new logit and log-scales within {ulps.max():.2f} f32 ulp (bar 2)")
        assert ulps.max() <= 2.0
        dest, source = np.array(ref["dest_row"], np.int64), np.array(ref["source_of"], np.int64)
        assert np.array_equal(bits(got["ft"][dest, 4:8]), bits(got["ft"][source, 4:8]))                    # the same bits within a group
    if got["moments"] is not None:
        for after, before in zip(got["moments"], mom):
            assert (bits(after[touched]) == 0).all() and np.array_equal(bits(after[~touched]), bits(before[~touched]))


@pytest.mark.parametrize("n", SIZES)
def test_relocate_against_the_reference(n):
    s = make_scene(n, seed=1)
    got, ref, mom = run_relocate(s)
    check_relocate(s, got, ref, mom)
    if n >= 63:
        assert ref["counts"][1] > 0 and ref["counts"][4] > 0 and ref["counts"][5] == ref["counts"][1] + ref["counts"][4]
        assert ref["counts"][4] == min(ref["counts"][3], ref["counts"][0] * 50 // 1000)


def test_relocate_with_nothing_to_do_keeps_every_bit():
    s = make_scene(300, seed=2)
    full = dict(s, mask=np.where(s["mask"] == 1, 2, s["mask"]).astype(np.int8), ft=s["ft"].copy())
    full["ft"][:, 7] = np.abs(full["ft"][:, 7])                    # no dead row, no free row
    got, ref, mom = run_relocate(full)
    assert ref["counts"][1] == ref["counts"][3] == ref["counts"][5] == 0 and ref["counts"][0] == ref["counts"][7] > 0
    check_relocate(full, got, ref, mom)
    assert np.array_equal(bits(got["ft"]), bits(full["ft"])) and np.array_equal(bits(got["pc"]), bits(full["pc"]))
    # every valid row dead: nothing to copy from, D = 0 although there are dead and free rows
    gone = dict(s, ft=s["ft"].copy())
    gone["ft"][:, 7] = -8.0
    gone["ft"][3, 7] = np.nan
    got, ref, mom = run_relocate(gone)
    assert ref["counts"][2] == 0 and ref["counts"][1] == ref["counts"][0] > 0 and ref["counts"][3] > 0 and ref["counts"][4:7] == [0, 0, 0]
    check_relocate(gone, got, ref, mom)
    assert np.array_equal(bits(got["ft"]), bits(gone["ft"])) and np.array_equal(got["mask"], gone["mask"])


def test_relocate_budget_clipped_by_the_cap_and_by_the_free_rows():
    s = make_scene(700, seed=3)
    valid = int((s["mask"] == 0).sum())
    got, ref, mom = run_relocate(s, cap_max=valid - 5)              # a cap below the valid rows: relocation only
    assert ref["counts"][4] == 0 and ref["counts"][5] == ref["counts"][1] > 0 and ref["counts"][7] == valid
    check_relocate(s, got, ref, mom)
    got, ref, mom = run_relocate(s, cap_max=valid + 3)              # the cap cuts the growth
    assert ref["counts"][4] == 3 and ref["counts"][7] == valid + 3
    check_relocate(s, got, ref, mom)
    free = int((s["mask"] == 1).sum())
    got, ref, mom = run_relocate(s, grow_permille=900)              # more wanted than there are free rows
    assert valid * 900 // 1000 > free and ref["counts"][4] == free and ref["counts"][7] == valid + free
    check_relocate(s, got, ref, mom)
    assert (got["mask"] != 1).all()


def test_relocate_one_alive_row_among_many_dead_clamps_the_group_size():
    s = make_scene(300, seed=4)
    ft = s["ft"].copy()
    ft[:, 7] = -7.0
    ft[130, 7] = 2.0
    lone = dict(s, ft=ft)
    assert lone["mask"][130] == 0
    for n_max in (51, 5):
        got, ref, mom = run_relocate(lone, n_max=n_max)
        assert ref["counts"][2] == 1 and ref["counts"][6] == 1 and ref["multiplicity"][130] == ref["counts"][5] > 60
        assert set(ref["source_of"]) == {130}
        check_relocate(lone, got, ref, mom)
        assert (got["mask"][lone["mask"] == 0] == 0).all() and got["ft"][130, 7] < 2.0


def test_relocate_with_a_block_of_saturated_rows_and_across_block_boundaries():
    """256 rows of sigmoid = 1.0f: the block's weights sum to 256 (2^24 - 1) > 2^31, and every later prefix carries it"""
    s = make_scene(1500, seed=5, dead_share=0.3)
    ft, mask = s["ft"].copy(), s["mask"].copy()
    ft[256:512, 7], mask[256:512] = 30.0, 0
    sat = dict(s, ft=ft, mask=mask)
    got, ref, mom = run_relocate(sat, grow_permille=200)
    assert ref["W"] > 2 ** 32 and sum(ref["weights"][256:512]) == 256 * (2 ** 24 - 1) > 2 ** 31
    in_block = sum(1 for r in ref["source_of"] if 256 <= r < 512)
    assert in_block > 0 and any(r >= 512 for r in ref["source_of"]) and any(r < 256 for r in ref["source_of"])
    check_relocate(sat, got, ref, mom)
    # two alive rows, the last of one block and the first of the next; everything else dead or free
    ft = s["ft"].copy()
    ft[:, 7] = -7.0
    ft[255, 7], ft[256, 7] = 0.5, -0.5
    pair = dict(s, ft=ft, mask=np.where(np.isin(np.arange(1500), (255, 256)), 0, s["mask"]).astype(np.int8))
    got, ref, mom = run_relocate(pair)
    assert set(ref["source_of"]) == {255, 256}
    check_relocate(pair, got, ref, mom)


def test_relocate_without_moments_and_with_another_call_index():
    s = make_scene(700, seed=6)
    got, ref, mom = run_relocate(s, moments=False)
    check_relocate(s, got, ref, mom)
    first, ref_first, mom = run_relocate(s, call_index=0)
    again, _, _ = run_relocate(s, call_index=0)
    other, ref_other, _ = run_relocate(s, call_index=1)
    check_relocate(s, other, ref_other, mom)
    for name in ("source_of", "ft", "pc", "mask"):
        assert np.array_equal(bits(first[name]), bits(again[name])), name
    assert first["counts"][:6] == other["counts"][:6] and not np.array_equal(first["source_of"], other["source_of"])
    assert not np.array_equal(bits(first["ft"]), bits(other["ft"]))
    seeded, _, _ = run_relocate(s, seed=4)
    assert not np.array_equal(first["source_of"], seeded["source_of"])


# ---- relocate past 1024 blocks, and where a draw lands on a prefix (tests/mcmc_cases.py) ------------------------------------------
def relocate_case(name, **override):
    s = MC.scene(name)
    settings = dict(s["settings"], **override)
    call_index = settings.pop("call_index", 0)
    got, ref, mom = run_relocate(s, call_index=call_index, seed=MC.SEED, ref=MC.reference(name, **override), **settings)
    print(name, override, dict(zip(mcmc_ref.COUNTS, got["counts"])))
    check_relocate(s, got, ref, mom)
    return s, got, ref


@pytest.mark.parametrize("name", MC.LARGE_SPARSE)
def test_relocate_with_two_blocks_per_scan_thread(name):
    """More than 1024 blocks of 256 rows: k_mcmc_scan's threads own two blocks each, write three exclusive prefixes back over two
    entries, and the threads behind the last block own none.  Nearly every row has mask 2, so the reference stays fast (0.6 s on
    the host per case, and 0.5 s for the four moment tensors).  Counts on the device, as the reference's
    (valid / dead / alive / free / new / D / sources):
      past_1024_blocks        262 403 rows, 1026 blocks   712 / 241 / 471 / 228 / 142 / 383 / 231, 66 destinations and 66 draws in blocks 1024 and 1025
      blocks_1024             262 144 rows, 1024 blocks   440 / 139 / 301 / 166 / 88 / 227 / 136   (one block per thread: the last such size)
      blocks_1025_last_alive  262 145 rows, 1025 blocks   440 / 140 / 300 / 166 / 88 / 228 / 139   (block 1024 is one alive row, and it is drawn)
      blocks_1025_last_dead   262 145 rows, 1025 blocks   440 / 141 / 299 / 166 / 88 / 229 / 144   (block 1024 is one dead row, the last dead destination)"""
    s, got, ref = relocate_case(name)
    n = s["pc"].shape[0]
    assert (MC.per_thread(n) == 2) == (n > MC.N_FULL)
    if name == "past_1024_blocks":
        assert (got["source_of"][:ref["counts"][5]] >= MC.N_FULL).any() and (got["dest_row"][:ref["counts"][5]] >= MC.N_FULL).any()
        # the partial block: its dead row was filled, its free row is behind the n_new that were brought in
        assert got["mask"][-3:].tolist() == [0, 1, 0] and (got["mask"] == 1).sum() == ref["counts"][3] - ref["counts"][4] > 0


@pytest.mark.parametrize("n_max", [51, 5])
def test_relocate_with_more_destinations_than_one_turn_of_the_grid_holds(n_max):
    """262 443 rows: 262 403 valid, all dead but five (rows 7, 255, 256, 131 072 and 262 402), and 40 free rows behind them.
    D = 262 398 + 40 = 262 438 > 1024 x 256, so the 1024 blocks of k_mcmc_sample and k_mcmc_apply_dest take a second turn, over 254
    dead rows and the 40 free ones.  The five sources are drawn 74 264, 52 534, 31 636, 61 809 and 42 195 times: M = n_max.
    Counts on the device: 262 403 / 262 398 / 5 / 40 / 40 / 262 438 / 5.  On the host the reference takes 1.3 s (it is linear in
    sources x D, so the sources are few), the four moment tensors 0.6 s."""
    s, got, ref = relocate_case("second_turn", n_max=n_max)
    assert got["counts"][5] > MC.N_FULL and (got["mask"] == 0).all()
    late = got["dest_row"][MC.N_FULL:got["counts"][5]]
    assert len(late) == 294 and (s["mask"][late] == 1).sum() == 40
    assert len(np.unique(bits(got["ft"][:, 4:8]), axis=0)) == 5                 # five groups, one set of bits each


def test_relocate_where_every_draw_lands_on_a_prefix():
    """Scene C of tests/mcmc_cases.py: 1500 rows at min_opacity 1e-9 with opacities of 2^-24 and below.  Every weight is 1 or 2
    (393 of the 523 alive rows by the clamp max(w, 1)), W = 572, and of the D = 557 draws 501 have t == C(source): the searches'
    `<=` decides them.  Rows 512..767 hold no weight; one draw has t = 232, the prefix that this block shares with the next, and
    its source is row 771, the first alive row behind the empty block.  Draws also pick the last alive row of blocks 3 and 4 and the
    first of blocks 4 and 5.  Every p is clamped up to 0.005 (o / M is 1e-8 at most), so each group ends at logit(0.005) and its
    log-scales move by log(o / d), about -15.
    Counts on the device: 900 valid / 377 dead / 523 alive / 450 free / 180 new / D 557 / 337 sources.

    What this catches, tried once each on an MI355X in a build of k_mcmc_sample that was not kept:
      `ws.wpre[mid] < t` for `<=` (block search): the other 48 tests of this file pass, the cases past 1024 blocks among them;
          this one fails on source_of, first at destination 183: row 511, the last row of the block before the empty one, for 771
      `ws.excl[first + mid] < local` for `<=` (row search): the other 48 tests pass; this one fails on the counts, 340 sources
          for 337 (a draw on a row's own prefix goes to the row before it, alive or not)
    The suite as it was before this test passes on both."""
    f = MC.unit_facts()
    s, got, ref = relocate_case("unit_weights")
    D = got["counts"][5]
    assert f["W"] < 1000 and 2 * f["draws_on_a_prefix"] >= D
    first = f["first_alive_after_the_empty_block"]
    assert first in f["draws_on_the_shared_prefix"] and got["multiplicity"][first] >= 1
    assert (got["multiplicity"][MC.UNIT_EMPTY_BLOCK * MC.BLOCK:(MC.UNIT_EMPTY_BLOCK + 1) * MC.BLOCK] == 0).all()


def test_relocate_of_an_empty_scene():
    from taichi_3d_gaussian_splatting_amd import mcmc
    dev = SimpleNamespace(point_cloud=torch.zeros((0, 3), device=DEV), point_cloud_features=torch.zeros((0, 56), device=DEV),
                          point_invalid_mask=torch.zeros(0, dtype=torch.int8, device=DEV), point_object_id=torch.zeros(0, dtype=torch.int32, device=DEV))
    plan = mcmc.MCMCPlan(0, DEV)
    plan.counts.fill_(9)
    assert mcmc.relocate(dev, plan=plan).cpu().tolist() == [0] * 8
    mcmc.inject_noise(dev, 1.0, 0)
    assert mcmc.add_regulariser_grad(dev, 0.01, 0.01, with_grad=False).cpu().tolist() == [0.0, 0.0, 0.0]
