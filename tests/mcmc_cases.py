"""The scenes of tests/test_gpu_mcmc.py and tests/test_gpu_mcmc_loop.py that exist for one path of csrc/k_mcmc.hip each, and the
facts about them that make them take it.  numpy and tests/mcmc_ref.py only: tests/test_mcmc_ref_host.py asserts the facts without
a GPU, the GPU tests run the library on the same arrays.  Scenes and references are cached and never edited.

Sizes.  A block is 256 rows; k_mcmc_scan and k_mcmc_reg_total give each of 1024 threads per = ceil(nb / 1024) block sums, and
k_mcmc_sample / k_mcmc_apply_dest launch min(nb, 1024) blocks that stride over the D destinations.
  N_FULL  = 1024 * 256      nb = 1024, per = 1: the last size at which every thread owns one block
  N_FULL + 1                nb = 1025, per = 2: thread 512 owns block 1024 (one row) alone, threads 513.. own nothing
  N_LARGE = 1025 * 256 + 3  nb = 1026, per = 2: thread 512 owns block 1024 and the partial block 1025 (three rows)
"""
import numpy as np

import mcmc_ref

BLOCK = mcmc_ref.BLOCK
SCAN_THREADS = 1024
N_FULL = SCAN_THREADS * BLOCK
N_LARGE = 1025 * BLOCK + 3
MASK_PATTERN = (0, 0, 1, 0, 2, 0, 1, 0, 0, 1)
SEED = 3                                        # run_relocate's
UNIT_MIN_OPACITY = 1e-9
DEAD_LOGIT = -7.0

_scenes, _refs = {}, {}


def blocks(n):
    return (n + BLOCK - 1) // BLOCK


def per_thread(n):
    """block sums per thread of the one-block kernels"""
    return (blocks(n) + SCAN_THREADS - 1) // SCAN_THREADS


def _rows(rng, n):
    """n rows of make_scene's kind, every logit alive"""
    ft = rng.standard_normal((n, 56), dtype=np.float32) * np.float32(0.6)
    ft[:, 4:7] = rng.standard_normal((n, 3), dtype=np.float32) * np.float32(0.5) - np.float32(3.0)
    ft[:, 7] = rng.uniform(-4.0, 4.0, n).astype(np.float32)
    return dict(pc=rng.standard_normal((n, 3), dtype=np.float32), ft=ft, mask=np.full(n, 2, np.int8),
                obj=rng.integers(0, 5, n).astype(np.int32))


def _mix(rng, s, rows):
    """the rows become alive, dead or free, about 50 : 24 : 26"""
    kind = rng.choice(3, len(rows), p=(0.5, 0.24, 0.26))
    s["mask"][rows] = np.where(kind == 2, 1, 0)
    s["ft"][rows[kind == 1], 7] = DEAD_LOGIT


def _sparse(n, seed, around=()):
    """n rows, nearly all mask 2: 600 random rows and the rows within five of each row of `around` are a mix"""
    rng = np.random.default_rng(seed)
    s = _rows(rng, n)
    chosen = [rng.choice(n, 600, replace=False)] + [np.arange(max(0, r - 5), min(n, r + 5)) for r in around]
    _mix(rng, s, np.unique(np.concatenate(chosen)))
    return rng, s


def scene(name):
    """-> dict of numpy arrays pc, ft, mask, obj, and `settings`: what run_relocate is given beyond the scene"""
    if name not in _scenes:
        _scenes[name] = _BUILDERS[name]()
    return _scenes[name]


def _past_1024_blocks():
    """Scene A.  600 random rows, blocks 300 and 301 (both of scan thread 150), the rows around the 1023 / 1024 block boundary and
    the last 300 rows are a mix; the last three rows -- the partial block -- are dead, free, alive."""
    n = N_LARGE
    rng, s = _sparse(n, 41, around=(1024 * BLOCK,))
    _mix(rng, s, np.concatenate([np.arange(300 * BLOCK + 40, 300 * BLOCK + 60), np.arange(301 * BLOCK + 10, 301 * BLOCK + 30),
                                 np.arange(n - 300, n - 3)]))
    s["mask"][n - 3:] = (0, 1, 0)
    s["ft"][n - 3, 7], s["ft"][n - 1, 7] = DEAD_LOGIT, 1.5
    return dict(s, settings=dict(grow_permille=200))


SECOND_TURN_ALIVE = ((7, 2.0), (255, 0.5), (256, -0.5), (131072, 1.0), (N_LARGE - 1, 0.0))
SECOND_TURN_FREE = 40


def _second_turn():
    """Scene B.  N_LARGE valid rows, all dead but five, and 40 free rows behind them that the default growth brings in: the
    destinations past 1024 * 256 are dead rows and then free rows."""
    n = N_LARGE + SECOND_TURN_FREE
    s = _rows(np.random.default_rng(42), n)
    s["mask"][:N_LARGE], s["mask"][N_LARGE:] = 0, 1
    s["ft"][:, 7] = DEAD_LOGIT
    for row, logit in SECOND_TURN_ALIVE:
        s["ft"][row, 7] = logit
    return dict(s, settings=dict())


UNIT_EMPTY_BLOCK = 2                            # rows 512..767 hold no weight
UNIT_CALL_INDEX = 1                             # frozen: the first call index at which every condition of unit_facts() holds


def _unit_weights():
    """Scene C.  Opacities of 2^-24 and below: every alive weight is 1 or 2, W is a few hundred, and a draw lands on a prefix
    boundary more often than not."""
    n = 1500
    rng = np.random.default_rng(43)
    s = _rows(rng, n)
    s["mask"] = np.array([MASK_PATTERN[i % 10] for i in range(n)], np.int8)
    s["ft"][:, 7] = rng.uniform(-20.0, -15.55, n).astype(np.float32)     # (above -15.54 the weight would be 3)
    s["ft"][rng.random(n) < 0.3, 7] = -25.0
    s["ft"][UNIT_EMPTY_BLOCK * BLOCK:(UNIT_EMPTY_BLOCK + 1) * BLOCK, 7] = -25.0
    return dict(s, settings=dict(grow_permille=200, min_opacity=UNIT_MIN_OPACITY, call_index=UNIT_CALL_INDEX))


def _boundary(n, last_logit=None):
    def build():
        rng, s = _sparse(n, 44, around=(n - 1,))
        if last_logit is not None:
            s["mask"][n - 1], s["ft"][n - 1, 7] = 0, last_logit
        return dict(s, settings=dict(grow_permille=200))
    return build


_BUILDERS = {"past_1024_blocks": _past_1024_blocks, "second_turn": _second_turn, "unit_weights": _unit_weights,
             "blocks_1024": _boundary(N_FULL), "blocks_1025_last_alive": _boundary(N_FULL + 1, 1.0),
             "blocks_1025_last_dead": _boundary(N_FULL + 1, DEAD_LOGIT)}
LARGE_SPARSE = ("past_1024_blocks", "blocks_1024", "blocks_1025_last_alive", "blocks_1025_last_dead")


def reference(name, **override):
    """mcmc_ref.relocate of the scene under its settings (and `override`), once"""
    key = (name, tuple(sorted(override.items())))
    if key not in _refs:
        s = scene(name)
        settings = dict(s["settings"], **override)
        min_logit = mcmc_ref.min_opacity_logit(settings.get("min_opacity", 0.005))
        _refs[key] = mcmc_ref.relocate(s["pc"], s["ft"], s["mask"], s["obj"], SEED, settings.get("call_index", 0), min_logit=min_logit,
                                       n_max=settings.get("n_max", mcmc_ref.N_MAX), grow_permille=settings.get("grow_permille", 50))
    return _refs[key]


def counts(ref):
    return dict(zip(mcmc_ref.COUNTS, ref["counts"]))


def block_facts(name):
    """per block of the scene: weight, dead, free and alive rows, from the reference's classes"""
    s, ref = scene(name), reference(name)
    n = s["pc"].shape[0]
    nb = blocks(n)
    w = np.array(ref["weights"], np.int64)
    pad = nb * BLOCK - n
    valid, free = np.asarray(s["mask"]) == 0, np.asarray(s["mask"]) == 1
    per_block = lambda x: np.concatenate([x.astype(np.int64), np.zeros(pad, np.int64)]).reshape(nb, BLOCK).sum(1)
    return dict(weight=per_block(w), dead=per_block(valid & (w == 0)), free=per_block(free), alive=per_block(w > 0))


def second_turn_rows(name, **override):
    """the destination rows that the second turn of k_mcmc_sample's and k_mcmc_apply_dest's loops handles"""
    return np.array(reference(name, **override)["dest_row"][N_FULL:], np.int64)


def unit_facts():
    """What scene C exists for, from the reference's integers: -> dict"""
    s, ref = scene("unit_weights"), reference("unit_weights")
    w = ref["weights"]
    n = len(w)
    D = ref["counts"][5]
    source_of, ts, W = mcmc_ref.draw_sources(w, D, SEED, s["settings"]["call_index"])
    assert source_of == ref["source_of"] and W == ref["W"]
    C = np.concatenate([[0], np.cumsum(w)])[:n]                    # exclusive prefix by row
    alive = np.nonzero(np.array(w) > 0)[0]
    scaled = np.floor(mcmc_ref.sigmoid_f32(s["ft"][:, 7]).astype(np.float64) * mcmc_ref.WEIGHT_ONE)
    first_after = UNIT_EMPTY_BLOCK + 1
    shared = int(C[first_after * BLOCK])                            # the prefix of the empty block and of the one after it
    assert shared == int(C[UNIT_EMPTY_BLOCK * BLOCK])
    last_of, first_of = {}, {}
    for r in alive:
        first_of.setdefault(r // BLOCK, int(r))
        last_of[r // BLOCK] = int(r)
    drawn = set(source_of)
    seams = [b for b in last_of if b + 1 in first_of and last_of[b] in drawn and first_of[b + 1] in drawn]
    clamped = []
    for r in sorted(drawn):
        m = int(ref["multiplicity"][r])
        M = min(m + 1, mcmc_ref.N_MAX)
        o = float(mcmc_ref.sigmoid_f32(s["ft"][r, 7]))
        unclamped = 1.0 - np.power(1.0 - o, 1.0 / M)
        _, _, (_, p, _) = mcmc_ref.relocated(s["ft"][r, 7], s["ft"][r, 4:7], m, mcmc_ref.N_MAX)
        if unclamped < mcmc_ref.P_MIN and p == mcmc_ref.P_MIN:
            clamped.append(r)
    return dict(weights=sorted(set(w[r] for r in alive)), raised_to_one=int((scaled[alive] == 0).sum()), W=W, D=D,
                draws_on_a_prefix=sum(1 for t, r in zip(ts, source_of) if t == C[r]),
                draws_on_the_shared_prefix=[r for t, r in zip(ts, source_of) if t == shared],
                first_alive_after_the_empty_block=first_of[first_after], empty_block_weight=sum(w[UNIT_EMPTY_BLOCK * BLOCK:first_after * BLOCK]),
                weight_before_the_empty_block=shared, seams_drawn_on_both_sides=[int(b) for b in seams], sources_clamped_up=len(clamped), sources=len(drawn),
                largest_multiplicity=int(ref["multiplicity"].max()))


# ---- the trainer's initial scene (tests/test_gpu_mcmc_loop.py) ---------------------------------------------------------------
LOOP_PLANTED = 40
LOOP = dict(noise_lr=5e5, position_learning_rate=1e-4, seed=3)


def loop_initial(point_cloud, features):
    """-> (point_cloud, features) with the logits of 40 rows, every tenth, spread over [-6, -2.5]: both sides of logit(0.005) =
    -5.29, so some are dead at the first refinement, and all of them so transparent that the noise gate is open"""
    ft = np.array(features, np.float32)
    rows = np.arange(LOOP_PLANTED) * 10 + 3
    ft[rows, 7] = np.linspace(-6.0, -2.5, LOOP_PLANTED).astype(np.float32)
    return np.array(point_cloud, np.float32), ft, rows


def rows_moved_by_more_than_an_ulp(point_cloud, features, mask, noise_scale, seed, step):
    """the rows on which mcmc_ref.noise's delta exceeds one f32 ulp of the position, in some component"""
    delta, _, moves = mcmc_ref.noise(features, mask, noise_scale, seed, step)
    ulp = np.spacing(np.abs(np.asarray(point_cloud, np.float32))).astype(np.float64)
    return np.nonzero(moves & (np.abs(delta) > ulp).any(1))[0]
