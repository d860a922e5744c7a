"""The chained rollout kernels from mid-game boards and across the RNG-table chunk boundaries.

From fresh boards the built-in random policy dies after about 17 pieces and never clears two rows at once, so the other tests of
k_chain<1>, k_chain_affine<1>, k_chain_fused<1>, k_chain_fused_affine<1> and the chained k_duo forms only ever show them almost
empty boards early in an episode.  Here the batches are SEEDED (tests/seeded.py): a pool of 96 games is played by the heuristic model of
tests/policy_model.py on the oracle (24 steps for one player, 40 for two, 64 for three), the recorded (rot, trans, player) are replayed on
a pool batch of the engine under test through step_rt, and both pools are tiled into the batches (copy_from / snapshot + restore).
The tiled games share boards and piece sequences but not policy draws (keyed by game id), so they diverge at once.  From such
boards the random rollout clears several rows at a time, builds combos, queues garbage more than one packet deep, blocks lines and
draws holes: the G_LINES / G_SENT atomics, the combo timers, the conditionally loaded and stored W_FIFO_* rows.  A second
preparation (O pieces laid side by side, tests/test_engine_vs_oracle.py) brings every game just below draw 624, 748 (the
low-water mark of a two-chunk table) or 1248, so that a chained call itself crosses the boundary and raises the request to extend.

Every comparison is exact equality against the oracle, after every call.  The oracle is stepped ONE step per rollout_random call
and observed after each (Census), so that no test passes because nothing rare happened on the very trajectory it compares."""
import numpy as np
import pytest

from tests import engines
from tests.seeded import N_CPU, N_GPU, Census, _assert_path, _call, _interleaved_step, _model_pool, _o_pool, _seeded, _set_path

CHUNK, LOW_WATER = 624, 500   # draws per RNG-table chunk; margin of tetris_rollout_launch (one step per launch)


# ---------------------------------------------------------------- 1. CPU harness
@pytest.mark.parametrize("P,H", [(1, 20), (2, 20), (3, 20), (1, 22)])
def test_cpu_single_steps_equal_fused_steps_from_midgame_boards(P, H):
    """CPU harness, 333 seeded games: K launches of one step, one launch of K steps and the oracle leave the same boards and
    counters, twice (the second time from a first_step other than 0), with a launch of no steps in between."""
    n, K = N_CPU, 60
    prepared = _model_pool(P, H)
    single, ref = _seeded("harness", n, P, H, prepared)
    fused, _ = _seeded("harness", n, P, H, prepared)
    cen = Census(ref)
    for rep in range(2):
        before = cen.total.copy()
        cK, _ = fused.rollout_random(1, K, first_step=cen.step)
        _call(single, cen, K, 1, f"K launches of one step, round {rep}")
        assert cK.tolist() == (cen.total - before).tolist()
        engines.assert_same_state(fused, ref, where=f"one launch of K steps, round {rep}")
        for e in (single, fused):
            c0, _ = e.rollout_random(2, 0, first_step=cen.step)
            assert c0.tolist() == [0, 0, 0, 0]
            engines.assert_same_state(e, ref, where=f"launches of no steps, round {rep}")
    cen.assert_rare_events(P)


# ---------------------------------------------------------------- 2. GPU
# (launches, steps per launch): S = 1, S = 3 and S = 0 take turns, 152 env-steps in all
TURNS = [(20, 1), (6, 3), (17, 0), (33, 1), (5, 3), (1, 1), (40, 1), (7, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("path,H", [("streams", 20), ("queues_write_through", 20), ("queues_affine", 20), ("unchained", 20),
                                    ("queues_affine", 22)])
def test_gpu_one_player_chained_calls_from_midgame_boards(path, H):
    """1 100 seeded one-player boards; chained calls of S = 1, S = 3 and S = 0 take turns (all four k_chain* kernels), one step_rt
    with resets between them; counters, full state, error bits and the launch path checked after EVERY call.  `unchained` is the
    control."""
    n = N_GPU
    eng, ref = _seeded("hip", n, 1, H, _model_pool(1, H))
    _set_path(eng, path)
    cen, rng = Census(ref), np.random.default_rng(41)
    for k, (launches, S) in enumerate(TURNS):
        if path == "streams":
            launches = min(launches, 15)
        _call(eng, cen, launches, S, f"{path}, call {k} ({launches} x {S})")
        _assert_path(eng, path)
        _interleaved_step(eng, ref, rng, k)
    for S in (0, 1, 3):
        assert eng.rollout_is_chained(S) == (path != "unchained")          # no wave gave up, nothing fell back
    cen.assert_rare_events(1)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["streams", "queues", "queues_affine", "unchained"])
def test_gpu_two_player_chained_calls_from_midgame_boards(path):
    """1 100 seeded two-player games (35 k_duo waves; 40 XCD-affine), one step per launch (fused calls of two players do not
    chain): garbage queues several packets deep, blocked lines, hole draws."""
    n = N_GPU
    eng, ref = _seeded("hip", n, 2, 20, _model_pool(2, 20))
    _set_path(eng, path)
    cen, rng = Census(ref), np.random.default_rng(42)
    for k, launches in enumerate((20, 33, 1, 40, 7, 50)):
        _call(eng, cen, launches, 1, f"{path}, call {k} ({launches} x 1)")
        _assert_path(eng, path)
        _interleaved_step(eng, ref, rng, k)
    assert eng.rollout_is_chained(1) == (path != "unchained")
    cen.assert_rare_events(2)


# ---------------------------------------------------------------- 3. RNG-table boundaries
BOUNDARIES = [CHUNK, 2 * CHUNK - LOW_WATER, 2 * CHUNK, "low_water"]
PATHS = [pytest.param("harness", None, id="harness"), pytest.param("hip", "streams", marks=pytest.mark.gpu, id="streams"),
         pytest.param("hip", "queues_affine", marks=pytest.mark.gpu, id="queues_affine")]


@pytest.mark.parametrize("kind,path", PATHS)
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_chained_calls_cross_the_rng_table_boundaries(kind, path, boundary):
    """Games prepared to just below draw 624, 748 or 1248 (8 O-only games tiled to 1 100), then 40 chained launches of one step and
    4 of three: the calls themselves cross the boundary.  Exact after each call, no TETRIS_ERR_STREAM.  At 748 the kernel of a
    chained call on the GPU raises the request to extend a two-chunk table: if the process's tables (shared by all its batches)
    still have two chunks before the calls they have at least three after; if another test has grown them already only exactness is
    checked.  (The CPU harness looks at the flag words after every launch and keeps a margin of 64 draws, not 500: there the
    case at 748 is one more exactness check.)
    `low_water` is the same case made independent of what ran before: the boundary is the low-water mark of the tables as this
    process has them NOW, so the chained calls always raise the request themselves and the tables always have to grow."""
    n = N_GPU
    grows = boundary == "low_water"
    if grows:
        probe = engines.make(kind, 8, 1, pieces=(6,))
        boundary = probe.table_chunks * CHUNK - (LOW_WATER if kind == "hip" else 64)
        probe.close()
    eng, ref = _seeded(kind, n, 1, 20, _o_pool(boundary), pieces=(6,))
    if path:
        _set_path(eng, path)
    cen = Census(ref)
    assert cen.first_draws < boundary
    chunks = eng.table_chunks
    if grows:
        assert boundary + (LOW_WATER if kind == "hip" else 64) == chunks * CHUNK, "the preparation itself made the tables grow"
    for k, (launches, S) in enumerate(((40, 1), (4, 3))):
        _call(eng, cen, launches, S, f"boundary {boundary}, call {k}")
        if path:
            _assert_path(eng, path)
    print(f"boundary {boundary}: piece_draws.max() {cen.first_draws} -> {cen.seen['draws']}, table_chunks {chunks} -> {eng.table_chunks}")
    assert cen.seen["draws"] >= boundary + 10, "the oracle's games did not pass the boundary"
    if grows or (kind == "hip" and boundary == 2 * CHUNK - LOW_WATER and chunks == 2):
        assert eng.table_chunks > chunks
    if boundary == 2 * CHUNK:
        assert eng.table_chunks >= 3
    if path:
        assert eng.rollout_is_chained(1) and eng.rollout_is_chained(3)
