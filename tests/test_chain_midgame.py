"""The chained rollout kernels from mid-game boards and across the RNG-table chunk boundaries.

From fresh boards the built-in random policy dies after about 17 pieces and never clears two rows at once, so the other tests of
k_chain<1>, k_chain_affine<1>, k_chain_fused<1>, k_chain_fused_affine<1> and the chained k_duo forms only ever show them almost
empty boards early in an episode.  Here the batches are SEEDED: a pool of 96 games is played by the heuristic model of
tests/test_policy_device.py on the oracle (24 steps for one player, 40 for two, 64 for three), the recorded (rot, trans, player) are replayed on
a pool batch of the engine under test through step_rt, and both pools are tiled into the batches (copy_from / snapshot + restore).
The tiled games share boards and piece sequences but not policy draws (keyed by game id), so they diverge at once.  From such
boards the random rollout clears several rows at a time, builds combos, queues garbage more than one packet deep, blocks lines and
draws holes: the G_LINES / G_SENT atomics, the combo timers, the conditionally loaded and stored W_FIFO_* rows.  A second
preparation (O pieces laid side by side, tests/test_engine_vs_oracle.py) brings every game just below draw 624, 748 (the
low-water mark of a two-chunk table) or 1248, so that a chained call itself crosses the boundary and raises the request to extend.

Every comparison is exact equality against the oracle, after every call.  The oracle is stepped ONE step per rollout_random call
and observed after each (Census), so that no test passes because nothing rare happened on the very trajectory it compares."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import engines
from tests.test_policy_device import W_A, Model

POOL = 96
N_CPU, N_GPU = 333, 1100      # 1100: 18 waves of 64 (the last of 12 games; 24 workgroups XCD-affine), 35 k_duo waves (40)
# Steps of the preparation by players.  Three players: 64, not 40 — with 40 the oracle's census at 333 games sees no combo of three
# after a rollout step (a player moves every 1 200 ms against a combo timer that starts at 1 800).  64 is no multiple of three, so
# the rollout's rotation meets players that moved 400 or 800 ms ago with their combos alive: 7 board-steps with a combo of three.
PREP = {1: 24, 2: 40, 3: 64}
CHUNK, LOW_WATER = 624, 500   # draws per RNG-table chunk; margin of tetris_rollout_launch (one step per launch)


def _pool_seeds(pool):
    return orc.episode_seed(np.arange(pool), 0)


# ---------------------------------------------------------------- 1. seeding
@functools.lru_cache(maxsize=None)
def _model_pool(P, H, ms=400, prep=None, pool_size=POOL, survivors=0.75):
    """-> the oracle pool after the model's play (`prep` steps of `ms` milliseconds; PREP[P] if None), the actions
    [(rot, trans, player, done)], the pool games that did not end"""
    pool = engines.make("oracle", pool_size, P, height=H, seeds=_pool_seeds(pool_size))
    m = Model(pool)
    ended, actions = np.zeros(pool_size, bool), []
    for s in range(PREP[P] if prep is None else prep):                        # (no auto-reset)
        r, t, _ = m.choose(W_A, s % P)
        done = pool.step_rt(r, t, s % P, ms=ms)
        ended |= done > 0
        actions.append((r.copy(), t.copy(), s % P, done.copy()))
    keep = np.nonzero(~ended)[0].astype(np.int32)
    assert len(keep) >= survivors * pool_size, f"only {len(keep)} of {pool_size} pool games survive the preparation"
    return pool, tuple(actions), keep


@functools.lru_cache(maxsize=None)
def _o_pool(boundary):
    """O pieces only, rot 0, trans 2 * (s % 5): two rows cleared every five pieces, no game ever ends.  Played until the furthest
    game is 24 draws short of `boundary` — short enough that the preparation's own step_rt (which loads its draws in aligned
    groups of eight) does not come within the margin of the tables' end, the chained call after it does."""
    pool = engines.make("oracle", 8, 1, pieces=(6,), seeds=_pool_seeds(8))
    actions, rot = [], np.zeros(8, np.uint8)
    while int(pool.observe()[0]["piece_draws"].max()) < boundary - 24:
        trans = np.full(8, 2 * (len(actions) % 5), np.uint8)
        done = pool.step_rt(rot, trans, 0)
        actions.append((rot, trans, 0, done.copy()))
    assert not any(a[3].any() for a in actions)
    return pool, tuple(actions), np.arange(8, dtype=np.int32)


def _seeded(kind, n, P, H, prepared, pieces=(0, 1, 2, 3, 4, 5, 6), ms=400):
    """-> engine batch and oracle batch of n games tiled from the prepared pool (played at `ms` per step), equal before any rollout"""
    pool_ref, actions, keep = prepared
    pool_eng = engines.make(kind, pool_ref.n_games, P, height=H, pieces=pieces, seeds=_pool_seeds(pool_ref.n_games))
    for s, (r, t, player, done) in enumerate(actions):
        assert np.array_equal(pool_eng.step_rt(r, t, player, ms=ms), done), f"preparation step {s}: done flags"
    engines.assert_same_state(pool_eng, pool_ref, where="the pool after the preparation")
    src = keep[np.arange(n) % len(keep)]
    eng = engines.make(kind, n, P, height=H, pieces=pieces, seeds=_pool_seeds(n))
    ref = engines.make("oracle", n, P, height=H, pieces=pieces, seeds=_pool_seeds(n))
    ref.copy_from(pool_ref, src_idx=src)
    eng.restore(pool_eng.snapshot(src))
    pool_eng.close()
    engines.assert_same_state(eng, ref, where="seeded boards, before any rollout")
    return eng, ref


# ---------------------------------------------------------------- 2. the census
class Census:
    """Steps an oracle batch one step per rollout_random call (carrying its episode array) and keeps what was seen."""

    def __init__(self, ref, ms=400):
        self.ref, self.ms, self.episode, self.step = ref, ms, None, 0
        self.total = np.zeros(4, np.uint64)
        self.seen = dict(reward=0, combo=0, fifo=0, blocked=0, holes=0, draws=0,
                         multi_clears=0, combo2=0, combo3=0, fifo2=0, blocked_steps=0, hole_steps=0)     # these: board-steps
        self.first_draws = int(ref.observe()[0]["piece_draws"].max())

    def _look(self, prev):
        """after a step of the rollout only: what the seeded boards hold does not count"""
        rec, s = self.ref.observe()[0], self.seen
        for key, field in (("reward", "reward"), ("combo", "combo_count"), ("fifo", "fifo_len"), ("blocked", "lines_blocked"),
                           ("holes", "hole_draws"), ("draws", "piece_draws")):
            s[key] = max(s[key], int(rec[field].max()))
        s["multi_clears"] += int((rec["reward"] >= 2).sum())
        s["combo2"] += int((rec["combo_count"] >= 2).sum())
        s["combo3"] += int((rec["combo_count"] >= 3).sum())
        s["fifo2"] += int((rec["fifo_len"] >= 2).sum())
        s["blocked_steps"] += int((rec["lines_blocked"] > prev["lines_blocked"]).sum())      # lines blocked / holes drawn BY this step
        s["hole_steps"] += int((rec["hole_draws"] > prev["hole_draws"]).sum())
        return rec

    def roll(self, steps, ms=None):
        """-> the oracle's counters of these steps (of `ms` milliseconds; the census's own if None)"""
        ms = self.ms if ms is None else ms
        c = np.zeros(4, np.uint64)
        rec = self.ref.observe()[0]
        for _ in range(steps):
            self.episode, one = self.ref.rollout_random(1, first_step=self.step, ms=ms, episode=self.episode)
            c += one
            self.step += 1
            rec = self._look(rec)
        self.total += c
        return c

    def assert_rare_events(self, P):
        s = self.seen
        print(f"census P={P}: {s}, counters {self.total.tolist()}")
        assert s["reward"] >= 2, "no step cleared two rows"
        assert s["combo"] >= 3, "no combo of three"
        assert self.total[2] > 0 and self.total[3] > 0, "no lines cleared / sent"
        if P == 2:
            assert s["fifo"] >= 2, "no garbage queue two packets deep"
            assert s["blocked"] >= 1, "no blocked line"
            assert s["holes"] >= 2, "fewer than two hole draws"
            assert s["blocked_steps"] >= 1 and s["hole_steps"] >= 1, "no rollout step blocked a line / drew a hole itself"


def _call(eng, cen, launches, S, where, ms=400):
    """one rollout call of the engine against the same steps of the oracle: counters and state"""
    c, _ = eng.rollout_random(launches, S, first_step=cen.step, ms=ms)
    want = cen.roll(launches * S, ms=ms)
    assert c.tolist() == want.tolist(), f"{where}: counters {c.tolist()}, the oracle's {want.tolist()}"
    assert int(c[0]) == eng.n_games * launches * S
    engines.assert_same_state(eng, cen.ref, where=where)
    assert eng.take_errors() == 0, where


# ---------------------------------------------------------------- 3. CPU harness
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


# ---------------------------------------------------------------- 4. GPU
def _set_path(eng, path):
    if path == "unchained":
        eng.set_chained(False)
    elif path == "streams":
        eng.set_direct_dispatch(False)
    else:
        if path in ("queues", "queues_write_through"):
            eng.set_xcd_affine(False)
        eng.set_direct_dispatch(True, min_launches=1)


def _assert_path(eng, path):
    assert eng.rollout_was_direct() == (path not in ("streams", "unchained")), path
    if path == "queues_affine":
        assert eng.rollout_was_affine(), "the call did not run the XCD-affine kernels"
    else:
        assert not eng.rollout_was_affine()


def _interleaved_step(eng, ref, rng, k, ms=400):
    """One step_rt of random (r, t) on the batch's stream between two chained calls, finished games reset with explicit seeds
    (tetris_reset leaves G_EPISODE alone, so the oracle's carried episode array still holds), then an observe: a stream kernel must
    meet current memory after a queue's last release, and the next chained call's first acquire must see the step."""
    n, P = eng.n_games, eng.n_players
    player = rng.integers(0, P, n).astype(np.uint8)
    r, t = rng.integers(0, 4, n).astype(np.uint8), rng.integers(0, 10, n).astype(np.uint8)
    done = ref.step_rt(r, t, player, ms=ms)
    assert np.array_equal(eng.step_rt(r, t, player, ms=ms), done), f"interleaved step {k}: done flags"
    d = np.nonzero(done)[0].astype(np.int32)
    if len(d):
        sd = orc.episode_seed(d, 1000 + k)
        ref.reset(d, seeds=sd)
        eng.reset(d, seeds=sd)
    engines.assert_same_state(eng, ref, where=f"interleaved step {k}")


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


# ---------------------------------------------------------------- 5. RNG-table boundaries
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
