"""Seeded batches for the tests that start from mid-game boards: pools of oracle games played by the heuristic model
(tests/policy_model.py) or with O pieces only, tiled into batches of the engine under test; the census of an oracle stepped one
step per rollout call; the launch paths of the chained rollout; the heuristic play at an elapsed time per step; the packed
observation computed from oracle records.  The pools are cached here and nowhere else, so every test file shares one copy; they
are oracle batches and hold no GPU stream."""
import functools

import numpy as np

from oracle import oracle as orc
from tests import engines
from tests.policy_model import W_A, Model

SEED_POOL = 96
N_CPU, N_GPU = 333, 1100      # 1100: 18 waves of 64 (the last of 12 games; 24 workgroups XCD-affine), 35 k_duo waves (40)
# Steps of the preparation by players.  Three players: 64, not 40 — with 40 the oracle's census at 333 games sees no combo of three
# after a rollout step (a player moves every 1 200 ms against a combo timer that starts at 1 800).  64 is no multiple of three, so
# the rollout's rotation meets players that moved 400 or 800 ms ago with their combos alive: 7 board-steps with a combo of three.
PREP = {1: 24, 2: 40, 3: 64}


def _pool_seeds(pool):
    return orc.episode_seed(np.arange(pool), 0)


# ---------------------------------------------------------------- seeding
@functools.lru_cache(maxsize=None)
def _model_pool(P, H, ms=400, prep=None, pool_size=SEED_POOL, survivors=0.75):
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
    assert not any(a[3].any() for a in actions), "a game of the O-piece pool ended"
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


# ---------------------------------------------------------------- the census
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
    assert int(c[0]) == eng.n_games * launches * S, f"{where}: {int(c[0])} env-steps counted, not {eng.n_games * launches * S}"
    engines.assert_same_state(eng, cen.ref, where=where)
    errors = eng.take_errors()
    assert errors == 0, f"{where}: take_errors() is {errors:#x}"


# ---------------------------------------------------------------- the launch paths of the chained rollout
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
    assert eng.rollout_was_direct() == (path not in ("streams", "unchained")), f"{path}: rollout_was_direct() is {eng.rollout_was_direct()}"
    if path == "queues_affine":
        assert eng.rollout_was_affine(), "the call did not run the XCD-affine kernels"
    else:
        assert not eng.rollout_was_affine(), f"{path}: the call ran the XCD-affine kernels"


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


# ---------------------------------------------------------------- heuristic play at `ms` per step
POOL = 32                               # games the heuristic model plays; tiled over the batch


def _heur_steps(P, ms):
    """steps the heuristic plays before the random ones: none for several players below 100 ms (the queue would fill), 130 at
    3001 (1000 -> 200 -> 100 -> 50 takes 80 + 20 + 25 speed-ups, one per tick; random play ends a game after about 40 steps)"""
    if P > 1 and ms < 100:
        return 0
    return 130 if ms == 3001 else 32


@functools.lru_cache(maxsize=None)
def _heuristic_play(P, ms):
    """The heuristic model of tests/policy_model.py on a pool of 32 oracle games, a random acting player per game and step,
    finished games reset by the built-in seed schedule -> ((rot, trans, player, done) [32] per step)"""
    pool = engines.make("oracle", POOL, P, seeds=orc.episode_seed(np.arange(POOL), 0))
    m = Model(pool, ms=ms)
    rng = np.random.default_rng(1000 * P + ms)
    out = []
    for _ in range(_heur_steps(P, ms)):
        player = rng.integers(0, P, POOL).astype(np.uint8)
        r, t, _ = m.choose(W_A, player)
        done, _, _ = m.step(r, t, player, True)
        out.append((r.copy(), t.copy(), player, done.copy()))
    return tuple(out)


# ---------------------------------------------------------------- the packed observation, from oracle records
def _expected_packed(rec, me, P, H):
    """state_dict + unpacker semantics (state_processors.py:23-54; state_unpack.py:88-137) computed from oracle records:
    -> visual [P][n][H][10], vector [P][n][12], piece [P][n], slot 0 = player me[i]'s board"""
    n = len(me)
    visual, vector, piece = np.zeros((P, n, H, 10), np.uint8), np.zeros((P, n, 12), np.uint8), np.zeros((P, n), np.uint8)
    for sl in range(P):
        who = me if sl == 0 else (P - 1 - me)
        r = rec[np.arange(n), who]
        visual[sl] = (r["field"][:, :H, :] > 0).astype(np.uint8)
        vector[sl, :, 0] = r["x"].astype(np.uint8); vector[sl, :, 1] = r["y"].astype(np.uint8); vector[sl, :, 2] = r["inc_count"]
        vector[sl, :, 3] = np.minimum(25000, (r["combo_remaining"].astype(np.uint32) + 50) & 0xFFFF) // 100
        vector[sl, :, 4] = r["combo_count"]
        vector[sl, np.arange(n), 5 + r["next"]] = 1
        piece[sl] = r["piece"]
    return visual, vector, piece
