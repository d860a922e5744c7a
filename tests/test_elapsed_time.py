"""Every stepping entry point at elapsed times per action other than 400 ms.

`ms` is the reference's settings["time_elapsed_each_action"], handed to finish_action(ms): it drives the drop delay and its speed-ups,
the lock-down timer, the garbage queue's delays and the combo timer (tetris_engine.h: gravity_due, soft_drop, tick, q_add, q_block,
q_release, combo_gain, combo_expire).  At 400 ms all of these sit in one narrow regime; the values here put them in the others:

      0  time stands still: nothing ever expires, combos only grow
      1  almost still
     50  combos far longer than at 400 (one player: counts above 8), packets queued for tens of steps
    170  no timer is a multiple of the tick
    399  the lock-down delay of 400 needs a third tick
    401  the lock-down fires on the first tick after the piece came to rest
   1000  a packet's delay of 1000 is not yet over on the next tick (strict >)
   1500  a packet is released on the tick after it arrived
   3001  a speed-up on every tick: the drop delay passes all four reduction tiers down to 10
  60000  many lines per expired combo, every timer long over on every tick

The compiled reference's traces at these values pin the oracle (tests/golden/trace_*_ms*.npz, tests/test_oracle_golden.py); here
the oracle checks what the traces cannot reach: batches, k_duo, the three- and four-player kernels, the device-side and fused
forms, the planning, policy and acting calls, the chained rollout kernels.  Every comparison is exact equality.  `harness` = the
kernel bodies built by g++ (CPU suite), `hip` = the product on the GPU.

No game is ever left out of a comparison.  The engine queues at most 8 garbage packets per board (TETRIS_ERR_FIFO,
tests/test_edge_cases.py), and small `ms` lets packets pile up, so the inputs are chosen to stay clear of that: heuristic play of two
or more players only at ms >= 100, random (r, t) below; every test asserts on the ORACLE's records that no board ever has more than
6 packets pending.  Each sweep and rollout test also asserts, again on the oracle alone, that its boards were in the regime its
`ms` stands for (Regime, FLOORS)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import engines
from tests.act_support import Call, model, pieces_of, random_maps
from tests.buffers import Buf
from tests.plan_support import _bits, _device_lists
from tests.policy_model import W_A, Model, _assert_rollout
from tests.seeded import (N_CPU, N_GPU, POOL, PREP, Census, _assert_path, _call, _expected_packed, _heuristic_play, _interleaved_step,
                          _model_pool, _seeded, _set_path)

MS_ALL = (0, 1, 50, 170, 399, 401, 1000, 1500, 3001, 60000)
MS_FEW = (50, 1500, 3001)
N_HARNESS, N_LANES = 192, 2048 + 3      # 2051: one lane per game, the last workgroup (and wave) ragged
MAX_PENDING = 6
RANDOM_STEPS = 32


def _n(kind):
    return N_LANES if kind == "hip" else N_HARNESS


# ---------------------------------------------------------------- the census of the regime, from the oracle alone
class Regime:
    """What the oracle's boards showed over a run; look() after every step with the records before and after it."""

    def __init__(self):
        self.min_drop_delay, self.max_combo, self.max_pending, self.max_sent = 1000, 0, 0, 0
        # board-steps
        self.low_delay = self.long_combo = self.timer_locks = self.prompt_holes = self.pending2 = self.blocked = 0
        self.arrived = None

    def look(self, prev, rec):
        """prev, rec: records [n, P] before and after one step (a game reset inside the step counts as nothing)"""
        self.min_drop_delay = min(self.min_drop_delay, int(rec["drop_delay"].min()))
        self.max_combo = max(self.max_combo, int(rec["combo_count"].max()))
        self.max_pending = max(self.max_pending, int(rec["fifo_len"].max()))
        assert self.max_pending <= MAX_PENDING, f"the oracle has {self.max_pending} garbage packets pending on one board: wrong inputs"
        sent = (rec["lines_sent"].astype(np.int64) - prev["lines_sent"]) & 0xFFFF
        sent = np.where(rec["piece_draws"] < prev["piece_draws"], 0, sent)                   # (a game reset inside the step)
        self.max_sent = max(self.max_sent, int(sent.max()))
        self.low_delay += int((rec["drop_delay"] <= 50).sum())
        self.long_combo += int((rec["combo_count"] > 8).sum())
        self.pending2 += int((rec["fifo_len"] >= 2).sum())
        self.blocked += int((rec["lines_blocked"] > prev["lines_blocked"]).sum())
        # every step deals every living board one piece (PythonHandle.cpp:149-188, loop 1); a second one in the same step is dealt
        # by the tick whose lock-down timer (armed, and over) locked the piece it found
        self.timer_locks += int((rec["piece_draws"].astype(np.int64) - prev["piece_draws"] >= 2).sum())
        holes = rec["hole_draws"] > prev["hole_draws"]
        if self.arrived is not None and self.arrived.shape == holes.shape:
            self.prompt_holes += int((self.arrived & holes).sum())                           # a row pushed in the step after its packet arrived
        self.arrived = rec["fifo_len"] > prev["fifo_len"]

    def forget(self, idx):
        """games reset by hand: their packets are gone"""
        if self.arrived is not None and len(idx):
            self.arrived[idx] = False

    def check(self, label, P, ms):
        print(f"census {label} P={P} ms={ms}: min drop delay {self.min_drop_delay}, max combo {self.max_combo}, max pending {self.max_pending}, "
              f"timer locks {self.timer_locks}, board-steps with drop delay <= 50: {self.low_delay}, with a combo above 8: {self.long_combo}, "
              f"with two packets pending: {self.pending2}, that blocked lines: {self.blocked}, with a hole drawn in the step after a packet "
              f"arrived: {self.prompt_holes}, most lines sent by one step {self.max_sent}")
        for what, floor in FLOORS.get((label, P, ms), {}).items():
            assert getattr(self, what) >= floor, f"{label} P={P} ms={ms}: '{what}' is {getattr(self, what)}, the floor is {floor}"
        if ms == 0:
            assert self.timer_locks == 0 and self.min_drop_delay == 1000, "no timer can run out while time stands still"


# Floors: at most half of what the oracle showed at the CPU harness's sizes (the observed value beside each); the GPU cases
# run the same inputs over ten times as many games.  Never taken from the engine.  What each `ms` must show:
#   3001  board-steps with a drop delay <= 50           50, one player  board-steps with a combo count above 8
#   1500, two players  a hole drawn in the step after a packet arrived        401  lock_armed boards that the timer locked
FLOORS = {
    ("step_rt", 1, 3001): dict(low_delay=2000),       # 4 208
    ("step_rt", 2, 3001): dict(low_delay=250),        # 566
    ("step_rt", 3, 3001): dict(low_delay=5000),       # 10 380
    ("step_rt", 4, 3001): dict(low_delay=12000),      # 24 175
    ("step_keys", 1, 3001): dict(low_delay=2400),     # 4 839
    ("step_keys", 2, 3001): dict(low_delay=220),      # 452
    ("step_rt", 1, 50): dict(long_combo=500),         # 1 013 (max combo 12)
    ("step_keys", 1, 50): dict(long_combo=500),       # 1 013
    ("step_rt", 2, 1500): dict(prompt_holes=500),     # 1 019
    ("step_keys", 2, 1500): dict(prompt_holes=500),   # 1 062
    ("step_rt", 2, 401): dict(timer_locks=2),         # 5 (at 399: 1)
    ("step_rt", 3, 401): dict(timer_locks=2),         # 5
    ("step_rt", 4, 401): dict(timer_locks=1),         # 3
    ("step_keys", 1, 401): dict(timer_locks=20),      # 43 (at 399: 2)
    ("step_keys", 2, 401): dict(timer_locks=20),      # 41 (at 399: 13)
    # the rollouts, from tests/test_chain_midgame.py's 333 games of the CPU case
    ("rollout", 1, 50): dict(long_combo=100),         # 209 (max combo 10)
    ("rollout", 2, 1500): dict(prompt_holes=75),      # 159
    ("rollout", 3, 1500): dict(prompt_holes=100),     # 225
    ("rollout", 1, 3001): dict(low_delay=2500),       # 5 223
    ("rollout", 2, 3001): dict(low_delay=2500),       # 5 144
    ("rollout", 3, 3001): dict(low_delay=9000),       # 19 947
}


# ---------------------------------------------------------------- inputs


def _tiled_pair(kind, n, P, height=20):
    """game g starts as pool game g % 32"""
    seeds = orc.episode_seed(np.arange(n) % POOL, 0)
    return engines.make(kind, n, P, height, seeds=seeds), engines.make("oracle", n, P, height, seeds=seeds)


def _reset_both(eng, ref, idx, episode, cen=None):
    if len(idx):
        episode[idx] += 1
        sd = orc.episode_seed(idx % POOL, episode[idx])
        eng.reset(idx, sd)
        ref.reset(idx, sd)
        if cen is not None:
            cen.forget(idx)


# ---------------------------------------------------------------- 1. per-step entry points
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("P", [1, 2, 3, 4])
@pytest.mark.parametrize("ms", MS_ALL)
def test_step_rt_at_every_elapsed_time(kind, P, ms):
    """tetris_step_rt over all games (two players: k_duo; three and four: tetris_hip_multi.hip), a random acting player per game,
    done / lines / dead of every step, the full state every 8 steps; the first steps are the heuristic's (lines, combos, garbage),
    the last 32 random, with resets of finished and of running games."""
    n = _n(kind)
    heur = _heuristic_play(P, ms)
    eng, ref = _tiled_pair(kind, n, P)
    cen, rng = Regime(), np.random.default_rng(7 * ms + P)
    episode, tile = np.zeros(n, np.int64), np.arange(n) % POOL
    for s in range(len(heur) + RANDOM_STEPS):
        if s < len(heur):
            rot, trans, player = (a[tile] for a in heur[s][:3])
        else:
            rot, trans = rng.integers(0, 4, n).astype(np.uint8), rng.integers(0, 10, n).astype(np.uint8)
            player = rng.integers(0, P, n).astype(np.uint8)
        prev = ref.observe()[0]
        done, lines, dead = eng.step_rt(rot, trans, player, ms=ms, full=True)
        want = ref.step_rt(rot, trans, player, ms=ms)
        rec = ref.observe()[0]
        assert np.array_equal(done, want), f"step {s}: done"
        assert np.array_equal(lines, rec["reward"]) and np.array_equal(dead, rec["dead"]), f"step {s}: lines / dead"
        if s < len(heur):
            assert np.array_equal(want, heur[s][3][tile]), f"step {s}: the tiled games left the pool's path"
        cen.look(prev, rec)
        if s % 8 == 7:
            engines.assert_same_state(eng, ref, where=f"step {s}")
        idx = np.nonzero(want)[0]
        if s >= len(heur) and s % 16 == 15:                        # running games too (last_winner = -1)
            idx = np.union1d(idx, np.arange(s % 7, n, 7))
        _reset_both(eng, ref, idx.astype(np.int32), episode, cen)
    engines.assert_same_state(eng, ref, where="end")
    assert eng.take_errors() == 0
    cen.check("step_rt", P, ms)


def _random_keys(rng, n, P, K):
    """key lists as in tests/test_engine_vs_oracle.py: every key 0..10, a hard drop at the end of most, mostly one player acting"""
    lens = rng.integers(0, K - 2, (n, P)).astype(np.uint8)
    keys = rng.integers(0, 11, (n, P, K)).astype(np.uint8)
    lock = rng.random((n, P)) < 0.6
    for p in range(P):
        rows = np.nonzero(lock[:, p])[0]
        keys[rows, p, lens[rows, p]] = 7
        lens[rows, p] += 1
    if P == 2:
        idle, solo = rng.integers(0, 2, n), rng.random(n) < 0.7
        for p in range(2):
            rows = np.nonzero(solo & (idle == p))[0]
            keys[rows, p, 0] = 0
            lens[rows, p] = 1
    return keys, lens


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("ms", MS_ALL)
def test_step_keys_on_shuffled_subsets_at_every_elapsed_time(kind, P, ms):
    """tetris_step_keys with an index list (two players: k_game<2>, which k_duo hides from calls over all games): every step is
    two calls over the two parts of a random permutation of the games.  The heuristic's (r, t) as key lists first, then random
    key lists with soft drops to the floor and without a hard drop, which leave the lock-down timer armed for the tick."""
    n, K = _n(kind), 20
    heur = _heuristic_play(P, ms)
    eng, ref = _tiled_pair(kind, n, P)
    cen, rng = Regime(), np.random.default_rng(11 * ms + P)
    episode, tile = np.zeros(n, np.int64), np.arange(n) % POOL
    for s in range(len(heur) + RANDOM_STEPS):
        if s < len(heur):
            rot, trans, player = (a[tile] for a in heur[s][:3])
            keys, lens = np.zeros((n, P, K), np.uint8), np.ones((n, P), np.uint8)          # [0] for the others
            for g in range(n):
                k = [8] * int(rot[g]) + [2] + [3] * int(trans[g]) + [7]
                keys[g, player[g], : len(k)] = k
                lens[g, player[g]] = len(k)
        else:
            keys, lens = _random_keys(rng, n, P, K)
        prev = ref.observe()[0]
        perm = rng.permutation(n).astype(np.int32)
        want = np.zeros(n, np.uint8)
        for idx in (perm[: n // 3], perm[n // 3:]):
            done, lines, dead = eng.step_keys(keys[idx], lens[idx], ms=ms, idx=idx)
            ref.make_actions(keys[idx], lens[idx], idx=idx)
            want[idx] = ref.finish_actions(ms, idx=idx)
            part = ref.observe(idx)[0]
            assert np.array_equal(done, want[idx]), f"step {s}: done"
            assert np.array_equal(lines, part["reward"]) and np.array_equal(dead, part["dead"]), f"step {s}: lines / dead"
        rec = ref.observe()[0]
        if s < len(heur):
            assert np.array_equal(want, heur[s][3][tile]), f"step {s}: the tiled games left the pool's path"
        cen.look(prev, rec)
        if s % 8 == 7:
            engines.assert_same_state(eng, ref, where=f"step {s}")
        _reset_both(eng, ref, np.nonzero(want)[0].astype(np.int32), episode, cen)
    engines.assert_same_state(eng, ref, where="end")
    assert eng.take_errors() == 0
    cen.check("step_keys", P, ms)


# ---------------------------------------------------------------- 2. device-side forms
MS_DEV = MS_FEW + (401,)


def _random_rt(rng, n, P):
    return rng.integers(0, 4, n).astype(np.uint8), rng.integers(0, 10, n).astype(np.uint8), rng.integers(0, P, n).astype(np.uint8)


def _schedule_reset(ref, done, episode, cen):
    """the oracle's side of auto_reset: the built-in seed schedule by game and episode -> the number of games reset"""
    idx = np.nonzero(done)[0].astype(np.int32)
    if len(idx):
        episode[idx] += 1
        ref.reset(idx, orc.episode_seed(idx, episode[idx]))
        cen.forget(idx)
    return len(idx)


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("ms", MS_DEV)
def test_step_rt_dev_with_auto_reset(kind, P, ms):
    n = _n(kind)
    seeds = orc.episode_seed(np.arange(n), 0)
    eng, ref = engines.make(kind, n, P, seeds=seeds), engines.make("oracle", n, P, seeds=seeds)
    rng, cen = np.random.default_rng(3 * ms + P), Regime()
    episode, ended = np.zeros(n, np.int64), 0
    done_d, lines_d, dead_d = Buf(kind, np.zeros(n, np.uint8)), Buf(kind, np.zeros((P, n), np.uint8)), Buf(kind, np.zeros((P, n), np.uint8))
    for s in range(64):
        rot, trans, player = _random_rt(rng, n, P)
        r_d, t_d, p_d = Buf(kind, rot), Buf(kind, trans), Buf(kind, player)
        prev = ref.observe()[0]
        eng.step_rt_dev(r_d.ptr, t_d.ptr, p_d.ptr, done_d.ptr, lines_d.ptr, dead_d.ptr, ms=ms, auto_reset=True)
        want = ref.step_rt(rot, trans, player, ms=ms)
        rec = ref.observe()[0]
        cen.look(prev, rec)
        if kind == "hip":
            eng.sync()
        assert np.array_equal(done_d.get(), want), f"step {s}: done"
        assert np.array_equal(lines_d.get().T, rec["reward"]) and np.array_equal(dead_d.get().T, rec["dead"]), f"step {s}: lines / dead"
        ended += _schedule_reset(ref, want, episode, cen)
        if s % 8 == 7:
            engines.assert_same_state(eng, ref, where=f"step {s}")
    assert ended > n // 2, "auto-reset is hardly inside the comparison"
    assert eng.take_errors() == 0
    cen.check("step_rt_dev", P, ms)


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("P,H", [(1, 20), (2, 20), (2, 21)])
@pytest.mark.parametrize("ms", MS_DEV)
def test_step_rt_observe_dev(kind, P, H, ms):
    """the fused step-and-observation kernels (H = 20, one and two players) and the two-kernel fallback (H = 21): the step against
    the oracle's, the observation bit-equal to observe_packed of the state just checked and to the oracle's records"""
    n = _n(kind)
    seeds = orc.episode_seed(np.arange(n), 0)
    eng, ref = engines.make(kind, n, P, H, seeds=seeds), engines.make("oracle", n, P, H, seeds=seeds)
    rng, cen = np.random.default_rng(5 * ms + 10 * P + H), Regime()
    episode, ended = np.zeros(n, np.int64), 0
    done_d, lines_d, dead_d = Buf(kind, np.zeros(n, np.uint8)), Buf(kind, np.zeros((P, n), np.uint8)), Buf(kind, np.zeros((P, n), np.uint8))
    vis_d, vec_d, pc_d = Buf(kind, np.zeros((P, n, H, 10), np.uint8)), Buf(kind, np.zeros((P, n, 12), np.uint8)), Buf(kind, np.zeros((P, n), np.uint8))
    for s in range(48):
        rot, trans, player = _random_rt(rng, n, P)
        nxt = rng.integers(0, P, n).astype(np.uint8)
        r_d, t_d, p_d, n_d = Buf(kind, rot), Buf(kind, trans), Buf(kind, player), Buf(kind, nxt)
        prev = ref.observe()[0]
        eng.step_rt_observe_dev(r_d.ptr, t_d.ptr, p_d.ptr, done_d.ptr, lines_d.ptr, dead_d.ptr, n_d.ptr,
                                vis_d.ptr, vec_d.ptr, pc_d.ptr, ms=ms, auto_reset=True)
        want = ref.step_rt(rot, trans, player, ms=ms)
        rec = ref.observe()[0]
        cen.look(prev, rec)
        if kind == "hip":
            eng.sync()
        assert np.array_equal(done_d.get(), want), f"step {s}: done"
        assert np.array_equal(lines_d.get().T, rec["reward"]) and np.array_equal(dead_d.get().T, rec["dead"]), f"step {s}: lines / dead"
        ended += _schedule_reset(ref, want, episode, cen)
        got = vis_d.get(), vec_d.get(), pc_d.get()
        for g, w, name in zip(got, _expected_packed(ref.observe()[0], nxt, P, H), ("visual", "vector", "piece")):
            assert np.array_equal(g, w), f"step {s}: '{name}' differs from the oracle's records"
        if s % 6 == 5:
            engines.assert_same_state(eng, ref, where=f"step {s}")
            for g, w, name in zip(got, eng.observe_packed(None, nxt), ("visual", "vector", "piece")):
                assert np.array_equal(g, w), f"step {s}: '{name}' differs from observe_packed"
    assert ended > n // 4
    assert eng.take_errors() == 0
    cen.check("step_rt_observe_dev", P, ms)


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("ms", MS_DEV)
def test_lists_simulated_and_stepped_on_the_device(kind, P, ms):
    """tetris_simulate_lists_dev(finalize) of every enumerated list and tetris_step_lists_dev of a chosen one against step_keys of
    the same lists on the oracle (make_actions + finish_actions(ms)): fields, done, lines, dead; then the stepped state."""
    n, L, K = _n(kind), 128, 48
    seeds = orc.episode_seed(np.arange(n), 0)
    eng, ref = engines.make(kind, n, P, seeds=seeds), engines.make("oracle", n, P, seeds=seeds)
    rng, cen = np.random.default_rng(13 * ms + P), Regime()
    episode = np.zeros(n, np.int64)

    def step(keys, lens, s):
        """the oracle's step_keys, finished games reset by hand on both"""
        prev = ref.observe()[0]
        ref.make_actions(keys, lens)
        want = ref.finish_actions(ms)
        cen.look(prev, ref.observe()[0])
        return want

    for s in range(20):                                            # mid-game boards, played at `ms`
        rot, trans, player = _random_rt(rng, n, P)
        want = ref.step_rt(rot, trans, player, ms=ms)
        assert np.array_equal(eng.step_rt(rot, trans, player, ms=ms), want)
        idx = np.nonzero(want)[0].astype(np.int32)
        if len(idx):
            episode[idx] += 1
            eng.reset(idx, orc.episode_seed(idx, episode[idx]))
            ref.reset(idx, orc.episode_seed(idx, episode[idx]))
    engines.assert_same_state(eng, ref, where="before planning")
    for s in range(6):
        player = rng.integers(0, P, n)
        cnt, lens, keys, pl = _device_lists(kind, eng, player, False, L=L, K=K)
        c, ln, kk = cnt.get(), lens.get(), keys.get()
        assert (c >= 1).all()
        if s % 3 == 0:                                             # every list of every game, finalized: one oracle game per list
            cols = Buf.full(kind, (L, P, 10, n), np.uint32)
            done, lines, dead = Buf.full(kind, (L, n), np.uint8, 77), Buf.full(kind, (L, P, n), np.uint8, 77), Buf.full(kind, (L, P, n), np.uint8, 77)
            blob = eng.snapshot()
            eng.simulate_lists_dev(cnt.ptr, lens.ptr, keys.ptr, cols.ptr, max_lists=L, max_keys=K, player=pl.ptr, finalize=True, ms=ms,
                                   done=done.ptr, lines=lines.ptr, dead=dead.ptr)
            got_cols, got_done, got_lines, got_dead = cols.get(), done.get(), lines.get(), dead.get()
            assert np.array_equal(eng.snapshot(), blob), "simulate wrote the batch's state"
            T = int(c.sum())
            src = np.repeat(np.arange(n), c).astype(np.int32)
            lk = np.concatenate([np.arange(x) for x in c])
            Kh, Lh = np.zeros((T, P, K), np.uint8), np.ones((T, P), np.uint8)
            Kh[np.arange(T), player[src]] = kk[src, lk]
            Lh[np.arange(T), player[src]] = ln[src, lk]
            one = orc.OracleBatch(T, P, 20, 10)
            one.copy_from(ref, dst_idx=np.arange(T, dtype=np.int32), src_idx=src)
            one.make_actions(Kh, Lh)
            want_done = one.finish_actions(ms)
            rec = one.observe()[0]
            assert np.array_equal(_bits(got_cols[lk, :, :, src], 20), rec["field"][:, :, :20] > 0), f"round {s}: simulated fields"
            assert np.array_equal(got_done[lk, src], want_done), f"round {s}: simulated done"
            assert np.array_equal(got_lines[lk, :, src], rec["reward"]) and np.array_equal(got_dead[lk, :, src], rec["dead"]), f"round {s}"
        choice = rng.integers(-3, 60, n).astype(np.int32)          # clamped into [0, count - 1]
        ch = Buf.full(kind, (n,), np.int32)
        ch.put(choice)
        done, lines, dead = Buf.full(kind, (n,), np.uint8), Buf.full(kind, (P, n), np.uint8), Buf.full(kind, (P, n), np.uint8)
        eng.step_lists_dev(ch.ptr, cnt.ptr, lens.ptr, keys.ptr, done.ptr, lines.ptr, dead.ptr, max_lists=L, max_keys=K, player=pl.ptr, ms=ms)
        pick = np.clip(choice, 0, c - 1)
        Kh, Lh = np.zeros((n, P, K), np.uint8), np.ones((n, P), np.uint8)
        Kh[np.arange(n), player] = kk[np.arange(n), pick]
        Lh[np.arange(n), player] = ln[np.arange(n), pick]
        want = step(Kh, Lh, s)
        rec = ref.observe()[0]
        assert np.array_equal(done.get(), want), f"round {s}: step_lists done"
        assert np.array_equal(lines.get().T, rec["reward"]) and np.array_equal(dead.get().T, rec["dead"]), f"round {s}: step_lists lines / dead"
        engines.assert_same_state(eng, ref, where=f"round {s}: after step_lists_dev")
        idx = np.nonzero(want)[0].astype(np.int32)
        if len(idx):
            episode[idx] += 1
            eng.reset(idx, orc.episode_seed(idx, episode[idx]))
            ref.reset(idx, orc.episode_seed(idx, episode[idx]))
            cen.forget(idx)
    assert eng.take_errors() == 0
    cen.check("lists", P, ms)


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("ms", MS_DEV)
def test_policy_step_and_rollout_equal_the_model(kind, P, ms):
    """tetris_step_policy_dev (auto-reset) and tetris_rollout_policy (single and fused launches) against the model stepping the
    oracle at `ms`; 67 games: a wave and a ragged second one (the model costs 40 oracle games per game and step)"""
    n = 67
    seeds = orc.episode_seed(np.arange(n), 0)
    b, o = engines.make(kind, n, P, seeds=seeds), engines.make("oracle", n, P, seeds=seeds)
    m, cen, rng = Model(o, ms=ms), Regime(), np.random.default_rng(17 * ms + P)
    w, pl = Buf.full(kind, (8,), np.int16).put(W_A), Buf.full(kind, (n,), np.uint8)
    done, lines, dead = Buf.full(kind, (n,), np.uint8, 7), Buf.full(kind, (P, n), np.uint8, 7), Buf.full(kind, (P, n), np.uint8, 7)
    rot, trans = Buf.full(kind, (n,), np.uint8, 7), Buf.full(kind, (n,), np.uint8, 77)
    for s in range(16):
        player = rng.integers(0, P, n).astype(np.uint8)
        pl.put(player)
        b.step_policy_dev(w.ptr, done.ptr, lines.ptr, dead.ptr, rot=rot.ptr, trans=trans.ptr, player=pl.ptr, ms=ms, auto_reset=True)
        prev = o.observe()[0]
        r, t, _ = m.choose(W_A, player)
        want_done, want_lines, want_dead = m.step(r, t, player, True)
        for name, got, want in (("done", done, want_done), ("lines", lines, want_lines.T), ("dead", dead, want_dead.T), ("rot", rot, r), ("trans", trans, t)):
            assert np.array_equal(got.get(), want), f"step {s}: step_policy_dev '{name}'"
        engines.assert_same_state(b, o, where=f"step {s}: step_policy_dev")
        cen.look(prev, o.observe()[0])                             # (a game reset inside the step shows fresh records: counted as nothing)
    steps = 24
    for s in range(16, 16 + steps):                                # the model's rollout, looked at after every step
        prev = o.observe()[0]
        m.rollout(W_A, 1, first_step=s)
        cen.look(prev, o.observe()[0])
    counters = np.zeros(4, np.int64)
    for launches, spl, first in ((10, 1, 16), (3, 4, 26), (2, 1, 38)):
        c, _ = b.rollout_policy(w.ptr, launches, spl, first_step=first, ms=ms)
        counters += c.astype(np.int64)
    assert counters[0] == n * steps
    _assert_rollout(kind, b, m, counters, f"rollout_policy at {ms} ms")
    assert b.take_errors() == 0
    cen.check("policy", P, ms)


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("ms", MS_DEV)
def test_step_eval_dev(kind, P, ms):
    """tetris_step_eval_dev (auto-reset; ARGMAX and EPSILON in turn) against the model of tests/act_support.py choosing and the
    oracle stepping at `ms`"""
    n = _n(kind)
    seeds = orc.episode_seed(np.arange(n), 0)
    a, o = engines.make(kind, n, P, seeds=seeds), engines.make("oracle", n, P, seeds=seeds)
    rng, cen = np.random.default_rng(19 * ms + P), Regime()
    ids, episode, ended = np.arange(n), np.zeros(n, np.int64), 0
    done, lines, dead = Buf(kind, np.full(n, 7, np.uint8)), Buf(kind, np.full((P, n), 7, np.uint8)), Buf(kind, np.full((P, n), 7, np.uint8))
    for s in range(40):
        mode = ("argmax", "epsilon")[s % 2]
        player = rng.integers(0, P, n).astype(np.uint8)
        ae = random_maps(rng, n, 7, np.float32, "normal")
        kw = dict(seed=9, draw=s, epsilon=0.5)
        want = model(ae, pieces_of(o, player), ids, mode, **kw)
        call = Call(kind, a, ae, mode, player=player, **kw)
        a.step_eval_dev(call.e, done.ptr, lines.ptr, dead.ptr, ms=ms, auto_reset=True)
        prev = o.observe()[0]
        want_done = o.step_rt(want["rot"], want["trans"], player, ms=ms)
        rec = o.observe()[0]
        cen.look(prev, rec)
        got = call.get()
        assert np.array_equal(got["rot"], want["rot"]) and np.array_equal(got["trans"], want["trans"]), f"step {s} ({mode}): the choice"
        assert np.array_equal(done.get(), want_done), f"step {s}: done"
        assert np.array_equal(lines.get(), rec["reward"].T) and np.array_equal(dead.get(), rec["dead"].T), f"step {s}: lines / dead"
        ended += _schedule_reset(o, want_done, episode, cen)
        if s % 8 == 7:
            engines.assert_same_state(a, o, where=f"step {s}")
    assert ended > 0, "no game finished: auto-reset is not inside the comparison"
    assert a.take_errors() == 0
    cen.check("step_eval_dev", P, ms)


# ---------------------------------------------------------------- 3. rollouts
class RolloutCensus(Census):
    """tests/seeded.py's census (one oracle step per rollout_random call) that also keeps the regime"""

    def __init__(self, ref, ms):
        super().__init__(ref, ms)
        self.regime = Regime()

    def _look(self, prev):
        rec = super()._look(prev)
        self.regime.look(prev, rec)
        return rec


def _prepared(P, ms):
    """the seeding pool of tests/seeded.py played at `ms`: 48 games; at 3001 for 130 steps, so that the drop delay
    is down at 50 when the rollout begins (a round of several players ends when one tops out: 12 of 48 two-player games get there)"""
    long = ms == 3001
    pool = _model_pool(P, 20, ms=ms, prep=130 if long else PREP[P], pool_size=48, survivors=0.2 if long and P > 1 else 0.75)
    assert int(pool[0].observe()[0]["fifo_len"].max()) <= MAX_PENDING
    return pool


@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("ms", MS_FEW)
def test_cpu_single_steps_equal_fused_steps(P, ms):
    """CPU harness, 333 seeded games: 40 launches of one step, one launch of 40 steps and the oracle leave the same boards and
    counters, twice"""
    n, K = N_CPU, 40
    prepared = _prepared(P, ms)
    single, ref = _seeded("harness", n, P, 20, prepared, ms=ms)
    fused, _ = _seeded("harness", n, P, 20, prepared, ms=ms)
    cen = RolloutCensus(ref, ms)
    for rep in range(2):
        before = cen.total.copy()
        cK, _ = fused.rollout_random(1, K, first_step=cen.step, ms=ms)
        _call(single, cen, K, 1, f"{K} launches of one step, round {rep}", ms=ms)
        assert cK.tolist() == (cen.total - before).tolist()
        engines.assert_same_state(fused, ref, where=f"one launch of {K} steps, round {rep}")
        assert fused.take_errors() == 0
    cen.regime.check("rollout", P, ms)


# (launches, steps per launch): S = 1, S = 3 and S = 0 take turns, 60 env-steps in all
TURNS = {1: [(12, 1), (4, 3), (5, 0), (20, 1), (3, 3), (7, 1)], 2: [(20, 1), (33, 1), (7, 1)]}
PATHS = {1: ("unchained", "streams", "queues_write_through", "queues_affine"), 2: ("unchained", "streams", "queues", "queues_affine")}


@pytest.mark.gpu
@pytest.mark.parametrize("P,path", [(P, path) for P in (1, 2) for path in PATHS[P]])
@pytest.mark.parametrize("ms", MS_FEW)
def test_gpu_chained_calls(P, path, ms):
    """1 100 seeded boards (18 waves with a short last one, 35 k_duo waves): the four k_chain* kernels and the chained k_duo on
    every launch path, one step_rt at `ms` with resets between the calls; counters, full state, error bits and the launch path
    after EVERY call."""
    eng, ref = _seeded("hip", N_GPU, P, 20, _prepared(P, ms), ms=ms)
    _set_path(eng, path)
    cen, rng = RolloutCensus(ref, ms), np.random.default_rng(41 + P)
    for k, (launches, S) in enumerate(TURNS[P]):
        if path == "streams" and P == 1:
            launches = min(launches, 15)
        _call(eng, cen, launches, S, f"{path}, call {k} ({launches} x {S})", ms=ms)
        _assert_path(eng, path)
        _interleaved_step(eng, ref, rng, k, ms=ms)
    for S in (0, 1, 3) if P == 1 else (1,):
        assert eng.rollout_is_chained(S) == (path != "unchained")          # no wave gave up, nothing fell back
    print(f"launch path P={P} ms={ms}: asked for {path}; direct {eng.rollout_was_direct()}, affine {eng.rollout_was_affine()}, "
          f"chained {eng.rollout_is_chained(1)}")
    cen.regime.check("rollout", P, ms)
