"""Both capacity limits of include/tetris_hip.h — 8 pending garbage packets per board, 624 * chunks piece draws per episode — on
every step path, harness (`-m "not gpu"`) and MI355X (`-m gpu`).

The reference has neither limit (Garbage.h:27, randomizer.h:44-50), so the expectation is a MODEL: the oracle, stepped one env-step
at a time, plus the rule of the header, written here with nothing taken from the engine.  After a step a game is OVER CAPACITY if
one of its boards has piece_draws >= 624 * limit or fifo_len > 8 on the oracle.  (The queue cases run at 10 ms per step for fewer
than 100 steps, no packet's 1000 ms run out: more than 8 pending after a step means the ninth arrived in that step.)  For such a
game the model expects done = 1 in that step, TETRIS_ERR_STREAM on every board of the game, TETRIS_ERR_FIFO on the boards whose
queue was full and only there, lines and dead as the oracle has them for the step; without auto-reset the game stays round-over,
later steps leave it alone and after a reset with the same seeds on both sides it equals the oracle again; with auto-reset the model
resets it with episode_seed(game, episode + 1), bumps the carried episode array and counts one episode.  Every other game is compared
with engines.assert_same_state after EVERY call; take_errors() must give exactly the bits of the games that went over in the call,
and 0 when asked again.  Every comparison is exact equality.

The draw limit is lowered per batch with tetris_debug_table_limit (the real one needs 2.6 GB of tables): limit 1 = 624 draws.  On the
GPU the limit is at most 3, below the tables' allocated capacity (2 chunks at creation, 4 or more once there is a third), so a wrong
index reads resident memory; the limit at the end of the allocation runs under ASan on the CPU (tests/sanitizers/capacity_main.cpp).

Inputs (each test asserts its own conditions on the oracle alone before it looks at the engine): O pieces only; a pool of 8 games,
each player in turn playing rot 0, trans 2 * (k % 5), 612 steps of 400 ms: every board at piece_draws 614, nobody dead, queues
empty; for the queue, player 0 alone playing that for 35 (P = 2), 64 (3) or 80 (4) steps of 10 ms: 8 packets pending on every other
board.  A batch is half such games (the even indices, tiled from the pool) and half fresh ones; at least 90 % of the prepared half
goes over capacity within the test's 16 steps at most, no fresh game does, and not every prepared game has gone over after the first
call.

The oracle-only census (every test prints its own line): games over capacity / not, of 1 100 on the GPU (333 on the harness: 167 /
166, the same steps), and the step of the first one.  Draw limit, every path: 550 / 550, step 9 — but the random rollout of one
player, 549 / 551 (one prepared game dies first).  Queue: step_rt P = 2 and the _dev / observe forms 549 / 551, step 8; P = 3 550 /
550, step 5; P = 4 550 / 550, step 13; list steps 550 / 550, step 8; evaluation steps 548 / 552, step 8; the rollouts 549 / 551,
step 8.  Limit 3: 550 / 550, step 9, tables 2 -> 3 chunks.

What these tests found in the engine, all fixed with them: a fused rollout launch kept ST_STREAM_EXHAUSTED for the rest of the launch
and ended the reset game again in every further step (3 episodes counted for 1); one-player kernels zeroed the board's error bit at
the first load after the step that set it; a simulation's overflow was reported by take_errors; split batches never ended a game at
the draw limit.  (A candidate that is none: every live board is dealt a piece in every step, so the group of draws a step reads
ahead at piece_draws % 8 == 7 is the group that step consumes.)"""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import engines
from tests import policy_model
from tests.buffers import Buf
from tests.plan_support import _device_lists
from tests.policy_model import W_A
from tests.seeded import _assert_path, _set_path
from tests.traj_support import GaeWindow

ERR_FIFO, ERR_STREAM, ERR_CHAIN_FELL_BACK = 1, 2, 4
CHUNK, QUEUE = 624, 8
N_CPU, N_GPU = 333, 1100      # as tests/test_chain_midgame.py: ragged last waves, 35 k_duo waves, 24 XCD-affine workgroups
POOL = 8
STEPS = 16
QUEUE_PREP = {2: 35, 3: 64, 4: 80}


def _n(kind):
    return N_GPU if kind == "hip" else N_CPU


def _pool_seeds(n):
    return orc.episode_seed(np.arange(n), 0)


def rt_keys(rot, trans, player, P, K=16):
    """(r, t) for `player`, [0] for the others, as key lists (sventon_utils.py:9-13) -> keys [n, P, K], lens [n, P]"""
    n = len(rot)
    keys, lens = np.zeros((n, P, K), np.uint8), np.ones((n, P), np.uint8)
    pl = np.broadcast_to(np.asarray(player), (n,))
    for g in range(n):
        k = [8] * int(rot[g]) + [2] + [3] * int(trans[g]) + [7]
        keys[g, pl[g], :len(k)] = k
        lens[g, pl[g]] = len(k)
    return keys, lens


# ---------------------------------------------------------------- the prepared pools (oracle) and the batches
@functools.lru_cache(maxsize=None)
def _prep(case, P, limit=1):
    """-> the oracle pool, its actions [(rot, trans, player)], ms per step"""
    pool = engines.make("oracle", POOL, P, pieces=(6,), seeds=_pool_seeds(POOL))
    rot, actions = np.zeros(POOL, np.uint8), []
    if case == "draws":
        ms, steps = 400, CHUNK * limit - 12                       # 612 (1860 at limit 3): two draws at the reset, one per step
        turns = [(s % P, (s // P) % 5) for s in range(steps)]
    else:
        ms, steps = 10, QUEUE_PREP[P]
        turns = [(0, s % 5) for s in range(steps)]
    for player, k in turns:
        trans = np.full(POOL, 2 * k, np.uint8)
        assert not pool.step_rt(rot, trans, player, ms=ms).any(), "a pool game ended during the preparation"
        actions.append((rot, trans, player))
    rec = pool.observe()[0]
    assert not rec["dead"].any()
    if case == "draws":
        assert (rec["piece_draws"] == CHUNK * limit - 10).all() and not rec["fifo_len"].any()
    else:
        assert (rec["fifo_len"][:, 1:] == QUEUE).all() and not rec["fifo_len"][:, 0].any() and rec["piece_draws"].max() < 100
    return pool, tuple(actions), ms


def _batch(kind, P, case, limit=1, n=None):
    """-> engine batch, oracle batch (equal), the prepared games' indices, ms per step"""
    n = _n(kind) if n is None else n
    pool_ref, actions, ms = _prep(case, P, limit)
    pool_eng = engines.make(kind, POOL, P, pieces=(6,), seeds=_pool_seeds(POOL))
    if case == "draws":
        pool_eng.debug_table_limit(limit)
    for s, (r, t, player) in enumerate(actions):
        assert not pool_eng.step_rt(r, t, player, ms=ms).any(), f"preparation step {s}"
    assert pool_eng.take_errors() == 0, "the preparation itself raised a capacity error"
    engines.assert_same_state(pool_eng, pool_ref, where="the pool after the preparation")
    eng = engines.make(kind, n, P, pieces=(6,), seeds=_pool_seeds(n))
    ref = engines.make("oracle", n, P, pieces=(6,), seeds=_pool_seeds(n))
    if case == "draws":
        eng.debug_table_limit(limit)
    prepared = np.arange(0, n, 2, dtype=np.int32)
    src = ((prepared // 2) % POOL).astype(np.int32)
    ref.copy_from(pool_ref, dst_idx=prepared, src_idx=src)
    eng.restore(pool_eng.snapshot(src), idx=prepared)
    pool_eng.close()
    engines.assert_same_state(eng, ref, where="the batch before the first step")
    return eng, ref, prepared, ms


# ---------------------------------------------------------------- the model
class Model:
    """The oracle plus the header's capacity rule.  auto: finished games are reset by the built-in seed schedule."""

    def __init__(self, ref, prepared, limit=1, auto=False, ms=400):
        self.ref, self.limit, self.auto, self.ms = ref, limit, auto, ms
        n, P = ref.n_games, ref.n_players
        self.prepared = np.zeros(n, bool)
        self.prepared[prepared] = True
        self.episode = np.zeros(n, np.uint32)
        self.ended = np.zeros(n, bool)             # over capacity and not reset since
        self.bits = np.zeros((n, P), np.uint8)     # tetris_record.fifo_overflow of the ended games
        self.ever = np.zeros(n, bool)
        # Reset after its ninth packet was dropped, and not stepped since: State.inc_count is refreshed by a step, not by a reset
        # (the reference's, the oracle's and the engine's alike), so until then it shows the queue as the step before the reset
        # left it — nine packets on the oracle, eight here.  The one field that is not compared for these games.
        self.stale = np.zeros(n, bool)
        self.step = self.calls = 0
        self.first_over = self.short_after_first_call = None
        self.total = np.zeros(4, np.uint64)

    def _over(self, live):
        rec = self.ref.observe()[0]
        draws = (rec["piece_draws"] >= CHUNK * self.limit).any(axis=1)
        full = rec["fifo_len"] > QUEUE
        over = (draws | full.any(axis=1)) & live
        bits = (np.where(draws[:, None], ERR_STREAM, 0) | np.where(full, ERR_FIFO, 0)).astype(np.uint8)
        if over.any() and self.first_over is None:
            self.first_over = self.step
        self.ever |= over
        return over, bits, rec

    def _reset_by_schedule(self, idx):
        self.episode[idx] += 1
        self.ref.reset(idx, seeds=orc.episode_seed(idx, self.episode[idx]))

    def play(self, keys, lens):
        """One step of key lists.  -> done, lines [n, P], dead [n, P] (before a reset), the games compared in this step, the
        bits take_errors owes"""
        live = ~self.ended
        self.stale[:] = False
        sent0 = self.ref.observe()[0]["lines_sent"].astype(np.int64).sum(axis=1)
        self.ref.make_actions(keys, lens)
        d = self.ref.finish_actions(self.ms) > 0
        over, bits, rec = self._over(live)
        sent = (rec["lines_sent"].astype(np.int64).sum(axis=1) - sent0) & 0xFFFF
        # what a built-in rollout counts for this step (auto-reset, so every game is live): env-steps, episodes, lines of the
        # players alive after it, lines sent — the oracle's numbers for the step, also for a game the step ends by capacity
        self.counted = np.array([len(d), int((d | over).sum()), int((rec["reward"].astype(np.int64) * (rec["dead"] == 0)).sum()),
                                 int(sent.sum())], np.uint64)
        self.bits[over] = bits[over]
        raised = int(np.bitwise_or.reduce(bits[over].ravel())) if over.any() else 0
        done = d | over | self.ended
        self.ended |= over
        self.step += 1
        if self.auto:
            idx = np.nonzero(done)[0].astype(np.int32)
            if len(idx):
                self._reset_by_schedule(idx)
            self.stale = over & ((bits & ERR_FIFO) > 0).any(axis=1)
            self.ended[:] = False
        return done.astype(np.uint8), rec["reward"].copy(), rec["dead"].copy(), live, raised

    def roll(self, steps):
        """`steps` steps of the built-in random rollout -> its counters, the bits take_errors owes"""
        c, raised = np.zeros(4, np.uint64), 0
        for _ in range(steps):
            self.episode, one = self.ref.rollout_random(1, first_step=self.step, ms=self.ms, episode=self.episode)
            over, bits, _ = self._over(np.ones(len(self.ended), bool))
            self.stale = over & ((bits & ERR_FIFO) > 0).any(axis=1)
            self.step += 1
            idx = np.nonzero(over)[0].astype(np.int32)
            if len(idx):
                raised |= int(np.bitwise_or.reduce(bits[over].ravel()))
                self._reset_by_schedule(idx)
                one[1] += np.uint64(len(idx))
            c += one
        self.total += c
        return c, raised

    def end_of_call(self):
        self.calls += 1
        if self.calls == 1:
            self.short_after_first_call = int((self.prepared & ~self.ever).sum())

    def assert_conditions(self, label):
        """the test's inputs did what they are there for (the oracle alone)"""
        p = self.prepared
        print(f"census {label}: {int(self.ever.sum())} games over capacity ({int(self.ever[p].sum())} of {int(p.sum())} prepared), "
              f"{int((~self.ever).sum())} not, first in step {self.first_over}; prepared games short of it after the first call: "
              f"{self.short_after_first_call}")
        assert self.ever[p].sum() >= 0.9 * p.sum(), "fewer than 90 % of the prepared games went over capacity"
        assert not self.ever[~p].any(), "a fresh game went over capacity"
        assert self.short_after_first_call >= 1, "every prepared game was over capacity after the first call"


def _same_state(eng, m, where, idx=None):
    """engines.assert_same_state of the games `idx` (all), but State.inc_count of the model's stale games"""
    stale = m.stale if idx is None else m.stale[idx]
    if not stale.any():
        return engines.assert_same_state(eng, m.ref, idx=idx, where=where)
    all_idx = np.arange(eng.n_games, dtype=np.int32) if idx is None else idx
    engines.assert_same_state(eng, m.ref, idx=all_idx[~stale], where=where)
    a, ro_a, lw_a = eng.observe(all_idx[stale])
    b, ro_b, lw_b = m.ref.observe(all_idx[stale])
    for f in engines.ENGINE_FIELDS:
        if f != "inc_count":
            assert np.array_equal(a[f] > 0, b[f] > 0) if f == "field" else np.array_equal(a[f], b[f]), f"{where}: '{f}' of a game reset after TETRIS_ERR_FIFO"
    assert np.array_equal(ro_a, ro_b) and np.array_equal(lw_a, lw_b), f"{where}: round_over / last_winner of a game reset after TETRIS_ERR_FIFO"


def _errors(eng, want, where):
    got = eng.take_errors()
    assert not got & ERR_CHAIN_FELL_BACK, f"{where}: a chained call fell back"
    assert got == want, f"{where}: take_errors {got}, the model's {want}"
    assert eng.take_errors() == 0, f"{where}: the bits were reported twice"


class Watch:
    """Compares an engine batch with the model after every call of a step path without auto-reset."""

    def __init__(self, eng, m):
        self.eng, self.m, self.frozen = eng, m, {}

    def after_step(self, got, want, where):
        eng, m = self.eng, self.m
        done, lines, dead = got
        wdone, wlines, wdead, live, raised = want
        assert np.array_equal(done, wdone), f"{where}: done differs in games {np.nonzero(done != wdone)[0][:8]}"
        assert np.array_equal(lines[live], wlines[live]), f"{where}: lines"
        assert np.array_equal(dead[live], wdead[live]), f"{where}: dead"
        _errors(eng, raised, where)
        rec, ro, _ = eng.observe()
        ok = np.nonzero(~m.ended)[0].astype(np.int32)
        _same_state(eng, m, where, idx=ok)
        assert not rec["fifo_overflow"][~m.ended].any(), f"{where}: an error bit on a game that is not over capacity"
        if not m.auto:
            assert np.array_equal(rec["fifo_overflow"][m.ended], m.bits[m.ended]), f"{where}: the error bits of the ended games"
            assert ro[m.ended].all(), f"{where}: an ended game is not round-over"
            for g in np.nonzero(m.ended)[0]:
                blob = eng.snapshot(np.array([g], np.int32))
                if g in self.frozen:
                    assert np.array_equal(blob, self.frozen[g]), f"{where}: a step changed game {g}, ended by capacity earlier"
                self.frozen[g] = blob
            idx = np.nonzero((wdone > 0) & ~m.ended)[0].astype(np.int32)      # ordinary game-overs: reset on both sides
            if len(idx):
                sd = orc.episode_seed(idx, 1000 + m.step)
                eng.reset(idx, seeds=sd)
                m.ref.reset(idx, seeds=sd)
        m.end_of_call()

    def finish(self, label):
        """the ended games, reset with the same seeds on both sides, equal the oracle again from their next step on (a reset does
        not refresh State.reward, inc_count and combo_time: they show the last step, which was not the oracle's)"""
        eng, m = self.eng, self.m
        m.assert_conditions(label)
        idx = np.nonzero(m.ended)[0].astype(np.int32)
        if len(idx):
            sd = orc.episode_seed(idx, 77)
            eng.reset(idx, seeds=sd)
            m.ref.reset(idx, seeds=sd)
            m.ended[:] = False
        n, P = eng.n_games, eng.n_players
        rot, trans = np.zeros(n, np.uint8), np.full(n, 4, np.uint8)
        assert np.array_equal(eng.step_rt(rot, trans, 0, ms=m.ms), m.ref.step_rt(rot, trans, 0, ms=m.ms))
        engines.assert_same_state(eng, m.ref, where=f"{label}: one step after the reset")
        _errors(eng, 0, label)


def _random_rt(rng, n, P, s, case="draws", phase=None):
    """Random (r, t), the players taking turns.  In the queue cases of three and four players player 0 moves in every step and
    lays its O pieces side by side from a random place of its own per game (`phase`): only its clears fill the other boards'
    queues, and each sends them half or a third of a line — with uniform t and a move in three or four, fewer than 90 % of the
    games see a ninth packet within 16 steps (489 of 550 on the oracle).  In any one step some games clear rows and others do not."""
    rot = rng.integers(0, 4, n).astype(np.uint8)
    if case == "queue" and P > 2:
        return rot, (2 * ((s + phase) % 5)).astype(np.uint8), 0
    return rot, rng.integers(0, 10, n).astype(np.uint8), s % P


# ---------------------------------------------------------------- 1. + 2. the synchronous entry points
def _sync_step(eng, path, rot, trans, player, keys, lens, ms):
    if path == "step_rt":
        return eng.step_rt(rot, trans, player, ms=ms, full=True)
    if path == "step_keys":
        return eng.step_keys(keys, lens, ms=ms)
    eng.make_actions(keys, lens)
    return eng.finish_actions(ms, full=True)


SYNC = ([("step_keys", "draws", 1), ("step_keys", "draws", 2), ("make_finish", "draws", 1), ("make_finish", "draws", 2)]
        + [("step_rt", "draws", P) for P in (1, 2, 3)] + [("step_rt", "queue", P) for P in (2, 3, 4)])


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("path,case,P", SYNC)
def test_synchronous_steps(kind, path, case, P):
    """step_rt, step_keys and make_actions + finish_actions with random (r, t): some games clear rows in the step that ends
    them, others do not."""
    eng, ref, prepared, ms = _batch(kind, P, case)
    m, rng = Model(ref, prepared, ms=ms), np.random.default_rng(7 * P + len(path))
    w, phase = Watch(eng, m), rng.integers(0, 5, eng.n_games)
    for s in range(STEPS):
        rot, trans, player = _random_rt(rng, eng.n_games, P, s, case, phase)
        keys, lens = rt_keys(rot, trans, player, P)
        got = _sync_step(eng, path, rot, trans, player, keys, lens, ms)
        w.after_step(got, m.play(keys, lens), f"{path} {case} P={P}, step {s}")
    w.finish(f"{path} {case} P={P}")


# ---------------------------------------------------------------- 3. the device-pointer steps
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("case", ["draws", "queue"])
@pytest.mark.parametrize("path", ["dev", "dev_auto", "observe", "observe_auto"])
def test_device_steps(kind, path, case):
    """step_rt_dev with and without auto-reset and step_rt_observe_dev, two players (k_duo on the GPU); the observation shows
    the game as it ended or, with auto-reset, as it was reset."""
    P = 2
    eng, ref, prepared, ms = _batch(kind, P, case)
    n, H = eng.n_games, eng.height
    auto = path.endswith("auto")
    m, rng = Model(ref, prepared, auto=auto, ms=ms), np.random.default_rng(31)
    w = Watch(eng, m)
    d_rot, d_trans, d_pl, d_next = (Buf.full(kind, (n,), np.uint8) for _ in range(4))
    d_done, d_lines, d_dead = Buf.full(kind, (n,), np.uint8), Buf.full(kind, (P, n), np.uint8), Buf.full(kind, (P, n), np.uint8)
    vis, vec, pc = Buf.full(kind, (P, n, H, 10), np.uint8), Buf.full(kind, (P, n, 12), np.uint8), Buf.full(kind, (P, n), np.uint8)
    for s in range(STEPS):
        rot, trans, player = _random_rt(rng, n, P, s)
        keys, lens = rt_keys(rot, trans, player, P)
        d_rot.put(rot), d_trans.put(trans), d_pl.put(player), d_next.put((s + 1) % P)
        if path.startswith("observe"):
            eng.step_rt_observe_dev(d_rot.ptr, d_trans.ptr, d_pl.ptr, d_done.ptr, d_lines.ptr, d_dead.ptr, d_next.ptr, vis.ptr, vec.ptr,
                                    pc.ptr, ms=ms, auto_reset=auto)
        else:
            eng.step_rt_dev(d_rot.ptr, d_trans.ptr, d_pl.ptr, d_done.ptr, d_lines.ptr, d_dead.ptr, ms=ms, auto_reset=auto)
        eng.sync()
        got = (d_done.get(), d_lines.get().T, d_dead.get().T)
        where = f"{path} {case}, step {s}"
        if path.startswith("observe"):
            v2, c2, p2 = eng.observe_packed(player=np.full(n, (s + 1) % P, np.uint8))
            assert np.array_equal(vis.get(), v2) and np.array_equal(vec.get(), c2) and np.array_equal(pc.get(), p2), f"{where}: observation"
        w.after_step(got, m.play(keys, lens), where)
    if auto:
        m.assert_conditions(f"{path} {case}")
    else:
        w.finish(f"{path} {case}")


# ---------------------------------------------------------------- 7. the built-in random rollout
def _rollout_calls(eng, m, calls, S, label, check_path=None, launches=1, last=True):
    for k in range(calls):
        c, _ = eng.rollout_random(launches, S, first_step=m.step, ms=m.ms)
        want, raised = m.roll(launches * S)
        where = f"{label}, call {k}"
        assert c.tolist() == want.tolist(), f"{where}: counters {c.tolist()}, the model's {want.tolist()}"
        if check_path:
            check_path()
        _same_state(eng, m, where)
        assert not eng.observe()[0]["fifo_overflow"].any(), where
        _errors(eng, raised, where)
        m.end_of_call()
    if last:
        assert eng.rollout_totals().tolist() == m.total.tolist(), f"{label}: the per-game counter words"
        m.assert_conditions(label)


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("case,P", [("draws", 1), ("draws", 2), ("queue", 2)])
@pytest.mark.parametrize("S", [1, 4])
def test_rollout_unchained(kind, S, case, P):
    """rollout_random, un-chained, one launch per call of S = 1 and S = 4 steps: a game ended by capacity inside a fused launch
    is reset and plays on in the same launch."""
    eng, ref, prepared, ms = _batch(kind, P, case)
    eng.set_chained(False)
    _rollout_calls(eng, Model(ref, prepared, auto=True, ms=ms), STEPS // S, S, f"rollout un-chained S={S} {case} P={P}")


CHAINED = ([(path, 1, S, "draws") for path in ("streams", "queues", "queues_affine", "unchained") for S in (1, 3)]
           + [(path, 2, 1, case) for path in ("streams", "queues", "queues_affine", "unchained") for case in ("draws", "queue")])


@pytest.mark.gpu
@pytest.mark.parametrize("path,P,S,case", CHAINED)
def test_gpu_rollout_paths(path, P, S, case):
    """The chained kernels (k_chain, k_chain_affine, k_chain_fused, k_chain_fused_affine, the chained k_duo forms) and the
    un-chained control: their death path ends a game by capacity exactly as finish_game does, and the W_FIFO_* rows they load and
    store conditionally hold a full queue.  Counters, full state, error bits and the launch path after every call."""
    eng, ref, prepared, ms = _batch("hip", P, case)
    _set_path(eng, path)
    m = Model(ref, prepared, auto=True, ms=ms)
    for k, launches in enumerate((4, 4, 4, 4) if S == 1 else (2, 2, 1)):
        _rollout_calls(eng, m, 1, S, f"{path} S={S} {case} P={P}, {launches} launches ({k})", lambda: _assert_path(eng, path), launches=launches,
                       last=False)
    assert eng.rollout_totals().tolist() == m.total.tolist()
    m.assert_conditions(f"{path} S={S} {case} P={P}")
    assert eng.rollout_is_chained(S) == (path != "unchained")


@pytest.mark.parametrize("kind,path", [pytest.param("harness", None, id="harness"), pytest.param("hip", "streams", marks=pytest.mark.gpu, id="streams"),
                                       pytest.param("hip", "queues_affine", marks=pytest.mark.gpu, id="queues_affine")])
def test_rollout_at_a_limit_of_three_chunks(kind, path):
    """Limit 3 from boards at draw 1862: where the process's tables still have two chunks the request to extend is granted up to
    the limit and refused from there on; the games end at draw 1872."""
    probe = engines.make(kind, 8, 1, pieces=(6,))
    before = probe.table_chunks
    probe.close()
    eng, ref, prepared, ms = _batch(kind, 1, "draws", limit=3)
    if path:
        _set_path(eng, path)
    m = Model(ref, prepared, limit=3, auto=True, ms=ms)
    for k in range(4):
        _rollout_calls(eng, m, 1, 1, f"limit 3, {path or kind}, call {k}", (lambda: _assert_path(eng, path)) if path else None, launches=4, last=False)
    m.assert_conditions(f"limit 3, {path or kind}")
    print(f"table_chunks {before} -> {eng.table_chunks}")
    assert eng.table_chunks >= 3
    if before <= 3:
        assert eng.table_chunks == 3, "the tables grew past the batch's limit"


# ---------------------------------------------------------------- 4. planning: list steps and simulations
def _simulated_model(m, cnt, ln, kk, player):
    """every list of every game on a scratch oracle: -> done [L, n] as the model expects it of a finalized simulation"""
    ref, n, P = m.ref, m.ref.n_games, m.ref.n_players
    L = int(max(1, cnt.max()))
    scratch = orc.OracleBatch(n * L, P, ref.height, 10, pieces=(6,))
    scratch.copy_from(ref, src_idx=np.repeat(np.arange(n), L).astype(np.int32))
    keys, lens = np.zeros((n * L, P, kk.shape[2]), np.uint8), np.ones((n * L, P), np.uint8)
    g, k = np.repeat(np.arange(n), L), np.tile(np.arange(L), n)
    kc = np.minimum(k, np.maximum(cnt[g], 1) - 1)
    keys[np.arange(n * L), player] = kk[g, kc]
    lens[np.arange(n * L), player] = ln[g, kc]
    scratch.make_actions(keys, lens)
    d = scratch.finish_actions(m.ms) > 0
    rec = scratch.observe()[0]
    over = (rec["piece_draws"] >= CHUNK * m.limit).any(axis=1) | (rec["fifo_len"] > QUEUE).any(axis=1)
    return (d | over).reshape(n, L).T, over.reshape(n, L).T


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("case", ["draws", "queue"])
@pytest.mark.parametrize("auto", [False, True])
def test_list_steps_and_simulations(kind, case, auto):
    """step_lists_dev with and without auto-reset, and before every step the finalized simulation of all lists: done = 1 for the
    lists that take their game over capacity, the batch's state unchanged and take_errors() == 0 — no game of the batch was ended
    by a simulation."""
    P, L, K = 2, 64, 48
    eng, ref, prepared, ms = _batch(kind, P, case)
    n = eng.n_games
    m, rng = Model(ref, prepared, auto=auto, ms=ms), np.random.default_rng(5)
    w, simulated_over = Watch(eng, m), 0
    for s in range(STEPS):
        player = s % P
        cnt, lens, keys, pl = _device_lists(kind, eng, np.full(n, player), False, L=L, K=K)
        c, ln, kk = cnt.get(), lens.get(), keys.get()
        live = ~m.ended
        assert (c[live] >= 1).all() and (c <= L).all()
        before = eng.snapshot()
        cols, d_done = Buf.full(kind, (L, P, 10, n), np.uint32), Buf.full(kind, (L, n), np.uint8, 77)
        eng.simulate_lists_dev(cnt.ptr, lens.ptr, keys.ptr, cols.ptr, max_lists=L, max_keys=K, player=pl.ptr, finalize=True, ms=ms, done=d_done.ptr)
        eng.sync()
        want, over = _simulated_model(m, c, ln, kk, player)
        got = d_done.get()
        for k in range(want.shape[0]):
            sel = live & (k < c)
            assert np.array_equal(got[k][sel], want[k][sel].astype(np.uint8)), f"{case}, step {s}: simulated done of list {k}"
            simulated_over += int(over[k][sel].sum())
        assert np.array_equal(eng.snapshot(), before), f"{case}, step {s}: the simulation wrote the batch's state"
        assert eng.take_errors() == 0, f"{case}, step {s}: a simulation reported a game ended by capacity"
        choice = rng.integers(0, 1 << 20, n) % np.maximum(c, 1)
        ch = Buf.full(kind, (n,), np.int32)
        ch.put(choice.astype(np.int32))
        done, lines, dead = Buf.full(kind, (n,), np.uint8), Buf.full(kind, (P, n), np.uint8), Buf.full(kind, (P, n), np.uint8)
        eng.step_lists_dev(ch.ptr, cnt.ptr, lens.ptr, keys.ptr, done.ptr, lines.ptr, dead.ptr, max_lists=L, max_keys=K, player=pl.ptr, ms=ms,
                           auto_reset=auto)
        eng.sync()
        keys_h, lens_h = np.zeros((n, P, K), np.uint8), np.ones((n, P), np.uint8)
        keys_h[np.arange(n), player] = kk[np.arange(n), choice]
        lens_h[np.arange(n), player] = np.where(c >= 1, ln[np.arange(n), choice], 1)
        w.after_step((done.get(), lines.get().T, dead.get().T), m.play(keys_h, lens_h), f"step_lists {case} auto={auto}, step {s}")
    assert simulated_over > 0, "no simulated list took a game over capacity"
    if auto:
        m.assert_conditions(f"step_lists {case} auto")
    else:
        w.finish(f"step_lists {case}")


# ---------------------------------------------------------------- 5. the heuristic policy
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("path", ["step", "rollout_1", "rollout_4"])
def test_policy_steps_and_rollouts(kind, path):
    """step_policy_dev with auto-reset and rollout_policy at one and four steps per launch, one player: the policy does not die,
    so its episodes are ended by exactly this limit.  The choice comes from tests.policy_model.Model on the oracle."""
    steps = 12
    eng, ref, prepared, ms = _batch(kind, 1, "draws")
    n = eng.n_games
    m, pm = Model(ref, prepared, auto=True, ms=ms), policy_model.Model(ref)
    w = Watch(eng, m)
    wt = Buf.full(kind, (8,), np.int16).put(W_A)
    done, lines, dead = Buf.full(kind, (n,), np.uint8), Buf.full(kind, (1, n), np.uint8), Buf.full(kind, (1, n), np.uint8)
    rot, trans = Buf.full(kind, (n,), np.uint8), Buf.full(kind, (n,), np.uint8)
    S = 1 if path == "step" else int(path[-1])
    for call in range(steps // S):
        total, raised, first = np.zeros(4, np.uint64), 0, None
        for s in range(S):
            r, t, _ = pm.choose(W_A, 0)
            want = m.play(*rt_keys(r, t, 0, 1))
            total, raised, first = total + m.counted, raised | want[4], first or (r, t, want)
        where = f"policy {path}, call {call}"
        if path == "step":
            eng.step_policy_dev(wt.ptr, done.ptr, lines.ptr, dead.ptr, rot=rot.ptr, trans=trans.ptr, ms=ms, auto_reset=True)
            eng.sync()
            assert np.array_equal(rot.get(), first[0]) and np.array_equal(trans.get(), first[1]), f"{where}: the choice"
            w.after_step((done.get(), lines.get().T, dead.get().T), first[2], where)
        else:
            c, _ = eng.rollout_policy(wt.ptr, 1, S, first_step=call * S, ms=ms)
            assert c.tolist() == total.tolist(), f"{where}: counters {c.tolist()}, the model's {total.tolist()}"
            m.total += total
            _same_state(eng, m, where)
            _errors(eng, raised, where)
            m.end_of_call()
    if path != "step":
        assert eng.rollout_totals().tolist() == m.total.tolist()
    m.assert_conditions(f"policy {path}")


# ---------------------------------------------------------------- 6. acting on an evaluation, and the trajectory row
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("case", ["draws", "queue"])
@pytest.mark.parametrize("observe", [False, True])
def test_eval_steps_and_the_recorded_row(kind, case, observe):
    """step_eval_dev / step_eval_observe_dev with random evaluations (argmax) and auto-reset, two players, then traj_record_dev of
    the row: a game ended by capacity is done = 1 with reward 0 unless somebody died in that very step — environment._reward on the
    copied outputs."""
    import importlib
    import types
    env = importlib.import_module("drl-tetris_amd.environment")
    P = 2
    reward_of = lambda done, dead, player: env.tetris_environment_vector._reward(types.SimpleNamespace(n_players=P), done, dead, player)    # noqa: E731
    eng, ref, prepared, ms = _batch(kind, P, case)
    n, H = eng.n_games, eng.height
    m, rng = Model(ref, prepared, auto=True, ms=ms), np.random.default_rng(17)
    w, win = Watch(eng, m), GaeWindow(kind, eng, STEPS, fill=7)
    u8 = lambda *shape: Buf(kind, np.zeros(shape, np.uint8))      # noqa: E731
    rot, trans, piece, done, lines, dead = u8(n), u8(n), u8(n), u8(n), u8(P, n), u8(P, n)
    ev = Buf(kind, np.zeros(n, np.float32))
    vis, vec, pc = u8(P, n, H, 10), u8(P, n, 12), u8(P, n)
    capacity_rows = 0
    for s in range(STEPS):
        player = np.full(n, s % P, np.uint8)
        ae, plb, nxt = Buf(kind, rng.random((n, 4, 10, 7)).astype(np.float32)), Buf(kind, player), Buf(kind, 1 - player)
        e = eng.act_eval(ae.ptr, rot.ptr, trans.ptr, n_pieces=7, mode="argmax", player=plb.ptr, piece=piece.ptr, eval=ev.ptr)
        if observe:
            eng.step_eval_observe_dev(e, done.ptr, lines.ptr, dead.ptr, nxt.ptr, vis.ptr, vec.ptr, pc.ptr, ms=ms, auto_reset=True)
        else:
            eng.step_eval_dev(e, done.ptr, lines.ptr, dead.ptr, ms=ms, auto_reset=True)
        eng.traj_record_dev(win.traj, s, e, done.ptr, dead.ptr)
        eng.sync()
        where = f"step_eval {case} observe={observe}, step {s}"
        if observe:
            v2, c2, p2 = eng.observe_packed(player=1 - player)
            assert np.array_equal(vis.get(), v2) and np.array_equal(vec.get(), c2) and np.array_equal(pc.get(), p2), f"{where}: observation"
        was_over = m.ever.copy()
        want = m.play(*rt_keys(rot.get(), trans.get(), s % P, P))
        got_done, got_dead = done.get(), dead.get()
        w.after_step((got_done, lines.get().T, got_dead.T), want, where)
        row_done, row_reward = win.done.get()[s], win.reward.get()[s]
        assert np.array_equal(row_done, got_done), f"{where}: the row's done"
        wr = np.array([reward_of(bool(got_done[i]), got_dead[:, i], int(player[i])) for i in range(n)], np.float32)
        assert np.array_equal(row_reward, wr), f"{where}: the row's reward"
        ended_now = m.ever & ~was_over
        assert row_done[ended_now].all() and not row_reward[ended_now & ~got_dead.any(axis=0)].any(), f"{where}: a capacity ending's row"
        capacity_rows += int(ended_now.sum())
    assert capacity_rows > 0
    m.assert_conditions(f"step_eval {case} observe={observe}")
