"""The heuristic policy's CPU model on top of the oracle, for every test that plays or checks it (tests/test_policy_device.py
describes it): the eight features, the choice, the step with the built-in reset schedule, the rollout and its totals."""
import numpy as np

from oracle import oracle as orc
from tests import engines
from tests.buffers import Buf

ROT = np.repeat(np.arange(4), 10).astype(np.uint8)
TRA = np.tile(np.arange(10), 4).astype(np.uint8)
W_A = np.array([76, -71, -18, -51, 0, 0, 0, 0], np.int16)          # lines, holes, bumpiness, aggregate height
W_B = np.array([34, -79, 0, -10, 0, -32, -93, -34], np.int16)      # Dellacherie-like
W_ZERO = np.zeros(8, np.int16)


# ---------------------------------------------------------------- the model
def features(f):
    """f bool [M, H, W] (row 0 = top) -> int32 [M, 8], the table of include/tetris_hip.h"""
    M, H, W = f.shape
    full = f.all(axis=2)
    lines = full.sum(axis=1)
    g = np.zeros_like(f)                              # full rows removed, the rows above moved down
    for m in range(M):
        keep = f[m][~full[m]]
        g[m, H - len(keep):] = keep
    heights = np.where(g.any(axis=1), H - g.argmax(axis=1), 0)
    below = np.cumsum(g, axis=1) > 0
    holes = (below & ~g).sum(axis=(1, 2))
    bump = np.abs(np.diff(heights, axis=1)).sum(axis=1)
    agg = heights.sum(axis=1)
    mx = heights.max(axis=1)
    padded = np.concatenate([np.ones((M, H, 1), bool), g, np.ones((M, H, 1), bool)], axis=2)
    rowtr = (padded[:, :, 1:] != padded[:, :, :-1]).sum(axis=(1, 2))
    padv = np.concatenate([g, np.ones((M, 1, W), bool)], axis=1)
    coltr = (padv[:, 1:] != padv[:, :-1]).sum(axis=(1, 2))
    hp = np.concatenate([np.full((M, 1), H), heights, np.full((M, 1), H)], axis=1)
    d = np.maximum(np.minimum(hp[:, :-2], hp[:, 2:]) - heights, 0)
    wells = (d * (d + 1) // 2).sum(axis=1)
    return np.stack([lines, holes, bump, agg, mx, rowtr, coltr, wells], axis=1).astype(np.int32)


class Model:
    """The policy on the oracle.  `o` is the OracleBatch it plays; weights int16 [8] or [N, 8]; ms = game time per step."""

    def __init__(self, o, ids=None, ms=400):
        self.o, self.ms = o, ms
        self.ids = np.arange(o.n_games) if ids is None else np.asarray(ids)      # global game ids (the reset-seed schedule's key)
        self.scratch = orc.OracleBatch(40 * o.n_games, o.n_players, o.height, 10)
        self.episode = np.zeros(o.n_games, np.int64)
        self.totals = np.zeros((4, o.n_games), np.int64)     # env-steps, episodes, lines, sent
        self.decisions = self.tied = 0

    def candidate_fields(self, player):
        o, N, P, H = self.o, self.o.n_games, self.o.n_players, self.o.height
        self.scratch.copy_from(o, src_idx=np.repeat(np.arange(N), 40).astype(np.int32))
        keys = np.zeros((40 * N, P, 16), np.uint8)
        lens = np.ones((40 * N, P), np.uint8)              # [0] for the others
        pl = np.broadcast_to(np.asarray(player, np.int64), (N,))
        for c in range(40):
            k = [8] * int(ROT[c]) + [2] + [3] * int(TRA[c]) + [7]
            sel = np.arange(N) * 40 + c
            keys[sel, pl, :len(k)] = k
            lens[sel, pl] = len(k)
        self.scratch.make_actions(keys, lens)
        rec, _, _ = self.scratch.observe()
        return rec["field"][np.arange(40 * N), np.repeat(pl, 40), :H, :]      # [40 N, H, W] tile values

    def features(self, player):
        """-> int32 [N, 40, 8]"""
        return features(self.candidate_fields(player) > 0).reshape(self.o.n_games, 40, 8)

    def choose(self, weights, player):
        """-> rot, trans, score [N]"""
        N = self.o.n_games
        w = np.broadcast_to(np.asarray(weights, np.int64).reshape(-1, 8), (N, 8))
        score = (self.features(player).astype(np.int64) * w[:, None, :]).sum(axis=2)        # [N, 40]
        best = score.argmax(axis=1)                       # lowest index on ties
        self.decisions += N
        self.tied += int(((score == score.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
        return ROT[best], TRA[best], score[np.arange(N), best].astype(np.int32)

    def step(self, rot, trans, player, auto_reset, count=False):
        """step_rt + the reset of finished games by the built-in seed schedule -> done, lines [N, P], dead [N, P] before the reset"""
        o = self.o
        sent0 = o.observe()[0]["lines_sent"].astype(np.int64).sum(axis=1) if count else None
        done = o.step_rt(rot, trans, player, ms=self.ms)
        rec = o.observe()[0]
        lines, dead = rec["reward"].copy(), rec["dead"].copy()
        if count:
            self.totals[0] += 1
            self.totals[2] += (lines.astype(np.int64) * (dead == 0)).sum(axis=1)
            self.totals[3] += (rec["lines_sent"].astype(np.int64).sum(axis=1) - sent0) & 0xFFFF
        d = np.nonzero(done)[0].astype(np.int32)
        if auto_reset and len(d):
            self.episode[d] += 1
            self.totals[1][d] += 1
            o.reset(d, seeds=orc.episode_seed(self.ids[d], self.episode[d]))
        return done, lines, dead

    def rollout(self, weights, steps, first_step=0):
        P = self.o.n_players
        for s in range(first_step, first_step + steps):
            r, t, _ = self.choose(weights, s % P)
            self.step(r, t, s % P, True, count=True)


def _assert_rollout(kind, b, m, counters, label):
    engines.assert_same_state(b, m.o, where=label)
    n = m.o.n_games
    tot = Buf.full(kind, (4, n), np.uint32, 0xFFFF)
    b.rollout_game_totals_dev(tot.ptr)
    b.sync()
    assert np.array_equal(tot.get().astype(np.int64), m.totals), f"{label}: per-game totals"
    assert np.array_equal(b.rollout_totals().astype(np.int64), m.totals.sum(axis=1)), f"{label}: rollout_totals"
    assert np.array_equal(np.asarray(counters, np.int64), m.totals.sum(axis=1)), f"{label}: counters"
