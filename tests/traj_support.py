"""What the trajectory tests share: the GAE model written from the header's definition and the window of value / reward / done
arrays it runs on (tests/test_traj_device.py), the window with observation records, the numpy expansion of a minibatch and the
played boards (tests/test_traj_batch.py)."""
import numpy as np

from oracle import oracle as orc
from tests import engines
from tests.buffers import Buf
from tests.seeded import POOL, _heuristic_play

F32, U32, U8, I32 = np.float32, np.uint32, np.uint8, np.int32
PIECE_SWAP = np.array([1, 0, 3, 2, 4, 5, 6, 7], U8)           # the header's piece_swap, 7 stays 7


# ---------------------------------------------------------------- the GAE model
def model(value, reward, done, rows, gamma, lambda_adv, lambda_value, boot=None):
    """value float32 [2, T, n], reward float32 [T, n], done [T, n] -> adv, target float32 [rows, n], closed uint8 [rows, n]: the
    header's recurrence, one row at a time, all games of a row side by side (elementwise float32 operations round as the
    scalar ones do)."""
    n = reward.shape[1]
    g, la, lv = F32(gamma), F32(lambda_adv), F32(lambda_value)
    gla, glv = F32(g * la), F32(g * lv)
    zero, one = F32(0.0), F32(1.0)
    A1, A2, W1, W2 = (np.zeros(n, F32) for _ in range(4))
    vnext = np.zeros(n, F32) if boot is None else boot.astype(F32).copy()
    seen = np.zeros(n, np.uint8)
    adv, target, closed = np.zeros((rows, n), F32), np.zeros((rows, n), F32), np.zeros((rows, n), np.uint8)
    with np.errstate(all="ignore"):
        for t in range(rows - 1, -1, -1):
            d = done[t] != 0
            A1, A2, W1, W2 = (np.where(d, zero, x).astype(F32) for x in (A1, A2, W1, W2))
            seen = np.where(d, 1, seen).astype(np.uint8)
            v0, v1 = value[0, t].astype(F32), value[1, t].astype(F32)
            boot_term = ((g * vnext).astype(F32) * np.where(d, zero, one).astype(F32)).astype(F32)
            td = ((reward[t].astype(F32) + boot_term).astype(F32) - v0).astype(F32)
            A1 = ((A1 * gla).astype(F32) + td).astype(F32)
            W1 = ((W1 * la).astype(F32) + one).astype(F32)
            A2 = ((A2 * glv).astype(F32) + td).astype(F32)
            W2 = ((W2 * lv).astype(F32) + one).astype(F32)
            adv[t] = (((A1 + v0).astype(F32) - v1).astype(F32) / W1).astype(F32)
            target[t] = (v1 + (((A2 + v0).astype(F32) - v1).astype(F32) / W2).astype(F32)).astype(F32)
            closed[t] = seen
            vnext = v0
    return adv, target, closed


class GaeWindow:
    """A window of T rows of the batch's games in buffers of the engine's kind, and the struct over them"""

    def __init__(self, kind, b, T, value=None, reward=None, done=None, fill=0):
        n = b.n_games
        self.T, self.n = T, n
        self.action = Buf(kind, np.full((T, n, 4), fill, np.uint8))
        self.prob = Buf(kind, np.full((T, n), fill, F32))
        self.value = Buf(kind, np.full((2, T, n), fill, F32) if value is None else value.astype(F32))
        self.reward = Buf(kind, np.full((T, n), fill, F32) if reward is None else reward.astype(F32))
        self.done = Buf(kind, np.full((T, n), fill, np.uint8) if done is None else done.astype(np.uint8))
        self.traj = b.traj(T, self.action.ptr, self.prob.ptr, self.value.ptr, self.reward.ptr, self.done.ptr)


class Window:
    """A window of T rows of the batch's games with its observation records, in buffers of the engine's kind"""

    def __init__(self, kind, b, T, rng=None):
        n, S = b.n_games, b.n_players
        self.kind, self.b, self.T, self.n, self.S = kind, b, T, n, S
        def rb(shape, dt):         # zeros, or distinct random bits
            if rng is None:
                return np.zeros(shape, dt)
            return rng.integers(0, 256, shape).astype(U8) if dt == U8 else rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(U32)

        obs, action = rb((T, n, S, 12), U32), rb((T, n, 4), U8)
        if rng is not None:       # words 10 / 11 as the header defines them: four bytes; combo_count, next 0..7, piece 0..7, zero
            obs[..., 11] = rng.integers(0, 256, (T, n, S)) | (rng.integers(0, 8, (T, n, S)) << 8) | (rng.integers(0, 8, (T, n, S)) << 16)
            action[..., 1] = rng.integers(0, 10, (T, n))
            action[..., 2] = rng.integers(0, 7, (T, n))
        self.obs, self.action = Buf(kind, obs), Buf(kind, action)
        self.prob, self.value, self.reward = Buf(kind, rb((T, n), U32)), Buf(kind, rb((2, T, n), U32)), Buf(kind, rb((T, n), U32))
        self.done = Buf(kind, rb((T, n), U8))
        self.adv, self.target = Buf(kind, rb((T, n), U32)), Buf(kind, rb((T, n), U32))
        self.traj = b.traj(T, self.action.ptr, self.prob.ptr, self.value.ptr, self.reward.ptr, self.done.ptr)
        self.tobs = b.traj_obs(T, self.obs.ptr)


OUTPUTS = ("visual", "vector", "piece", "action", "prob", "adv", "target", "reward", "done", "valid")


def out_shapes(S, M, H):
    return dict(visual=((S, M, H, 10), U8), vector=((S, M, 12), U8), piece=((S, M), U8), action=((M, 3), U8), prob=((M,), U32),
                adv=((M,), U32), target=((M,), U32), reward=((M,), U32), done=((M,), U8), valid=((M,), U8))


# ---------------------------------------------------------------- the model, from the header's text
def model_batch(obs, action, prob, reward, done, adv, target, index, H):
    """obs uint32 [T, N, S, 12], action uint8 [T, N, 4], prob / reward / adv / target uint32 [T, N] (adv, target or None), done
    uint8 [T, N]; index [M] -> the ten outputs (floats as uint32)"""
    T, N, S, _ = obs.shape
    e = np.asarray(index, np.int64).astype(U32)
    at, mir = (e & U32(0x7FFFFFFF)).astype(np.int64), (e >> 31) == 1
    valid = at < T * N
    at, mir = np.where(valid, at, 0), mir & valid
    M = len(e)
    rec = obs.reshape(T * N, S, 12)[at]                                            # [M, S, 12]
    cols = np.where(mir[:, None, None], rec[:, :, 9::-1], rec[:, :, :10])          # field column c is column 9 - c
    visual = ((cols[:, :, None, :] >> np.arange(H, dtype=U32)[None, None, :, None]) & 1).astype(U8)
    w10, w11 = rec[:, :, 10], rec[:, :, 11]
    vector = np.zeros((M, S, 12), U8)
    for k in range(4):
        vector[:, :, k] = (w10 >> (8 * k)) & 255                                    # x, y, inc_lines, combo_time
    vector[:, :, 4] = w11 & 255                                                     # combo_count
    hot = (((w11 >> 8) & 255)[:, :, None] == np.arange(7)[None, None, :]).astype(U8)
    vector[:, :, 5:] = np.where(mir[:, None, None], 1 - hot, hot)                   # piece_swap[int(p == next)]: the quirk
    piece = ((w11 >> 16) & 255).astype(U8)
    piece = np.where(mir[:, None], PIECE_SWAP[np.minimum(piece, 7)], piece)
    a = action.reshape(T * N, 4)[at]
    act = np.stack([a[:, 0], np.where(mir, 9 - a[:, 1].astype(np.int64), a[:, 1]).astype(U8), np.where(mir, PIECE_SWAP[np.minimum(a[:, 2], 7)], a[:, 2])], axis=1)
    z = lambda x: np.where(valid.reshape((M,) + (1,) * (x.ndim - 1)), x, 0).astype(x.dtype)          # noqa: E731
    flat = lambda x: np.zeros(M, U32) if x is None else z(x.reshape(T * N)[at])                      # noqa: E731
    return dict(visual=z(visual).transpose(1, 0, 2, 3), vector=z(vector).transpose(1, 0, 2), piece=z(piece).T, action=z(act),
                prob=flat(prob), adv=flat(adv), target=flat(target), reward=flat(reward), done=z(done.reshape(T * N)[at]),
                valid=valid.astype(U8))


def assert_outputs(got, want, where):
    for k, v in got.items():
        assert np.array_equal(v, want[k]), f"{where}: '{k}' differs at {np.argwhere(v != want[k])[:4].tolist()}"


def played(kind, n, P, H, colours, seed):
    """a batch after 30 (r, t) steps: 24 of the heuristic play of tests/seeded.py at 400 ms (lines, combos, garbage; game
    g starts as its pool game g % 32 and, at height 20, follows it), then 6 random ones with 10 ms and 400 ms ticks mixed;
    finished games are reset by the seed schedule"""
    rng = np.random.default_rng(seed)
    heur = _heuristic_play(P, 400)[:24]
    tile = np.arange(n) % POOL
    b = engines.make(kind, n, P, H, seeds=orc.episode_seed(tile, 0), colours=colours)
    episode = np.zeros(n, np.int64)
    for s in range(len(heur) + 6):
        if s < len(heur):
            rot, trans, player, ms = heur[s][0][tile], heur[s][1][tile], heur[s][2][tile], 400
        else:
            rot, trans, player = rng.integers(0, 4, n).astype(U8), rng.integers(0, 10, n).astype(U8), rng.integers(0, P, n).astype(U8)
            ms = (10, 400)[s % 2]
        done = b.step_rt(rot, trans, player, ms=ms)
        idx = np.nonzero(done)[0].astype(I32)
        if len(idx):
            episode[idx] += 1
            b.reset(idx, orc.episode_seed(idx % POOL, episode[idx]))
    return b, rng
