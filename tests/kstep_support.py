"""The k-step target estimator and the step-list gather (include/tetris_hip.h: tetris_kstep_target_dev,
tetris_replay_gather_steps_dev): a numpy model written from the header's definition, operation by operation and vectorised over
the samples — in float32 it gives the bits the call must give, in float64 the numbers of the reference —, the reference's own lines
(agents/networks/value_estimator.py:52-87, network_utils.q_to_v) restated in float64 numpy, inputs that reach every branch, the
buffers of one call with the argument struct over them, and a ring of random bits for the gather.  The model owes nothing to
drl-tetris_amd/csrc/tetris_kstep.h."""
import math

import numpy as np

import __graft_entry__ as ge
from tests.buffers import Buf, out

F32, F64, U32, U8, I32 = np.float32, np.float64, np.uint32, np.uint8, np.int32
U24 = 2.0 ** -24          # the relative error of one float32 rounding
SAFETY = 4.0


def capi():
    return ge.package().capi


def tolerance(k, n):
    """|float32 target - exact target| for rewards and values in [-1, 1], gamma and lambda in (0, 1].  Every partial sum P_t and every
    estimate E_s is at most k + 1 in magnitude, and the target is a convex combination of the E_s (the weights are >= 0), so an
    absolute error of e in any E_s, or a relative error of e / (k + 1) in num or den, moves the target by at most e.  Roundings,
    each 2^-24 relative to a magnitude of at most k + 1:
      the value of a step: at most 7 additions and a division of numbers up to 1 (counted as of k + 1: 8);
      E_s: k products r_t g_t and one V_s g_s with a rounded constant each — 2 (k + 1) roundings of magnitude 1, that is 2 of
        magnitude k + 1 — and k + 1 additions;
      the aggregate: n products E_s w_s with a rounded l_s each (2 n), n additions into num, n into den, one division.
    N = 8 + 2 + (k + 1) + 2 n + 2 n + 1 = k + 4 n + 12 roundings of (k + 1) 2^-24, times a safety factor of SAFETY = 4 for what the
    count simplifies (the float16 inputs are exact in both models)."""
    return SAFETY * (k + 4 * n + 12) * (k + 1) * U24


def discounts(ft, base, k):
    """(float)pow((double)base, t) for t = 0..k — base is the float32 the call carries —, as `ft`; in float64: not rounded"""
    p = [math.pow(float(F32(base)), t) for t in range(k + 1)]
    return [ft(F32(x)) if ft is F32 else ft(x) for x in p]


def view_rows(arr, index, k, max_size):
    """rows index[j] + t, t = 0..k, of a ring's array -> [M, k + 1] and the samples' validity; zeros for an invalid sample"""
    index = np.asarray(index, np.int64)
    ok = (index >= 0) & (index < max_size)
    at = np.where(ok, index, 0)[:, None] + np.arange(k + 1)[None, :]
    return np.where(ok[:, None], arr[at], np.zeros((), arr.dtype)), ok


def step_values(ft, x, K, W, values_mode, used):
    """x: Q [M, n, 4, 10, K] or v [M, n, W] -> V [M, n] in `ft`, by the header's order: the maximum over c ascending with
    `m < x ? x : m`, the sum over the used pieces from +0 in ascending p, one division"""
    x = x.astype(ft)
    M, n = x.shape[:2]
    if values_mode:
        m = x.reshape(M, n, W)
        width = W
    else:
        q = x.reshape(M, n, 40, K)
        m = q[:, :, 0, :]
        for c in range(1, 40):
            m = np.where(m < q[:, :, c, :], q[:, :, c, :], m)
        width = K
    if width == 1:
        return m[:, :, 0]
    s = np.zeros((M, n), ft)
    for p in range(width):
        if (used >> p) & 1:
            s = s + m[:, :, p]
    return s / ft(bin(used).count("1"))


def model(ft, x, reward, done, ok, k, steps, K, W, values_mode, used, gamma, lam, truncate):
    """reward float32 / done uint8 [M, k + 1]: the samples' rows; ok [M]: validity -> dict(target, values [M, n], done_time, den)"""
    M, n = reward.shape[0], len(steps)
    g, l = discounts(ft, gamma, k), discounts(ft, lam, k)
    V = np.where(ok[:, None], step_values(ft, x, K, W, values_mode, used), ft(0))
    nz = done != 0
    dt = np.where(nz.any(axis=1), nz.argmax(axis=1), k + 1)
    r = reward.astype(ft)
    P, num, den = np.zeros(M, ft), np.zeros(M, ft), np.zeros(M, ft)
    i = 0
    with np.errstate(all="ignore"):
        for s in range(1, k + 1):
            t = s - 1
            P = np.where(dt >= t, P + r[:, t] * g[t], P)
            if s not in steps:
                continue
            E = np.where(dt >= s, P + V[:, i] * g[s], P)
            w = np.where(dt < s - 1, ft(0), l[s]) if truncate else np.full(M, l[s], ft)
            num = num + E * w
            den = den + w
            i += 1
        target = np.where(ok & (den != 0), num / np.where(den != 0, den, ft(1)), ft(0))
    return dict(target=target.astype(ft), values=V.astype(ft), done_time=np.where(ok, dt, 0).astype(U8), den=np.where(ok, den, ft(1)), dt=dt)


def reference(x, reward, done, k, steps, K, W, values_mode, used, gamma, lam, truncate):
    """value_estimator.py:52-87 and q_to_v line by line in float64 numpy (TensorFlow is not needed for the arithmetic): dones 0 / 1,
    the net's outputs x, gamma and lambda the values the call carries.  -> the estimator's output [M] (NaN where it divides 0 by 0)"""
    M = reward.shape[0]
    gamma, lam = float(F32(gamma)), float(F32(lam))
    dones = (done != 0).astype(F64)[:, :, None]
    rewards = reward.astype(F64)[:, :, None]
    mask = np.array([(used >> p) & 1 for p in range(K)], F64).reshape(1, 1, 1, K)
    n_used = bin(used).count("1")
    _d = np.minimum(1, np.cumsum(dones, axis=1))
    done_time = np.sum(1 - _d, axis=1)                                             # [M, 1]
    v_step, idx_dict = [None] * len(steps), {}
    for idx, t in enumerate(steps):
        idx_dict[t] = idx
        out_t = x[:, idx].astype(F64)
        if values_mode:
            _v_t = out_t.reshape(M, 1, 1, W)
            if W == K and K > 1:                                                   # separate_piece_values
                _v_t = np.sum(_v_t * mask, axis=3, keepdims=True) / n_used
        else:                                                                      # q_to_v
            q_p = np.max(out_t.reshape(M, 4, 10, K), axis=(1, 2), keepdims=True)
            _v_t = np.sum(q_p * mask, axis=3, keepdims=True) / n_used if K > 1 else q_p
        v_step[idx] = _v_t.reshape(-1, 1)

    def k_step_estimate(kk):
        e = 0
        for t in range(kk):
            e = e + rewards[:, t, :] * (done_time >= t).astype(F64) * (gamma ** t)
        v_k = v_step[idx_dict[kk]]
        return e + v_k * (done_time >= kk).astype(F64) * (gamma ** kk)
    estimators = [(kk, k_step_estimate(kk)) for kk in steps]
    estimator_sum, weight = 0, 0
    for kk, e in estimators:
        lambda_filter = (done_time >= kk - 1).astype(F64) if truncate else 1.0
        _lambda = lam * lambda_filter
        estimator_sum = estimator_sum + e * _lambda ** kk
        weight = weight + _lambda ** kk
    with np.errstate(all="ignore"):
        return (estimator_sum / weight).reshape(M)


# ---------------------------------------------------------------- inputs
def step_sets(k):
    """the step sets of a k: all, filter [2], (k = 37) filter [2, 3], the single step {k}, one without step 1 — without repeats"""
    c = capi()
    sets = [c.kstep_steps(k), c.kstep_steps(k, [2])]
    if k == 37:
        sets.append(c.kstep_steps(k, [2, 3]))
    sets += [[k], list(range(2, k + 1))]
    res = []
    for s in sets:
        if s and s not in res:
            res.append(s)
    return res


def make_inputs(rng, M, k, n, K, W, values_mode, dtype):
    """-> dict(x, rows_r [M, k + 1], rows_d, ring_r, ring_d, index, max_size): the net's outputs in [-1, 1] as `dtype`, rewards in
    [-1, 1], and a ring of (M + 1) (k + 1) positions in which sample j's view is the block perm[j] — its done row by j % 8: none;
    row 0; row k; the middle; several, the first one 255; random; none; row min(1, k) with a 255 —, the last block's last position
    a view that runs past max_size, and where M >= 33 two indices outside [0, max_size)."""
    shape = (M, n, W) if values_mode else (M, n, 4, 10, K)
    x = rng.uniform(-1, 1, shape)
    if not values_mode:
        q = x.reshape(M * n, 40, K)
        rows = np.arange(M * n)
        q[rows % 11 == 3] = -0.5 * np.abs(q[rows % 11 == 3]) - 1e-3               # negative values only
        q[rows % 13 == 5] = rng.choice([0.0, -0.0], q[rows % 13 == 5].shape)       # ties of +0 and -0: the order of the maximum
        q[rows % 7 == 1, 0, :] = 1.0                                               # the maximum first ...
        q[rows % 7 == 2, 39, :] = 1.0                                              # ... and last
        q[rows % 17 == 4, 5, :] = 3e-6                                             # (binary16: subnormal)
        x = q.reshape(shape)
    x = x.astype(dtype)
    blocks, width = M + 1, k + 1
    max_size = blocks * width
    rows_r = rng.uniform(-1, 1, (blocks, width)).astype(F32)
    rows_d = np.zeros((blocks, width), U8)
    for j in range(blocks):
        kind = j % 8
        if kind == 1:
            rows_d[j, 0] = 1
        elif kind == 2:
            rows_d[j, k] = 1
        elif kind == 3:
            rows_d[j, k // 2] = 1
        elif kind == 4:
            rows_d[j, rng.integers(0, width, 3)] = 1
            rows_d[j, np.argmax(rows_d[j])] = 255
        elif kind == 5:
            rows_d[j] = rng.random(width) < 1.0 / width
        elif kind == 7:
            rows_d[j, min(1, k)] = 255
    perm = rng.permutation(M)
    index = (perm * width).astype(np.int64)
    if M >= 2:
        index[M - 1] = max_size - 1                                               # rows 1 .. k lie at and past max_size: zeros
    if M >= 33:
        index[5], index[M - 3] = -1, max_size + 2
    ring_r = np.concatenate([rows_r.reshape(-1), np.zeros(k, F32)])
    ring_d = np.concatenate([rows_d.reshape(-1), np.zeros(k, U8)])
    return dict(x=x, ring_r=ring_r, ring_d=ring_d, index=index.astype(np.int64).astype(U32).view(I32), max_size=max_size)


class KstepCall:
    """the buffers of one call and the argument struct over them; ring: ring mode (the ring's arrays and the index), else array mode
    (the samples' rows as [M, k + 1] arrays)"""

    def __init__(self, kind, b, inp, k, steps, K, W, values_mode, used, gamma, lam, truncate, ring=True, want_values=True, want_dt=True,
                 **override):
        self.kind = kind
        x = inp["x"]
        M, n = x.shape[0], len(steps)
        assert x.shape[1] == n, "the net's output must hold a row per step of the list"
        rows_r, ok = view_rows(inp["ring_r"], inp["index"], k, inp["max_size"])
        rows_d, _ = view_rows(inp["ring_d"], inp["index"], k, inp["max_size"])
        self.rows_r, self.rows_d, self.ok = rows_r, rows_d, (ok if ring else np.ones(M, bool))
        self.x = Buf(kind, x)
        if ring:
            self.reward, self.done, self.index = Buf(kind, inp["ring_r"]), Buf(kind, inp["ring_d"]), Buf(kind, inp["index"])
        else:
            self.reward, self.done, self.index = Buf(kind, rows_r), Buf(kind, rows_d), None
        self.outs = dict(target=out(kind, (max(M, 1),), F32))
        if want_values:
            self.outs["values"] = out(kind, (max(M, 1), n), F32)
        if want_dt:
            self.outs["done_time"] = out(kind, (max(M, 1),), U8)
        kw = dict(out=self.x.ptr, reward=self.reward.ptr, done=self.done.ptr, target=self.outs["target"].ptr, m=M, k_step=k, steps=steps,
                  index=self.index.ptr if ring else None, max_size=inp["max_size"] if ring else 0, values_mode=values_mode, n_pieces=K,
                  n_values=W if values_mode else 1, used_pieces=used, f16=np.dtype(x.dtype) == np.float16, truncate=truncate, gamma=gamma, lam=lam,
                  values=self.outs["values"].ptr if want_values else None, done_time=self.outs["done_time"].ptr if want_dt else None)
        kw.update(override)
        self.M = kw["m"]
        self.t = b.kstep_target(**kw)

    def get(self):
        return {name: buf.get() for name, buf in self.outs.items()}


# ---------------------------------------------------------------- a ring of random bits for the gather
RING_ARRAYS = ("obs", "action", "prob", "adv", "target", "reward", "done", "flags", "prio", "cursor")


class RandomRing:
    """a replay buffer of random bits below max_size, zeros in the never-written rows, flags 0 / 1"""

    def __init__(self, kind, b, capacity, k_step, rng):
        S = b.n_players
        self.kind, self.b, self.C, self.k_step, self.max_size, self.S = kind, b, capacity, k_step, capacity - k_step, S
        bits = lambda shape, dt: rng.integers(0, 256, shape).astype(U8) if dt == U8 else rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(U32)  # noqa: E731
        shapes = dict(obs=((capacity, S, 12), U32), action=((capacity, 4), U8), prob=((capacity,), U32), adv=((capacity,), U32),
                      target=((capacity,), U32), reward=((capacity,), U32), done=((capacity,), U8), flags=((capacity,), U8),
                      prio=((self.max_size,), U32), cursor=((4,), I32))
        self.np = {}
        for name, (shape, dt) in shapes.items():
            v = np.zeros(shape, dt) if name == "cursor" else bits(shape, dt)
            if name == "flags":
                v &= 1
            if name == "obs":                                                      # words 10 / 11 as the header defines them
                v[..., 11] = rng.integers(0, 256, shape[:2]) | (rng.integers(0, 8, shape[:2]) << 8) | (rng.integers(0, 8, shape[:2]) << 16)
            if name == "action":
                v[:, 1], v[:, 2] = rng.integers(0, 10, capacity), rng.integers(0, 7, capacity)
            if name not in ("prio", "cursor"):
                v[self.max_size:] = 0
            self.np[name] = v
        self.bufs = {name: Buf(kind, v) for name, v in self.np.items()}
        self.rp = b.replay(capacity, k_step, *[self.bufs[n].ptr for n in RING_ARRAYS])
