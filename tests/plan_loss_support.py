"""The planning loss head (include/tetris_hip.h: tetris_plan_loss_dev): a numpy model written from the definition in
drl-tetris_amd/csrc/tetris_loss.h (PLAN), operation by operation and vectorised over the samples, with every sum in the stated
order — in float32 it gives the bits the head must give wherever no logarithm enters, in float64 the numbers the entropy-dependent
outputs are compared with —, the tolerances of that comparison, the reference's expressions (delta_ppo_nets.py:150-182) written
with torch ops for autograd, a planning window recorded through the library's own calls, inputs that reach every branch, and the
buffers of one call with the argument struct over them.  The model is fed the planes batch_plan expands from the same records:
the very numbers the head has to reconstruct."""
import collections
import os

import numpy as np

from oracle import oracle as orc
from tests import engines, replay
from tests.buffers import MIRROR, Buf, out
from tests.loss_support import (E32, F32, F64, U24, assert_carry_mask, carry_mask, same_bits, stated_bound, stated_sum,        # noqa: F401
                                sum_bound, weigh_the_full_slots, written)                             # (re-exported to the test file)
from tests.plan_support import _crafted, _words

U8, U32, I32 = np.uint8, np.uint32, np.int32
WORDS = 112
LANES = 64                    # the lanes of the cell order
BLOCK = 16                    # samples of a block of the across-sample sums
LOGF_ULPS = 3                 # what tests/test_loss_head.py allows a device logf: the bound OpenCL sets and the device library documents
PlanParams = collections.namedtuple("PlanParams", "clip c1 c2 c3 c4")
# (clip, c1, c2, c3, c4) of the autograd comparison
PARAM_SETS = (PlanParams(0.15, 0.3, 1.0, 1e-4, 0.01), PlanParams(0.05, 1.0, 1.0, 0.5, 1.0), PlanParams(0.2, 0.5, 2.0, 0.01, 0.0))
STATS = ("n", "loss", "value_loss", "policy_loss", "entropy_loss", "impossibility_loss", "entropy", "entropy_sq", "values", "values_sq",
         "target_values", "target_values_sq", "clip_saturation", "ratio", "probability")
GOLDEN = os.path.join(replay.GOLDEN, "traj_plan.npz")


# ---------------------------------------------------------------- the model
def cell_sum(z):
    """SUM of the definition over z [M, HW]: cell t belongs to lane t mod 64, a lane starts at +0 and adds its cells in ascending
    t, the 64 lane sums go through the tree v[i] += v[i + off], off = 32, 16, .., 1"""
    M, HW = z.shape
    lanes = np.zeros((M, LANES), z.dtype)
    for first in range(0, HW, LANES):
        part = z[:, first:first + LANES]
        lanes[:, :part.shape[1]] = lanes[:, :part.shape[1]] + part
    off = LANES // 2
    while off >= 1:
        lanes[:, :off] = lanes[:, :off] + lanes[:, off:2 * off]
        off //= 2
    return lanes[:, 0].copy()


def plan_model(ft, phi, v, delta, sums, piece, old, adv, target, ok, prm, grad_scale=1.0):
    """The head in the float type `ft`, every line one operation of the definition.  delta, sums: float32 [M, H, 10] as batch_plan
    gives them; ok bool [M]: valid[m] != 0 and the index names an entry.  -> dict: per-sample probability, ratio, cl, pl, Hent, I,
    val (zeros for samples that are not ok), g [M, HW] (the piece's plane of grad_phi), gv [M], k, D, `terms` [M, 12] (the
    per-sample terms of the twelve sums), and what the tolerances need: y, l, w, S, the parts of g."""
    M, H, K, V = phi.shape[0], phi.shape[1], phi.shape[3], v.shape[1]
    HW = 10 * H
    rows = np.arange(M)
    k = np.minimum(piece.astype(np.int64), K - 1)
    one, zero, e = ft(1.0), ft(0.0), ft(E32)
    clip, c1, c2, c3, c4, gs = (ft(F32(z)) for z in (prm.clip, prm.c1, prm.c2, prm.c3, prm.c4, grad_scale))
    with np.errstate(all="ignore"):
        D = ft(ok.sum())
        raw = phi.reshape(M, HW, K)[rows, :, k].astype(ft)
        lowc = np.where(raw > one, one, raw)
        x = np.where(lowc < e, e, lowc)
        passes = (e <= raw) & (raw <= one)
        d, s = delta.reshape(M, HW).astype(ft), sums.reshape(M, HW).astype(ft)
        a, b, u = x * d, x * s, s + e
        m1 = np.where(s < one, s, one)
        i = x * (one - m1)
        num, dn, S, I = cell_sum(a), cell_sum(b), cell_sum(u), cell_sum(i)
        val = v[rows, np.minimum(k, V - 1)].astype(ft)
        old, A, T = old.astype(ft), adv.astype(ft), target.astype(ft)
        dv = val - T
        den2 = dn + e
        p = (num + e) / den2
        den = np.where(old < e, e, old)
        ratio = np.where(p < e, e, p) / den
        lo, hi = one - clip, one + clip
        low = np.where(ratio < lo, lo, ratio)
        cl = np.where(low > hi, hi, low)
        ra, ca = ratio * A, cl * A
        pl = np.where(ca < ra, ca, ra)
        rp = np.where(p >= e, one, zero) / den
        dpl = np.where(ra <= ca, A * rp, A * rp * np.where(cl == ratio, one, zero))
        pp = (-(c2 / D)) * dpl
        ci = (c4 / D) / ft(HW)
        ce = -(c3 / D)
        w = s / S[:, None]
        y = b / S[:, None] + e
        l = np.log(np.where(y <= e, e, y))
        above = np.where(y > e, one, zero)
        Hent = -cell_sum(y * l)
        dp = (d - p[:, None] * s) / den2[:, None]
        et = -(l + above)
        g_policy, g_imp, g_entropy = pp[:, None] * dp, ci * (one - m1), ce * (et * w)
        g = np.where(passes, ((g_policy + g_imp) + g_entropy) * gs, zero)
        gv = (((ft(2.0) * c1) * dv) / D) * gs
        terms = np.stack([dv * dv, pl, Hent, Hent * Hent, val, val * val, T, T * T, np.where(ratio != cl, one, zero), ratio, p, I], axis=1)
    res = dict(probability=p, ratio=ratio, cl=cl, pl=pl, Hent=Hent, I=I, val=val, g=g, gv=gv, terms=terms)
    for arr in res.values():
        arr[~ok] = 0
    assert all(arr.dtype == ft for arr in res.values()), "an operation of the model left its float type"
    res.update(k=k, ok=ok, D=float(D), A=A, y=y, l=l, w=w, S=S, b=b, u=u, et=et, passes=passes, raw=raw, s=s, x=x,
               g_policy=g_policy * gs, g_imp=np.broadcast_to(g_imp * gs, g.shape), g_entropy=g_entropy * gs, ce=float(ce * gs))
    return res


def plan_stated_stats(terms, D, prm, H):
    """float32 [16]: the statistics from the twelve per-sample float32 terms [M, 12] (plan_model's `terms`), summed in the stated
    order (loss_support.stated_sum with blocks of 16) and finished as the definition writes it, every operation in float32"""
    assert terms.dtype == F32 and terms.shape[1] == 12
    total = stated_sum(terms, BLOCK)
    stats = np.zeros(16, F32)
    D = F32(D)
    if not D > 0:
        return stats
    c1, c2, c3, c4 = (F32(z) for z in prm[1:])
    vl, pol, ent = c1 * (total[0] / D), (-c2) * (total[1] / D), (-c3) * (total[2] / D)
    imp = c4 * ((total[11] / D) / F32(10 * H))
    stats[:6] = D, ((vl + pol) + imp) + ent, vl, pol, ent, imp
    stats[6:15] = [total[col] / D for col in range(2, 11)]
    return stats


def expand(plane, k, K, dtype):
    """[M, HW] values of each sample's piece -> the whole [M, H, 10, K] array, zeros elsewhere, as `dtype`"""
    M, HW = plane.shape
    full = np.zeros((M, HW, K), plane.dtype)
    full[np.arange(M), :, k] = plane
    with np.errstate(over="ignore"):
        return full.reshape(M, HW // 10, 10, K).astype(dtype)


def expand_v(gv, k, V, dtype):
    full = np.zeros((gv.shape[0], V), gv.dtype)
    full[np.arange(gv.shape[0]), np.minimum(k, V - 1)] = gv
    with np.errstate(over="ignore"):
        return full.astype(dtype)


# ---------------------------------------------------------------- tolerances of what passes through the logarithm
def entropy_tolerances(m, grad_dtype):
    """From the float64 model m -> (tol_H [M], tol_g [M, HW]): how far the float32 head's Hent and, with policy_loss = 0, its
    grad_phi may lie from the model.
    S is a float32 sum of HW terms u_t = s_t + e, each rounded once: |dS| <= sum_bound(u) + 2^-24 sum |u_t|, rel_S = |dS| / |S|.
    y_t = b_t / S + e: b_t (one rounding), the quotient (one rounding and rel_S), the sum (one rounding):
      |dy_t| <= |b_t / S| (2 x 2^-24 + rel_S) + 2^-24 |y_t|.
    l_t = logf(max(e, y_t)): the argument's error over the argument, plus LOGF_ULPS ulp of the result (an ulp is at most
      2^-23 |l_t|):  |dl_t| <= |dy_t| / max(y_t, e) + LOGF_ULPS 2^-23 |l_t|.
    A term y_t l_t: |dy_t| |l_t| + |y_t| |dl_t| + 2^-24 |y_t l_t| (the product's rounding); Hent adds the bound of a float32
    sum of HW terms in any order, sum_bound.  Times four, as tests/test_loss_head.py takes its derived bounds.
    grad_phi with policy_loss = 0 is (ci (1 - m_t) + ce (e_t w_t)) grad_scale: e_t = -(l_t + [y_t > e]) carries |dl_t| and one
    rounding, w_t = s_t / S carries 2^-24 + rel_S, the product one rounding; ce, ci, the two products with them, the sum and the
    scale are at most eight roundings of magnitudes below |g_imp| + |g_entropy|.  Times four; a float16 gradient adds its own
    rounding, 2^-11 |g| and 2^-25 below the normal range."""
    with np.errstate(all="ignore"):
        e = float(E32)
        dS = np.array([sum_bound(row) for row in m["u"]]) + U24 * np.abs(m["u"]).sum(axis=1)
        rel_S = (dS / np.abs(m["S"]))[:, None]
        q = np.abs(m["b"] / m["S"][:, None])
        dy = q * (2 * U24 + rel_S) + U24 * np.abs(m["y"])
        dl = dy / np.maximum(m["y"], e) + LOGF_ULPS * 2 * U24 * np.abs(m["l"])
        yl = m["y"] * m["l"]
        dterm = dy * np.abs(m["l"]) + np.abs(m["y"]) * dl + U24 * np.abs(yl)
        tol_H = 4 * (dterm.sum(axis=1) + np.array([sum_bound(row) for row in yl]))
        etw = np.abs(m["et"] * m["w"])
        d_etw = (dl + U24 * np.abs(m["et"])) * np.abs(m["w"]) + etw * (2 * U24 + rel_S)
        size = np.abs(m["g_imp"]) + np.abs(m["g_entropy"])
        tol_g = 4 * (abs(m["ce"]) * d_etw + 8 * U24 * size)
        if np.dtype(grad_dtype) == np.float16:
            tol_g = tol_g + 2.0 ** -11 * np.abs(m["g"]) + 2.0 ** -25
    tol_H[~m["ok"]] = 0
    tol_g[~m["ok"]] = 0
    return tol_H, tol_g


# ---------------------------------------------------------------- the reference's expressions with torch ops (float64, CPU)
def clip_by_value(torch, x, lo, hi):
    """tf.clip_by_value: maximum(minimum(x, hi), lo); its gradient goes to x at a tie (torch.clamp's does too)"""
    return torch.clamp(x, min=lo, max=hi)


def torch_plan_loss(torch, raw_phi, values_in, delta, sums, piece, old, adv, target, rows, prm):
    """delta_ppo_nets.py:30 and 150-182 of the samples `rows`, line by line; raw_phi [M, H, 10, K] and values_in [M, V] are float64
    leaf tensors -> (loss, probability, r, entropy)"""
    clip_param, c1, c2, c3, c4 = (float(F32(z)) for z in prm)                    # the float32 values a call carries
    e = float(E32)
    K, V = raw_phi.shape[3], values_in.shape[1]
    sel = torch.from_numpy(np.nonzero(rows)[0])
    phi_all = clip_by_value(torch, raw_phi[sel], e, 1.0)                                                             # :30
    pieces_training = torch.from_numpy(np.minimum(piece.astype(np.int64), K - 1))[sel]
    deltas_training, delta_sums_training = (torch.from_numpy(z.astype(F64))[sel][..., None] for z in (delta, sums))
    old_probs, advantages, target_values = (torch.from_numpy(z.astype(F64))[sel] for z in (old, adv, target))
    p_mask = torch.nn.functional.one_hot(pieces_training, K).reshape(-1, 1, 1, K).double()                           # :152
    values = (values_in[sel] * p_mask.reshape(-1, K)).sum(dim=1) if V == K else values_in[sel][:, 0]                  # :153
    phi = (phi_all * p_mask).sum(dim=3, keepdim=True)                                                                # :155
    delta_phi = phi * deltas_training                                                                                # :156
    delta_sum_phi = phi * delta_sums_training                                                                        # :157
    probability = (delta_phi.sum(dim=(1, 2, 3)) + e) / (delta_sum_phi.sum(dim=(1, 2, 3)) + e)                         # :158
    r = torch.clamp(probability, min=e) / torch.clamp(old_probs, min=e)                                              # :161
    clipped_r = clip_by_value(torch, r, 1 - clip_param, 1 + clip_param)                                              # :162
    policy_loss = torch.minimum(r * advantages, clipped_r * advantages)                                              # :169
    impossibility_loss_tf = phi * (1 - torch.clamp(delta_sums_training, max=1.0))                                    # :171
    pi = delta_sum_phi / (delta_sums_training + e).sum(dim=(1, 2, 3), keepdim=True) + e                              # :173
    action_entropy = -(pi * torch.log(torch.clamp(pi, min=e))).sum(dim=(1, 2), keepdim=True)                         # network_utils.py:116-117
    value_loss_tf = c1 * ((values - target_values) ** 2).mean()                                                      # :177
    policy_loss_tf = -c2 * policy_loss.mean()                                                                        # :178
    entropy_loss_tf = -c3 * action_entropy.mean()                                                                    # :179
    impossibility = c4 * impossibility_loss_tf.mean()                                                                # :180
    return value_loss_tf + policy_loss_tf + impossibility + entropy_loss_tf, probability, r, action_entropy.reshape(-1)      # :182


# ---------------------------------------------------------------- a recorded planning window
class Window:
    """T rows of a batch's games with observation and plan records, recorded by the library's own calls"""

    def __init__(self, kind, b, T):
        n, S = b.n_games, b.n_players
        self.kind, self.b, self.T, self.n = kind, b, T, n
        shapes = dict(action=((T, n, 4), U8), prob=((T, n), F32), value=((2, T, n), F32), reward=((T, n), F32), done=((T, n), U8),
                      obs=((T, n, S, 12), U32), rec=((T, n, WORDS), U32))
        self.bufs = {name: Buf.full(kind, shape, dt) for name, (shape, dt) in shapes.items()}
        p = lambda name: self.bufs[name].ptr                                                     # noqa: E731
        self.traj = b.traj(T, p("action"), p("prob"), p("value"), p("reward"), p("done"))
        self.tobs = b.traj_obs(T, p("obs"))
        self.plan = b.traj_plan(T, p("rec"))
        self.total = T * n
        self.keep = []                    # the inputs of the recording calls, alive as long as the window

    def record(self, row, player, count, cols, choice, piece, L):
        b, kind, n = self.b, self.kind, self.n
        keep = [Buf(kind, np.asarray(player, U8)), Buf(kind, np.asarray(count, I32)), Buf(kind, np.ascontiguousarray(cols)),
                Buf(kind, np.asarray(choice, I32)), Buf(kind, np.asarray(piece, U8)), Buf(kind, np.full(n, 0.5, F32)),
                Buf(kind, np.zeros(n, U8)), Buf(kind, np.zeros((b.n_players, n), U8))]
        e = b.plan_eval(None, keep[1].ptr, keep[2].ptr, keep[3].ptr, max_lists=L, piece=keep[4].ptr, prob=keep[5].ptr, player=keep[0].ptr)
        b.traj_observe_dev(self.tobs, row, keep[0].ptr)
        b.traj_record_plan_dev(self.traj, self.plan, self.tobs, row, e, keep[6].ptr, keep[7].ptr)
        self.keep.append(keep)

    def planes(self, index, fill):
        """batch_plan of the index list in float32 -> (delta, sums) [M, H, 10]"""
        M, H = len(index), self.b.height
        ib = Buf(self.kind, np.asarray(index, np.int64).astype(U32).view(I32))
        d, s = out(self.kind, (M, H, 10), F32), out(self.kind, (M, H, 10), F32)
        self.b.traj_plan_batch_dev(self.plan, ib.ptr, M, delta=d.ptr, sums=s.ptr, small_fill=fill)
        return d.get(), s.get()

    def kinds(self):
        return self.bufs["rec"].get().reshape(self.total, WORDS)[:, 20]


def crafted_window(kind, H):
    """24 crafted games (tests/plan_support._crafted: per list nothing new, three cells (both SMALL), four cells, two cells leave
    and six arrive, random words; counts from -1 to past L), two rows with different choices -> Window.  The chosen lists are
    NORMAL, SMALL and, where a game has no list, none (PAST)."""
    N, T, L, P = 24, 2, 12, (2 if H == 20 else 1)
    b, player, count, cols, before, after = _crafted(kind, N, P, H, L, seed=1000 + H)
    w = Window(kind, b, T)
    rng = np.random.default_rng(H)
    for row in range(T):
        choice = rng.integers(-1, L + 1, N)
        choice[:10] = (np.arange(10) + row) % 5                    # (game + list) mod 5 is the list's case: every case is chosen
        w.record(row, player, count, cols, choice, rng.integers(0, 9, N), L)
    return w


def golden_window(kind):
    """The episodes of tests/golden/traj_plan.npz, one per game column from row 0 on: per row the acting player's boards are
    restored to the fixture's `before`, observed, and recorded with d_cols from its `after` fields and its a_idx.  -> (Window,
    index [M] of the entries that hold a fixture step, k [M]: the fixture's step of each)"""
    z = np.load(GOLDEN)
    E, H, L, P = len(z["case"]), 20, z["after"].shape[1], 2
    T = int(z["length"].max())
    b = engines.make(kind, E, P, height=H, seeds=orc.episode_seed(np.arange(E), 4))
    w = Window(kind, b, T)
    blob = b.snapshot()
    first_word = b.snapshot_words - P * b.lib.tetris_layout_words()                              # the acting player 0's column words
    index, steps = [], []
    for t in range(T):
        before, after = np.zeros((E, H, 10), bool), np.zeros((E, L, H, 10), bool)
        choice, piece = np.zeros(E, I32), np.zeros(E, U8)
        for e_ in range(E):
            if t < int(z["length"][e_]):
                k = int(z["start"][e_]) + t
                before[e_], after[e_], choice[e_], piece[e_] = z["before"][k], z["after"][k], z["a_idx"][k], z["piece"][k]
                index.append(t * E + e_)
                steps.append(k)
        blob[:, first_word:first_word + 10] = _words(before)
        b.restore(blob)
        cols = np.zeros((L, P, 10, E), U32)
        cols[:, 0] = _words(after).transpose(1, 2, 0)
        w.record(t, np.zeros(E, U8), np.full(E, L, I32), cols, choice, piece, L)
    return w, np.array(index, np.int64), np.array(steps, np.int64), z


# ---------------------------------------------------------------- inputs
def sample_index(rng, M, total):
    """M entries of a window of `total`: random with repeats, about half mirrored; from three samples on one names no entry (-1),
    from sixteen on also `total` and total + 5 with the mirror bit"""
    index = rng.integers(0, total, M).astype(np.int64)
    index = np.where(rng.random(M) < 0.5, index | MIRROR, index)
    if M >= 3:
        index[1] = -1
        index[2] |= MIRROR
    if M >= 16:
        index[7], index[12] = total, (total + 5) | MIRROR
    return index


def named(index, total):
    """whether an element of an index list names an entry"""
    return (np.asarray(index, np.int64).astype(U32) & U32(0x7FFFFFFF)) < total


def plan_inputs(rng, M, H, K, V, dtype, masked, ties=True):
    """phi raw: about a sixth of the cells below e (negative, zero, 5e-7), a sixth above 1, the rest in between (ties=False: all
    strictly inside (e, 1)); advantages of both signs; pieces out of range on some; with `masked` invalid samples at both ends.
    prob_old is set by with_old once the probabilities are known."""
    phi = 0.02 + 0.9 * rng.random((M, H, 10, K))
    if ties:
        what = rng.integers(0, 12, phi.shape)
        phi = np.where(what == 0, -rng.random(phi.shape), np.where(what == 1, 0.0, np.where(what == 2, 5e-7, phi)))
        phi = np.where(what >= 10, 1.0 + rng.random(phi.shape), phi)
    piece = rng.integers(0, K, M).astype(U8)
    if ties:
        piece[np.arange(M) % 5 == 1] = 250
    valid = None
    if masked:
        valid = np.ones(M, U8)
        valid[[0, M - 1]] = 0
        valid[valid != 0] = rng.integers(1, 256, int((valid != 0).sum()))       # any non-zero byte counts
    return dict(phi=phi.astype(dtype), v=rng.standard_normal((M, V)).astype(dtype), piece=piece, old=np.ones(M, F32),
                adv=rng.standard_normal(M).astype(F32), target=rng.standard_normal(M).astype(F32), valid=valid)


def with_old(inp, probability, rng):
    """prob_old = max(probability, e) / f with f around 0.5, 1 and 2 (ratio below, inside and above any clip range used here), 0 and
    5e-7 (< e) on some"""
    M = len(probability)
    rows = np.arange(M)
    factor = np.choose(rows % 3, [0.5 + 0.2 * rng.random(M), 0.97 + 0.06 * rng.random(M), 1.6 + rng.random(M)])
    with np.errstate(all="ignore"):
        old = (np.maximum(np.nan_to_num(probability.astype(F64)), float(E32)) / factor).astype(F32)
    old[rows % 17 == 6] = 0.0
    old[rows % 17 == 9] = 5e-7
    inp["old"] = old
    return inp


def ok_of(inp, index, total):
    M = len(index)
    return (np.ones(M, bool) if inp["valid"] is None else inp["valid"] != 0) & named(index, total)


# ---------------------------------------------------------------- calls
class PlanLossCall:
    """The buffers of one call, of exactly the documented sizes, and the argument struct over them.  Outputs are pre-filled with
    the guard byte and have guard bytes behind them.  stride3: the pieces travel as byte 2 of an action array [M][3]."""

    def __init__(self, kind, b, plan, inp, idx, prm, fill, grad_dtype=F32, grad_scale=1.0, terms=True, stride3=False, **override):
        phi, v = inp["phi"], inp["v"]
        M, H, K, V = phi.shape[0], phi.shape[1], phi.shape[3], v.shape[1]
        self.plan = plan
        self.inp = {name: None if a is None else Buf(kind, a) for name, a in inp.items()}
        self.inp["index"] = Buf(kind, np.asarray(idx, np.int64).astype(U32).view(I32))
        piece_ptr, stride = self.inp["piece"].ptr, 1
        if stride3:
            action = np.full((M, 3), 99, U8)
            action[:, 2] = inp["piece"]
            self.inp["action"] = Buf(kind, action)
            piece_ptr, stride = self.inp["action"].ptr + 2, 3
        self.out = dict(grad_phi=out(kind, (M, H, 10, K), grad_dtype), grad_v=out(kind, (M, V), grad_dtype), stats=out(kind, (16,), F32))
        if terms:
            self.out["terms"] = out(kind, (6, M), F32)
        p = lambda d, name: None if d.get(name) is None else d[name].ptr            # noqa: E731
        kw = dict(phi=p(self.inp, "phi"), v=p(self.inp, "v"), index=p(self.inp, "index"), piece=piece_ptr, prob_old=p(self.inp, "old"),
                  adv=p(self.inp, "adv"), target=p(self.inp, "target"), grad_phi=p(self.out, "grad_phi"), grad_v=p(self.out, "grad_v"),
                  stats=p(self.out, "stats"), m=M, n_pieces=K, n_values=V, piece_stride=stride, valid=p(self.inp, "valid"),
                  terms=p(self.out, "terms"), f16=phi.dtype == np.float16, value_f16=v.dtype == np.float16,
                  grad_f16=np.dtype(grad_dtype) == np.float16, small_fill=fill, clipping_parameter=prm.clip, value_loss=prm.c1,
                  policy_loss=prm.c2, entropy_loss=prm.c3, impossibility_loss=prm.c4, grad_scale=grad_scale)
        kw.update(override)
        self.l = b.plan_loss(**kw)

    def run(self, b):
        b.plan_loss_dev(self.plan, self.l)
        return self.get()

    def get(self):
        return {name: buf.get() for name, buf in self.out.items()}
