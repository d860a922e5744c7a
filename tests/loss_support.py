"""The trainer's loss heads (include/tetris_hip.h: tetris_ppo_loss_dev, tetris_dqn_loss_dev): a numpy model written from the
header's definitions, operation by operation and vectorised over the samples — in float32 it gives the bits the heads must give
wherever no logarithm enters, in float64 the numbers the entropy-dependent outputs are compared with —, the reference's two
losses written with torch ops for autograd, inputs that reach every branch, and the buffers of one call with the argument
struct over them.  The model owes nothing to drl-tetris_amd/csrc/tetris_loss.h."""
import collections

import numpy as np

from tests.buffers import GUARD, Buf, out

F32, F64 = np.float32, np.float64
E32 = F32(1e-6)
Params = collections.namedtuple("Params", "clip c1 c2 c3 eps cf cr")
# the three parameter sets (clip, c1, c2, c3, eps, cf, cr) of the autograd comparison
PARAM_SETS = (Params(0.15, 0.3, 1.0, 1e-4, 0.05, 1.0, 2.0), Params(0.15, 0.3, 1.0, 0.01, 0.9, 1.0, 0.0), Params(0.05, 1.0, 1.0, 0.5, 0.3, 0.5, 0.5))
PPO_STATS = ("n", "loss", "value_loss", "policy_loss", "entropy_loss", "entropy", "entropy_sq", "entropy_bonus", "values", "values_sq",
             "target_values", "target_values_sq", "clip_saturation", "ratio")
DQN_STATS = ("n", "n_weighted", "loss", "q_val", "q_val_sq", "q_target", "q_target_sq", "new_prio")
U24 = 2.0 ** -24          # half an ulp of a float32 in [1, 2): the relative error of one rounding


def entropy_constants(eps):
    """(floor, Hmax) in float64: ppo_nets.py:175-180"""
    floor = -eps * np.log(eps / 39.0) - (1.0 - eps) * np.log(1.0 - eps)
    u = np.full(40, 1.0 / 40.0)
    return float(floor), float(-np.sum(u * np.log(u + 1e-8)))


def indices(action, K):
    a = action.astype(np.int64)
    return np.minimum(a[:, 2], K - 1), 10 * np.minimum(a[:, 0], 3) + np.minimum(a[:, 1], 9)


def expand(plane, k, K, dtype):
    """[M, 40] values of each sample's piece -> the whole [M, 4, 10, K] array, zeros elsewhere, as `dtype`"""
    M = plane.shape[0]
    full = np.zeros((M, 40, K), plane.dtype)
    full[np.arange(M), :, k] = plane
    with np.errstate(over="ignore"):                    # (a float16 gradient past 65504 is an infinity on both sides)
        return full.reshape(M, 4, 10, K).astype(dtype)


def expand_v(gv, k, V, dtype):
    full = np.zeros((gv.shape[0], V), gv.dtype)
    full[np.arange(gv.shape[0]), np.minimum(k, V - 1)] = gv
    with np.errstate(over="ignore"):
        return full.astype(dtype)


# ---------------------------------------------------------------- the model
def ppo_model(ft, pi, v, action, old, adv, target, valid, prm, grad_scale=1.0, floor=None):
    """The PPO head in the float type `ft`, every line one operation of the header.  The parameters enter as the float32 values
    the call carries.  -> dict: per-sample p, ratio, cl, pl, H, bonus, val (zeros for invalid samples), g [M, 40] (the piece's plane
    of grad_pi), g_policy [M] (its policy part at c), g_entropy [M, 40], ce, gv [M], k, c, ok, D, floor, and `terms`: the eleven
    per-sample terms of the sums."""
    M, K, V = pi.shape[0], pi.shape[3], v.shape[1]
    k, c = indices(action, K)
    rows = np.arange(M)
    ok = np.ones(M, bool) if valid is None else valid != 0
    one, zero, e = ft(1.0), ft(0.0), ft(E32)
    fl, hmax = entropy_constants(prm.eps) if floor is None else (floor, entropy_constants(0.5)[1])
    clip, c1, c2, c3, cf, cr, fl, hmax, gs = (ft(F32(x)) for x in (prm.clip, prm.c1, prm.c2, prm.c3, prm.cf, prm.cr, fl, hmax, grad_scale))
    with np.errstate(all="ignore"):
        D = ft(ok.sum())
        x = pi.reshape(M, 40, K)[rows, :, k].astype(ft)
        val = v[rows, np.minimum(k, V - 1)].astype(ft)
        old, A, T = old.astype(ft), adv.astype(ft), target.astype(ft)
        p = x[rows, c]
        den = np.where(old < e, e, old)
        ratio = np.where(p < e, e, p) / den
        lo, hi = one - clip, one + clip
        low = np.where(ratio < lo, lo, ratio)
        cl = np.where(low > hi, hi, low)
        ra, ca = ratio * A, cl * A
        pl = np.where(ca < ra, ca, ra)
        q = x + e
        l = np.log(np.where(q <= e, e, q))
        s = np.zeros(M, ft)
        for j in range(40):
            s = s + q[:, j] * l[:, j]
        H = -s
        under = fl - H
        bonus0 = H - cf * np.where(under < zero, zero, under)
        bonus = bonus0 + cr * (hmax - bonus0)
        rp = np.where(p >= e, one, zero) / den
        dpl = np.where(ra <= ca, A * rp, A * rp * np.where(cl == ratio, one, zero))
        ce = ((-(c3 / D)) * (one - cr)) * (one + np.where(H < fl, cf, zero))
        pp = (-(c2 / D)) * dpl
        ej = -(l + np.where(q > e, one, zero))
        g = ce[:, None] * ej
        g_entropy = g * gs
        g[rows, c] = g[rows, c] + pp
        g = g * gs
        dv = val - T
        gv = (((ft(2.0) * c1) * dv) / D) * gs
        terms = np.stack([dv * dv, pl, bonus, H, H * H, val, val * val, T, T * T, np.where(ratio != cl, one, zero), ratio], axis=1)
    res = dict(p=p, ratio=ratio, cl=cl, pl=pl, H=H, bonus=bonus, val=val, g=g, g_policy=pp * gs, g_entropy=g_entropy, ce=ce * gs, gv=gv, terms=terms)
    for name, a in res.items():
        a[~ok] = 0
    assert all(a.dtype == ft for a in res.values()), "an operation of the model left its float type"
    res.update(k=k, c=c, ok=ok, D=float(D), floor=float(fl), bonus0=bonus0, A=A, T=T)
    return res


def dqn_model(ft, Q, action, target, weight, valid, optimistic=0.0, grad_scale=1.0):
    """The DQN head in `ft` -> dict: q, prio, g [M, 40] (the piece's plane of grad_Q), k, c, ok, D, Dnz, terms [M, 6]"""
    M, K = Q.shape[0], Q.shape[3]
    k, c = indices(action, K)
    rows = np.arange(M)
    ok = np.ones(M, bool) if valid is None else valid != 0
    w = np.ones(M, ft) if weight is None else weight.astype(ft)
    zero, opt, gs = ft(0.0), ft(F32(optimistic)), ft(F32(grad_scale))
    with np.errstate(all="ignore"):
        D, Dnz = ft(ok.sum()), ft((ok & (w != 0)).sum())
        q = Q.reshape(M, 40, K)[rows, c, k].astype(ft)
        T = target.astype(ft)
        d = q - T
        prio = np.abs(d)
        if optimistic != 0.0:
            prio = prio + opt * np.where(prio < zero, zero, prio)
        gq = (((ft(2.0) * w) * d) / Dnz) * gs if Dnz > 0 else np.zeros(M, ft)
        terms = np.stack([w * (d * d), q, q * q, T, T * T, prio], axis=1)
    g = np.zeros((M, 40), ft)
    g[rows, c] = gq
    res = dict(q=q, prio=prio, g=g, terms=terms)
    for a in res.values():
        a[~ok] = 0
    assert all(a.dtype == ft for a in res.values()), "an operation of the model left its float type"
    res.update(k=k, c=c, ok=ok, D=float(D), Dnz=float(Dnz))
    return res


# ---------------------------------------------------------------- the reference's expressions with torch ops (float64, CPU)
def _masks(torch, action, K):
    a = torch.from_numpy(action.astype(np.int64))
    oh = torch.nn.functional.one_hot
    r_mask = oh(a[:, 0], 4).reshape(-1, 4, 1, 1).double()
    t_mask = oh(a[:, 1], 10).reshape(-1, 1, 10, 1).double()
    p_mask = oh(a[:, 2], K).reshape(-1, 1, 1, K).double()
    return r_mask * t_mask * p_mask, p_mask


def torch_ppo_loss(torch, pi, v, action, old, adv, target, rows, prm):
    """create_training_ops (ppo_nets.py:152-190) of the samples `rows`; pi, v are float64 leaf tensors -> the loss"""
    e = float(E32)
    floor, hmax = entropy_constants(prm.eps)
    clip, c1, c2, c3, cf, cr, floor, hmax = (float(F32(z)) for z in (prm.clip, prm.c1, prm.c2, prm.c3, prm.cf, prm.cr, floor, hmax))      # the float32 values a call carries
    K = pi.shape[3]
    rtp_mask, p_mask = _masks(torch, action, K)
    sel = torch.from_numpy(np.nonzero(rows)[0])
    policy, rtp_mask, p_mask = pi[sel], rtp_mask[sel], p_mask[sel]
    old_probs, advantages, target_values = (torch.from_numpy(a.astype(F64))[sel] for a in (old, adv, target))
    probability = (policy * rtp_mask).sum(dim=(1, 2, 3))
    values = (v[sel] * p_mask.reshape(-1, K)).sum(dim=1) if v.shape[1] == K else v[sel][:, 0]
    r = torch.clamp(probability, min=e) / torch.clamp(old_probs, min=e)
    clipped_r = torch.clamp(r, 1 - clip, 1 + clip)
    policy_loss = torch.minimum(r * advantages, clipped_r * advantages)
    x = policy + e
    action_entropy = ((-(x * torch.log(torch.clamp(x, min=e))).sum(dim=(1, 2), keepdim=True)) * p_mask).sum(dim=(1, 2, 3))
    entropy_bonus = action_entropy + cf * (-torch.relu(floor - action_entropy))
    entropy_bonus = entropy_bonus + cr * (hmax - entropy_bonus)
    return c1 * ((values - target_values) ** 2).mean() - c2 * policy_loss.mean() - c3 * entropy_bonus.mean()


def torch_dqn_loss(torch, Q, action, target, weight, rows):
    """prio_qnet.py:103-114 of the samples `rows`: tf.losses.mean_squared_error's SUM_BY_NONZERO_WEIGHTS reduction"""
    rtp_mask, _ = _masks(torch, action, Q.shape[3])
    sel = torch.from_numpy(np.nonzero(rows)[0])
    q_rtp = (Q[sel] * rtp_mask[sel]).sum(dim=(1, 2, 3))
    t = torch.from_numpy(target.astype(F64))[sel]
    w = torch.ones_like(t) if weight is None else torch.from_numpy(weight.astype(F64))[sel]
    return (w * (q_rtp - t) ** 2).sum() / (w != 0).sum()


# ---------------------------------------------------------------- inputs
def ppo_inputs(rng, M, K, V, dtype, masked, ties=True):
    """Inputs that reach every branch a batch of M samples can: maps rng.random ** 3 normalised per piece; with `ties` every 11th
    sample a one-hot map (zeros in the plane: p < e where the action is not the hot candidate) and every 13th a nearly uniform
    one; prob_old = p / f with f around 0.5, 1 and 2 (ratio below, inside and above any clip range used here), 0 and 5e-7 (< e)
    on some; advantages of both signs; r, t and piece out of range on some; with `masked` invalid samples at both ends and in the
    middle."""
    # (no entry in (0, 1e-10): there x + e rounds to e in float32, and the indicator [q > e] of the float64 formula is not the
    # float32 one)
    raw = np.maximum(rng.random((M, 40, K)) ** 3, 1e-8)
    rows = np.arange(M)
    if ties:
        flat = rows % 13 == 5
        raw[flat] = 1.0 + 0.01 * rng.random((int(flat.sum()), 40, K))
        hot = rows % 11 == 3
        raw[hot] = 0.0
        raw[hot, rng.integers(0, 40, int(hot.sum())), :] = 1.0
    pi = (raw / raw.sum(axis=1, keepdims=True)).reshape(M, 4, 10, K).astype(dtype)
    action = np.stack([rng.integers(0, 4, M), rng.integers(0, 10, M), rng.integers(0, K, M)], axis=1).astype(np.uint8)
    if ties:
        action[rows % 7 == 2, 0] = 200
        action[rows % 7 == 4, 1] = 77
        action[rows % 5 == 1, 2] = 250
        spare = np.nonzero(rows % 11 == 3)[0][::2]                  # half of the one-hot samples take their hot candidate
        k_, _ = indices(action, K)
        hot_c = pi.reshape(M, 40, K)[spare, :, k_[spare]].argmax(axis=1)
        action[spare, 0], action[spare, 1] = hot_c // 10, hot_c % 10
    k, c = indices(action, K)
    p = pi.reshape(M, 40, K)[rows, c, k].astype(F32)
    factor = np.choose(rows % 3, [0.5 + 0.2 * rng.random(M), 0.97 + 0.06 * rng.random(M), 1.6 + rng.random(M)])
    old = (np.maximum(p, E32) / factor).astype(F32)
    if ties:
        old[rows % 17 == 6] = 0.0
        old[rows % 17 == 9] = 5e-7
    adv = rng.standard_normal(M).astype(F32)
    target = rng.standard_normal(M).astype(F32)
    v = rng.standard_normal((M, V)).astype(dtype)
    valid = None
    if masked:
        valid = np.ones(M, np.uint8)
        valid[[0, M // 2, M - 1]] = 0
        valid[rows % 19 == 8] = 0
        valid[valid != 0] = rng.integers(1, 256, int((valid != 0).sum()))       # any non-zero byte counts
    return dict(pi=pi, v=v, action=action, old=old, adv=adv, target=target, valid=valid)


def dqn_inputs(rng, M, K, dtype, masked, weighted):
    Q = rng.standard_normal((M, 4, 10, K)).astype(dtype)
    rows = np.arange(M)
    action = np.stack([rng.integers(0, 4, M), rng.integers(0, 10, M), rng.integers(0, K, M)], axis=1).astype(np.uint8)
    action[rows % 7 == 2, 0] = 200
    action[rows % 7 == 4, 1] = 77
    action[rows % 5 == 1, 2] = 250
    target = rng.standard_normal(M).astype(F32)
    weight = valid = None
    if weighted:
        weight = rng.random(M).astype(F32)
        weight[rows % 6 == 1] = 0.0
    if masked:
        valid = np.ones(M, np.uint8)
        valid[[0, M // 2, M - 1]] = 0
        valid[rows % 19 == 8] = 0
    return dict(Q=Q, action=action, target=target, weight=weight, valid=valid)


# ---------------------------------------------------------------- calls
class PpoCall:
    """The buffers of one PPO call and the argument struct over them.  Outputs are pre-filled with the guard byte."""

    def __init__(self, kind, b, inp, prm, grad_dtype=F32, grad_scale=1.0, terms=True, floor=None, **override):
        pi, v = inp["pi"], inp["v"]
        M, K, V = pi.shape[0], pi.shape[3], v.shape[1]
        self.inp = {name: None if a is None else Buf(kind, a) for name, a in inp.items()}
        self.out = dict(grad_pi=out(kind, (M, 4, 10, K), grad_dtype), grad_v=out(kind, (M, V), grad_dtype), stats=out(kind, (16,), F32))
        if terms:
            self.out["terms"] = out(kind, (6, M), F32)
        p = lambda d, name: None if d.get(name) is None else d[name].ptr            # noqa: E731
        kw = dict(pi=p(self.inp, "pi"), v=p(self.inp, "v"), action=p(self.inp, "action"), prob_old=p(self.inp, "old"), adv=p(self.inp, "adv"),
                  target=p(self.inp, "target"), grad_pi=p(self.out, "grad_pi"), grad_v=p(self.out, "grad_v"), stats=p(self.out, "stats"), m=M,
                  n_pieces=K, n_values=V, valid=p(self.inp, "valid"), terms=p(self.out, "terms"), f16=pi.dtype == np.float16,
                  value_f16=v.dtype == np.float16, grad_f16=np.dtype(grad_dtype) == np.float16, clipping_parameter=prm.clip, value_loss=prm.c1,
                  policy_loss=prm.c2, entropy_loss=prm.c3, ppo_epsilon=prm.eps, entropy_floor_loss=prm.cf, rescaled_entropy=prm.cr,
                  entropy_floor=floor, grad_scale=grad_scale)
        kw.update(override)
        self.l = b.ppo_loss(**kw)

    def get(self):
        return {name: buf.get() for name, buf in self.out.items()}


class DqnCall:
    """The buffers of one DQN call and the argument struct over them"""

    def __init__(self, kind, b, inp, grad_dtype=F32, optimistic=0.0, grad_scale=1.0, **override):
        Q = inp["Q"]
        M, K = Q.shape[0], Q.shape[3]
        self.inp = {name: None if a is None else Buf(kind, a) for name, a in inp.items()}
        self.out = dict(grad_Q=out(kind, (M, 4, 10, K), grad_dtype), new_prio=out(kind, (M,), F32), q=out(kind, (M,), F32), stats=out(kind, (16,), F32))
        p = lambda d, name: None if d.get(name) is None else d[name].ptr            # noqa: E731
        kw = dict(Q=p(self.inp, "Q"), action=p(self.inp, "action"), target=p(self.inp, "target"), grad_Q=p(self.out, "grad_Q"),
                  new_prio=p(self.out, "new_prio"), stats=p(self.out, "stats"), m=M, n_pieces=K, weight=p(self.inp, "weight"),
                  valid=p(self.inp, "valid"), q=p(self.out, "q"), f16=Q.dtype == np.float16, grad_f16=np.dtype(grad_dtype) == np.float16,
                  optimistic_prios=optimistic, grad_scale=grad_scale)
        kw.update(override)
        self.l = b.dqn_loss(**kw)

    def get(self):
        return {name: buf.get() for name, buf in self.out.items()}


def same_bits(got, want):
    """equal as bit patterns, a zero of either sign being a zero"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    u = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    return np.array_equal((got + got.dtype.type(0)).view(u), (want + want.dtype.type(0)).view(u))


def written(a, want=None):
    """no element of an output buffer still holds the guard bytes it was filled with — but where `want`, the array the output is
    then compared with, holds that very pattern: of 65536 float16 values one does (-23.2), and a large gradient array meets it"""
    held = (a.view(np.uint8).reshape(-1, a.dtype.itemsize) == GUARD).all(axis=1)
    if want is not None:
        held &= ~(np.ascontiguousarray(want).view(np.uint8).reshape(-1, want.dtype.itemsize) == GUARD).all(axis=1)
    return not held.any()


def sum_bound(x):
    """the standard bound on the error of a float32 sum of the terms x in any order: (n - 1) 2^-24 sum |x_i|"""
    x = np.asarray(x, F64)
    return (max(len(x), 1) - 1) * U24 * np.abs(x).sum()


# ---------------------------------------------------------------- the stated order of a statistic's sum
BLOCK = 64                # samples of a block of the PPO / DQN heads (the planning head: plan_loss_support.BLOCK = 16)
SLOTS = 256               # LOSS_REDUCE_LANES of the header's sentence


def tree(v):
    """loss_tree over axis 0 of a copy of v (2^k rows): v[i] += v[i + off] for off = n/2, n/4, .., 1 -> row 0"""
    v = v.copy()
    off = v.shape[0] // 2
    assert 2 * off == v.shape[0] or v.shape[0] == 1, "a tree takes a power of two"
    while off >= 1:
        v[:off] = v[:off] + v[off:2 * off]
        off //= 2
    return v[0]


def stated_sum(terms, block, order="stated"):
    """The one model of "the order of a statistic's sum is fixed" (drl-tetris_amd/csrc/tetris_loss.h, STATISTICS), over axis 0 of
    terms [M] or [M, n], in the terms' float type: the samples of a block of `block` by the tree (samples past M add zeros), block
    b's row into slot b mod 256 — a slot starts at +0 — in ascending b, the 256 slots by the same tree.  Vectorised: the rows of a
    trip b = 256 i .. 256 i + 255 are added to the slots at once, trips in ascending i.
    `order` other than "stated" gives what a departure from the sentence would: "slotless" adds the rows in ascending b into one
    accumulator, "descending" adds them into their slots in descending b.  (Only the test of this model itself uses these.)"""
    terms = np.asarray(terms)
    flat = terms.reshape(terms.shape[0], -1)
    M, n = flat.shape
    nb = (M + block - 1) // block
    padded = np.zeros((nb * block, n), flat.dtype)
    padded[:M] = flat
    rows = tree(padded.reshape(nb, block, n).transpose(1, 0, 2))                 # [nb, n]: the blocks' partial rows
    if order == "slotless":
        total = np.zeros(n, flat.dtype)
        for b in range(nb):
            total = total + rows[b]
    else:
        slots = np.zeros((SLOTS, n), flat.dtype)
        trips = range(0, nb, SLOTS)
        for first in (trips if order == "stated" else reversed(trips)):
            part = rows[first:first + SLOTS]
            slots[:len(part)] = slots[:len(part)] + part
        total = tree(slots)
    assert total.dtype == terms.dtype
    return total.reshape(terms.shape[1:])


def stated_bound(x, block):
    """The bound on the error of a float32 sum of the terms x in the stated order.  Any path from a term to the total passes
    log2(block) additions of the block's tree (6 for PPO / DQN, 4 for the planning head), then the additions of its slot — one per
    trip, ceil(blocks / 256) of them, the first onto +0 —, then the 8 of the slots' tree; each addition rounds its result by at
    most 2^-24 of it, and no partial result exceeds sum |x_i| (1 + depth 2^-24).  To first order, which at depth <= 17 leaves out
    less than 2^-44 sum |x_i|, the error is at most depth 2^-24 sum |x_i|: (14 + ceil(blocks / 256)) 2^-24 sum |x_i| for a block
    of 64.  At M = 32833 (514 blocks, 3 trips) that is 1.0e-6 sum |x_i|, against 3.0e-5 sum |x_i| for one sample of equal terms and
    2.0e-3 sum |x_i| of the bound that holds for any order."""
    x = np.asarray(x, F64)
    blocks = (max(len(x), 1) + block - 1) // block
    depth = int(np.log2(block)) + (blocks + SLOTS - 1) // SLOTS + 8
    assert 2 ** int(np.log2(block)) == block
    return depth * U24 * np.abs(x).sum()


def loop_sum(terms, block):
    """The same sentence as plain Python loops over one column of float32 terms, a scalar at a time: for every block, for every
    level of the tree, for every pair.  (Slow: for the test of stated_sum.)"""
    M = len(terms)
    nb = (M + block - 1) // block
    slots = [F32(0.0)] * SLOTS
    for b in range(nb):                                              # ascending b
        v = [terms[b * block + t] if b * block + t < M else F32(0.0) for t in range(block)]
        off = block // 2
        while off >= 1:
            for i in range(off):
                v[i] = F32(v[i] + v[i + off])
            off //= 2
        slots[b % SLOTS] = F32(slots[b % SLOTS] + v[0])
    off = SLOTS // 2
    while off >= 1:
        for i in range(off):
            slots[i] = F32(slots[i] + slots[i + off])
        off //= 2
    return slots[0]


def ppo_stated_stats(terms, D, prm):
    """float32 [16]: the PPO statistics from the eleven per-sample float32 terms [M, 11] (ppo_model's `terms`), summed in the stated
    order and finished as the header's STATISTICS and PPO paragraphs write it, every operation in float32: c1 (total / D) and so on"""
    assert terms.dtype == F32 and terms.shape[1] == 11
    total = stated_sum(terms, BLOCK)
    stats = np.zeros(16, F32)
    D = F32(D)
    if not D > 0:
        return stats
    c1, c2, c3 = F32(prm.c1), F32(prm.c2), F32(prm.c3)
    vl, pol, ent = c1 * (total[0] / D), (-c2) * (total[1] / D), (-c3) * (total[2] / D)
    stats[:5] = D, (vl + pol) + ent, vl, pol, ent
    stats[5:14] = [total[col] / D for col in (3, 4, 2, 5, 6, 7, 8, 9, 10)]
    return stats


def dqn_stated_stats(terms, D, Dnz):
    """float32 [16]: the DQN statistics from the six per-sample float32 terms [M, 6] in the stated order"""
    assert terms.dtype == F32 and terms.shape[1] == 6
    total = stated_sum(terms, BLOCK)
    stats = np.zeros(16, F32)
    D, Dnz = F32(D), F32(Dnz)
    if not D > 0:
        return stats
    stats[:3] = D, Dnz, (total[0] / Dnz if Dnz > 0 else F32(0.0))
    stats[3:8] = [total[col] / D for col in (1, 2, 3, 4, 5)]
    return stats


# ---------------------------------------------------------------- batches whose loops take more than one trip
COUNT_LANES = 1024        # the lanes of the one workgroup that counts D and Dnz: a lane's trips are m, m + 1024, ..
CARRY_SIZES = (1025, 5123, 16385, 32833)      # 64 x 16 + 1, 5 x 1024 + 3, 64 x 256 + 1, 64 x 513 + 1


def carry_mask(rng, M, block, last_valid, span):
    """A valid mask for a batch whose count loop and whose reduction take more than one trip: the first sample invalid, every
    19th, the whole block 3, with `span` 1024 consecutive samples (every lane of the count has one trip that counts nothing; they
    start inside a block and inside a trip: at 1500, or at 0 where M leaves no other room), the last sample as `last_valid` says;
    any non-zero byte counts as valid."""
    rows = np.arange(M)
    valid = np.ones(M, np.uint8)
    valid[0] = 0
    valid[rows % 19 == 8] = 0
    valid[3 * block:4 * block] = 0
    if span:
        first = 1500 if M >= 1500 + COUNT_LANES + block else 0
        valid[first:first + COUNT_LANES] = 0
    valid[M - 1] = 1 if last_valid else 0
    valid[valid != 0] = rng.integers(1, 256, int((valid != 0).sum()))
    return valid


def weigh_the_full_slots(target, block):
    """Where a slot of the stated order takes three rows or more (more than 512 blocks), the targets of the blocks that share the
    fullest slots times 1024, in place.  Only in those slots can the order of a slot's rows show, and only in a last bit; 255 other
    slots of equal weight would round most such bits away in the slots' tree.  So the sums of T, T^2 and (val - T)^2 or
    w (q - T)^2 tell the stated order from another."""
    M = len(target)
    nb = (M + block - 1) // block
    trips = (nb + SLOTS - 1) // SLOTS
    if trips >= 3:
        b = np.arange(M) // block
        target[b % SLOTS < nb - SLOTS * (trips - 1)] *= F32(1024.0)
    return target


def assert_carry_mask(ok, block, last_valid, span):
    """what carry_mask promises, stated on the model's `ok`"""
    M = len(ok)
    assert not ok[0] and ok[M - 1] == last_valid
    nb = M // block
    assert (~ok[:nb * block].reshape(nb, block)).all(axis=1).any(), "no block without a valid sample"
    if span:
        gaps = np.diff(np.concatenate([[-1], np.nonzero(ok)[0], [M]])) - 1
        assert gaps.max() >= COUNT_LANES, "no 1024 consecutive samples without a valid one"
