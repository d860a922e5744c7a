"""The network's output heads (include/tetris_hip.h: tetris_q_head_dev, tetris_policy_head_dev and their _grad_dev): a numpy
model written from the header's definition, operation by operation and vectorised over the samples — in float32 it follows the
order of every sum and gives the call's bits wherever no library call lies between input and output, in float64 it gives the numbers of
the reference —, the reference's own lines (agents/networks/network_utils.py:8-35, 95-104, 120-125) restated with torch ops for
autograd in float64, inputs with planted ties and extreme ranges, the tolerances with their derivation, and the buffers of one call
with the argument struct over them.  The model owes nothing to drl-tetris_amd/csrc/tetris_head.h."""
import numpy as np

import __graft_entry__ as ge
from tests.buffers import Buf, out

F16, F32, F64, U8 = np.float16, np.float32, np.float64, np.uint8
U24 = 2.0 ** -24          # the relative error of one float32 rounding
SAFETY = 4.0
# the documented bounds of the two library calls, in units in the last place: OpenCL's bounds, which the device library documents
# that it meets (tanh 5, exp 3); the host's libm stays below them (tanhf 2, expf 1)
TANH_ULP, EXP_ULP = 5.0, 3.0
ALL, SOME = 0x7F, 0b0100101          # all seven pieces; {0, 2, 5}
MODES = ("mean", "max", "none")


def capi():
    return ge.package().capi


def mask_bits(mask, K):
    return np.array([(mask >> k) & 1 for k in range(K)], bool)


def stored(x, dtype):
    """x as an array of the call's element type holds it (round to nearest even), widened again"""
    return x.astype(dtype).astype(x.dtype)


# ---------------------------------------------------------------- the model
def _max_j(x):
    """[M, 40, K] -> [M, K]: m = x_0; m = m < x_j ? x_j : m in ascending j"""
    m = x[:, 0]
    for j in range(1, 40):
        m = np.where(m < x[:, j], x[:, j], m)
    return m


def _min_j(x):
    m = x[:, 0]
    for j in range(1, 40):
        m = np.where(x[:, j] < m, x[:, j], m)
    return m


def _sum_j(x):
    """from +0 in ascending j"""
    s = np.zeros((x.shape[0], x.shape[2]), x.dtype)
    for j in range(40):
        s = s + x[:, j]
    return s


def _sum_k(x, used=None):
    """[M, K] -> [M]: from +0 in ascending k, the used k only"""
    s = np.zeros(x.shape[0], x.dtype)
    for k in range(x.shape[1]):
        if used is None or used[k]:
            s = s + x[:, k]
    return s


def q_value(ft, Q, mask):
    """V of the header from a stored Q [M, 40, K]: exact in float32"""
    Q = Q.astype(ft)
    used = mask_bits(mask, Q.shape[2])
    return _sum_k(_max_j(Q), used) / ft(used.sum())


def q_center(ft, a_raw, rho, mode, separate, mask):
    """-> dict(a, sub [M, K], eq_max [M, 40, K], eq_lo [M, 40, K], n_max [M, K], n_lo [M]): a = rho a_raw formed in float32 in
    both forms, so that both see the same ties"""
    M, _, K = a_raw.shape
    a = (a_raw.astype(F32) * F32(rho)).astype(ft)
    used = mask_bits(mask, K)
    U = ft(used.sum())
    r = dict(a=a, used=used, U=U, eq_max=np.zeros(a.shape, bool), eq_lo=np.zeros(a.shape, bool), n_max=np.ones((M, K), ft), n_lo=np.ones(M, ft))
    if mode == "mean":
        mu = _sum_j(a) / ft(40)
        c = _sum_k(mu, used) / U
        r["sub"] = np.repeat(c[:, None], K, axis=1)
    elif mode == "max":
        mn = _min_j(a)
        lo = mn[:, 0]
        for k in range(1, K):
            lo = np.where(mn[:, k] < lo, mn[:, k], lo)
        mx = np.where(used[None, :], _max_j(a), lo[:, None])
        r["eq_max"] = (a == mx[:, None, :]) & used[None, None, :]
        r["eq_lo"] = a == lo[:, None, None]
        r["n_max"] = np.maximum((a == mx[:, None, :]).sum(axis=1), 1).astype(ft)
        r["n_lo"] = r["eq_lo"].sum(axis=(1, 2)).astype(ft)
        c = _sum_k(np.where(used[None, :], mx, ft(0)), used) / U
        r["sub"] = mx if separate else np.repeat(c[:, None], K, axis=1)
        r["lo"] = lo
    else:
        r["sub"] = None
    return r


def _v_of(ft, v, M, K):
    if v is None:
        return np.zeros((M, K), ft)
    v = v.astype(ft)
    return v if v.shape[1] == K else np.repeat(v[:, :1], K, axis=1)


def q_forward(ft, a_raw, v, rho, mode, separate, mask, dtype):
    """a_raw [M, 40, K], v [M, Kv] or None -> dict(Q, A as `ft` before the rounding to the element type `dtype`, V from the stored
    Q, d, a and the tie sets)"""
    M, _, K = a_raw.shape
    r = q_center(ft, a_raw, rho, mode, separate, mask)
    d = r["a"] if r["sub"] is None else r["a"] - r["sub"][:, None, :]
    A = np.tanh(d)
    Q = _v_of(ft, v, M, K)[:, None, :] + A
    r.update(d=d, A=A, Q=Q, V=q_value(ft, stored(Q, dtype), mask))
    return r


def q_backward(ft, a_raw, G, rho, mode, separate, mask, Kv):
    """-> dict(grad_a [M, 40, K], grad_v [M, Kv] or None, gd, and q_center's fields)"""
    M, _, K = a_raw.shape
    r = q_center(ft, a_raw, rho, mode, separate, mask)
    used, U = r["used"], r["U"]
    a, G = r["a"], G.astype(ft)
    d = a if r["sub"] is None else a - r["sub"][:, None, :]
    A = np.tanh(d)
    sg = _sum_j(G)
    grad_v = None if not Kv else (sg if Kv == K else _sum_k(sg)[:, None])
    gd = G * (ft(1) - A * A)
    S_k = _sum_j(gd)
    S = _sum_k(S_k)
    ga = gd
    if mode == "mean":
        ga = np.where(used[None, None, :], gd - ((S / ft(40)) / U)[:, None, None], gd)
    elif mode == "max":
        share = S_k / r["n_max"] if separate else ((S / U)[:, None] / r["n_max"])
        ga = np.where(r["eq_max"], gd - share[:, None, :], gd)
        if separate:
            R = _sum_k(S_k, ~used)
            ga = np.where(r["eq_lo"], ga - (R / r["n_lo"])[:, None, None], ga)
    r.update(A=A, gd=gd, grad_a=ft(F32(rho)) * ga, grad_v=grad_v, S_k=S_k)
    return r


def policy_forward(ft, x, w):
    """x [M, 40, K], w [M, W] -> dict(pi [M, 40, K], v [M, 1 or K], z = x - mx)"""
    x, w = x.astype(ft), w.astype(ft)
    K, W = x.shape[2], w.shape[1]
    z = x - _max_j(x)[:, None, :]
    u = np.exp(z)
    pi = u / _sum_j(u)[:, None, :]
    if W == 1:
        v = np.tanh(w)
    else:
        c = _sum_k(w[:, 1:]) / ft(K)
        v = np.tanh(w[:, :1] + (w[:, 1:] - c[:, None]))
    return dict(pi=pi, v=v, z=z, u=u)


def policy_backward(ft, pi, v, g, gv, W):
    """from the stored outputs -> dict(grad_x, grad_w [M, W]); no library call: the float32 form gives the call's bits"""
    pi, v, g, gv = (t.astype(ft) for t in (pi, v, g, gv))
    K = pi.shape[2]
    dot = _sum_j(g * pi)
    grad_x = pi * (g - dot[:, None, :])
    gt = gv * (ft(1) - v * v)
    if W == 1:
        return dict(grad_x=grad_x, grad_w=gt)
    T = _sum_k(gt)
    return dict(grad_x=grad_x, grad_w=np.concatenate([T[:, None], gt - (T / ft(K))[:, None]], axis=1))


# ---------------------------------------------------------------- the reference's lines with torch ops (float64, CPU, autograd)
def ref_normalize_advantages(A, activation=None, inplace=False, mode="mean", axis=(1, 2), piece_axis=3, separate_piece_values=True,
                             piece_mask=1.0, n_used_pieces=7):
    """network_utils.py:8-35, line by line"""
    import torch
    if inplace:
        if A.shape[-1] == 1:
            return A if activation is None else activation(A)
        V = A[:, :, :, 0].unsqueeze(3)
        A = A[:, :, :, 1:]
    if isinstance(piece_mask, float) and piece_mask == 1.0:
        n_used_pieces = 1
    if mode == "max":
        all_axis = tuple(i + 1 for i in range(A.dim() - 1))
        a_maxmasked = piece_mask * A + (1 - piece_mask) * torch.amin(A, dim=all_axis, keepdim=True)
        _max_a = torch.amax(a_maxmasked, dim=axis, keepdim=True)
        if separate_piece_values:
            max_a = _max_a
        else:
            max_a = torch.sum(_max_a * piece_mask, dim=piece_axis, keepdim=True) / n_used_pieces
        A = A - max_a
    elif mode == "mean":
        _mean_a = torch.mean(A, dim=axis, keepdim=True)
        mean_a = torch.sum(_mean_a * piece_mask, dim=piece_axis, keepdim=True) / n_used_pieces
        A = A - mean_a
    if inplace:
        A = V + A
    if activation is not None:
        A = activation(A)
    return A


def ref_q_to_v(q, mask=1.0, n_used_pieces=7):
    import torch
    q_p = torch.amax(q, dim=(1, 2), keepdim=True)
    return (torch.sum(q_p * mask, dim=3, keepdim=True) / n_used_pieces).reshape(-1, 1)


def ref_mask(mask, K, like=None):
    """create_used_pieces_mask: (n_used_pieces, piece_mask), the mask on `like`'s device and of its type"""
    import torch
    if K == 1:
        return 1, 1.0
    bits = mask_bits(mask, K)
    piece_mask = torch.tensor(bits.astype(F64)).reshape(1, 1, 1, K)
    return int(bits.sum()), piece_mask if like is None else piece_mask.to(device=like.device, dtype=like.dtype)


def ref_qva(_V, _A, rho, mode, separate, mask):
    """base_architecture.py:53-62 -> qva_from_raw_streams: _A [M, 4, 10, K], _V broadcastable or 0"""
    import torch
    K = _A.shape[3]
    n_used, piece_mask = ref_mask(mask, K, _A)
    A = ref_normalize_advantages(rho * _A, activation=torch.tanh, separate_piece_values=separate, mode=mode, piece_mask=piece_mask,
                                 n_used_pieces=n_used)
    Q = _V + A
    return Q, ref_q_to_v(Q, mask=piece_mask, n_used_pieces=n_used), A


def ref_action_softmax(x):
    import torch
    max_x = torch.amax(x, dim=(1, 2), keepdim=True)
    pi_unnormalized = torch.exp(x - max_x)
    return pi_unnormalized / torch.sum(pi_unnormalized, dim=(1, 2), keepdim=True)


def ref_policy_value(w, mask, K):
    """ppo_nets' value: normalize_advantages(_V, tanh, axis=3, inplace=True, ...) of [M, 1, 1, W]"""
    import torch
    n_used, piece_mask = ref_mask(mask, K, w)
    return ref_normalize_advantages(w.reshape(-1, 1, 1, w.shape[1]), activation=torch.tanh, axis=3, inplace=True, piece_mask=piece_mask,
                                    n_used_pieces=n_used).reshape(w.shape[0], -1)


# ---------------------------------------------------------------- inputs
KINDS = ("free", "two_maxima", "equal_plane", "min_twice_used", "min_used_and_unused", "far_below", "far_above")


def q_inputs(rng, M, K, Kv, dtype, ties=True):
    """-> dict(a [M, 40, K], v [M, Kv] or None, G [M, 40, K], kind [M]) as `dtype`, every value a multiple of 2^-7 (a) or 2^-10
    (v, G) and so exact in binary16.  A sample's 40 K advantages are distinct multiples of 2^-7 in [-2, 2]: the two largest of a
    plane, and the two smallest of the sample, differ by at least 2^-7 (0.3 * 2^-7 > 2^-10).  With ties, sample m is of kind m % 7:
    0 as drawn; 1 two equal maxima in plane 0 (used by both masks) and in the last plane; 2 plane 0 all equal, and the last plane;
    3 the sample's minimum twice, both in piece 0 (used); 4 the minimum once in piece 0 (used) and once in piece 1 (unused by
    {0, 2, 5}); 5 one element at -30: d < -10 in every mode; 6 one element at +30: d > 10 under MEAN and NONE."""
    per = 40 * K
    a = np.stack([rng.permutation(513)[:per] - 256 for _ in range(M)]).reshape(M, 40, K).astype(F64) * 2.0 ** -7
    kind = np.zeros(M, int)
    if ties:
        kind = np.arange(M) % len(KINDS)
        for m in range(M):
            for k in sorted({0, K - 1}):
                j1, j2 = rng.choice(40, 2, replace=False)
                if kind[m] == 1:
                    a[m, j1, k] = a[m, j2, k] = a[m, :, k].max() + 0.5
                elif kind[m] == 2:
                    a[m, :, k] = a[m, j1, k]
            if kind[m] in (3, 4):
                j1, j2 = rng.choice(40, 2, replace=False)
                a[m, j1, 0] = a[m].min() - 0.25
                a[m, j2, 0 if kind[m] == 3 else min(1, K - 1)] = a[m, j1, 0]
            elif kind[m] == 5:
                a[m, rng.integers(40), rng.integers(K)] = -30.0
            elif kind[m] == 6:
                a[m, rng.integers(40), rng.integers(K)] = 30.0
    v = None if not Kv else rng.integers(-1024, 1025, (M, Kv)) * 2.0 ** -10
    G = rng.integers(-1024, 1025, (M, 40, K)) * 2.0 ** -10
    return dict(a=a.astype(dtype), v=None if v is None else v.astype(dtype), G=G.astype(dtype), kind=kind)


def policy_inputs(rng, M, K, W, dtype):
    """-> dict(x [M, 40, K], w [M, W], g [M, 40, K], gv [M, 1 or K], kind [M]) as `dtype`; sample m of kind m % 4: 0, 1 logits in
    [-4, 4]; 2 plane 0 spans -80 .. +80 (most of it underflows); 3 two equal maxima in plane 0 and a plane of equal logits"""
    x = rng.integers(-512, 513, (M, 40, K)) * 2.0 ** -7
    kind = np.arange(M) % 4
    for m in range(M):
        if kind[m] == 2:
            x[m, :, 0] = np.linspace(-80, 80, 40).round(2)[rng.permutation(40)]
        elif kind[m] == 3:
            x[m, :2, 0] = 5.0
            x[m, :, K - 1] = x[m, 0, K - 1]
    w = rng.integers(-2048, 2049, (M, W)) * 2.0 ** -10
    g = rng.integers(-1024, 1025, (M, 40, K)) * 2.0 ** -10
    gv = rng.integers(-1024, 1025, (M, 1 if W == 1 else K)) * 2.0 ** -10
    return dict(x=x.astype(dtype), w=w.astype(dtype), g=g.astype(dtype), gv=gv.astype(dtype), kind=kind)


# ---------------------------------------------------------------- tolerances
def half_ulp(x, dtype):
    """half a unit in the last place of the element type at |x| (binary16: 2^-11 |x|, 2^-25 among the subnormals); float32: 0 —
    its rounding is part of the bounds below"""
    return 2.0 ** -11 * np.abs(x) + 2.0 ** -25 if np.dtype(dtype) == np.float16 else 0.0 * np.abs(x)


def q_tolerances(m64, v, G=None):
    """Per-sample bounds [M] on |float32 result - exact result| of the Q head, u = 2^-24, for inputs that are exact in both.
      d: a = rho a_raw is one float32 product in both models, no error.  What is subtracted is at worst the MEAN's c: 40 additions
        per plane, a division, 7 additions, a division — each rounding at most u of a magnitude <= amax = max |a| of the sample:
        49 u amax; the subtraction rounds by u |d| <= 2 u amax.  E_d = 51 u amax.  (MAX: maxima are exact, at most 9 roundings.)
      A = tanhf(d): |tanh'| <= 1 hands E_d on; the library adds TANH_ULP units in the last place of a number below 1, u each.
        E_A = E_d + TANH_ULP u.
      Q = v + A: one rounding of a magnitude <= |v| + 1.  E_Q = E_A + u (vmax + 1).
      gd = G (1 - A A): 2 |A| E_A <= 2 E_A, three roundings of magnitudes <= 1:  |gd error| <= |G| E_g, E_g = 2 E_A + 3 u.
      A sum of n terms x_i with errors e_i in float32: sum e_i + (n - 1) u sum |x_i| (sum_bound).  Every share is such a sum of at
        most all 280 gd, divided by numbers >= 1 twice: E_S = E_g sum |G| + 279 u sum |gd| + 2 u sum |gd|.
      ga = gd - share - rshare, times rho: E_ga = Gmax E_g + 2 E_S + 4 u (Gmax + 2 sum |gd|).
      grad_v: sums of G alone: 279 u sum |G|.
    Each times SAFETY = 4 for what the count simplifies.  -> dict(A, Q, grad_a, grad_v)"""
    a = np.abs(m64["a"])
    M = a.shape[0]
    amax = a.reshape(M, -1).max(axis=1)
    E_A = 51 * U24 * amax + TANH_ULP * U24
    vmax = 0.0 if v is None else np.abs(v.astype(F64)).max(axis=1)
    tol = dict(A=SAFETY * E_A, Q=SAFETY * (E_A + U24 * (vmax + 1)))
    if G is not None:
        G = np.abs(G.astype(F64)).reshape(M, -1)
        gd = np.abs(m64["gd"]).reshape(M, -1).sum(axis=1)
        E_g = 2 * E_A + 3 * U24
        E_S = E_g * G.sum(axis=1) + 281 * U24 * gd
        tol["grad_a"] = SAFETY * (G.max(axis=1) * E_g + 2 * E_S + 4 * U24 * (G.max(axis=1) + 2 * gd))
        tol["grad_v"] = SAFETY * 279 * U24 * G.sum(axis=1)
    return tol


def policy_tolerances(m64, w):
    """Bounds on the policy head's forward, u = 2^-24.
      z = x - mx: one rounding, u |z|.  u_jk = expf(z): relative error |z| u from the argument and EXP_ULP units in the last place,
        2 u each, from the library: (|z| + 2 EXP_ULP) u.  s_k is a sum of 40 positive terms: the largest relative error of a term
        plus 39 u.  pi = u_jk / s_k: both relative errors and one rounding:  pi (2 (zmax + 2 EXP_ULP) + 40) u with zmax the largest
        |z| of the plane, and 2^-149 where the result is subnormal or underflows.  [M, 1, K]
      sum_j pi_jk = 1: 40 such errors (they are relative: their sum is the bound at pi = 1) and the 39 roundings of the check's sum.
      v = tanhf(w_0 + (w_k - c)): c has K additions and a division, the argument two more roundings, magnitudes <= 2 wmax:
        (K + 3) 2 wmax u; TANH_ULP u from the library.  [M]
    Each times SAFETY = 4.  -> dict(pi, v)"""
    zmax = np.abs(m64["z"]).max(axis=1, keepdims=True)
    rel = (2 * (zmax + 2 * EXP_ULP) + 40) * U24
    K = m64["pi"].shape[2]
    wmax = np.abs(w.astype(F64)).max(axis=1)
    return dict(pi=SAFETY * (m64["pi"] * rel + 2.0 ** -149), pi_sum=SAFETY * (rel[:, 0, :] + 39 * U24),
                v=SAFETY * ((K + 3) * 2 * wmax * U24 + TANH_ULP * U24))


# ---------------------------------------------------------------- calls
class QCall:
    """the buffers of one Q-head call (forward and backward outputs, guard-filled) and the argument struct over them"""

    def __init__(self, kind, b, inp, mode="mean", rho=1.0, separate=True, mask=None, want_A=True, offsets=None, **override):
        a = inp["a"]
        M, K = a.shape[0], a.shape[2]
        dt = a.dtype
        offsets = offsets or {}
        self.kind, self.M, self.K, self.dt = kind, M, K, dt
        self.a, self.G = Buf(kind, a, offset=offsets.get("a", 0)), Buf(kind, inp["G"], offset=offsets.get("G", 0))
        self.v = None if inp["v"] is None else Buf(kind, inp["v"])
        Kv = 0 if inp["v"] is None else inp["v"].shape[1]
        vdt = dt if inp["v"] is None else inp["v"].dtype
        self.outs = dict(Q=out(kind, (M, 40, K), dt), V=out(kind, (M,), F32), grad_a=out(kind, (M, 40, K), dt))
        if want_A:
            self.outs["A"] = out(kind, (M, 40, K), dt)
        if Kv:
            self.outs["grad_v"] = out(kind, (M, Kv), vdt)
        ptr = lambda name: self.outs[name].ptr + offsets.get(name, 0) if name in self.outs else None          # noqa: E731
        kw = dict(a=self.a.ptr, m=M, v=self.v.ptr if self.v else None, n_pieces=K, n_values=Kv or 1, mode=mode, advantage_range=rho,
                  separate_piece_values=separate, used_pieces=(ALL if K == 7 else 1) if mask is None else mask,
                  f16=np.dtype(dt) == np.float16, value_f16=np.dtype(vdt) == np.float16, Q=ptr("Q"), V=ptr("V"), A=ptr("A"),
                  grad_Q=self.G.ptr, grad_a=ptr("grad_a"), grad_v=ptr("grad_v"))
        kw.update(override)
        self.h = b.q_head(**kw)

    def get(self, *names):
        return {n: self.outs[n].get() for n in (names or self.outs)}


class PolicyCall:
    """the buffers of one policy-head call: forward writes pi, v; backward reads `pi`, `v` (as given, or what forward left) and g, gv"""

    def __init__(self, kind, b, inp, offsets=None, **override):
        x, w = inp["x"], inp["w"]
        M, K, W = x.shape[0], x.shape[2], w.shape[1]
        dt, vdt = x.dtype, w.dtype
        offsets = offsets or {}
        self.kind, self.M, self.K, self.W, self.dt = kind, M, K, W, dt
        self.x, self.w = Buf(kind, x, offset=offsets.get("x", 0)), Buf(kind, w)
        self.g, self.gv = Buf(kind, inp["g"], offset=offsets.get("g", 0)), Buf(kind, inp["gv"])
        self.outs = dict(pi=out(kind, (M, 40, K), dt), v=out(kind, (M, 1 if W == 1 else K), vdt), grad_x=out(kind, (M, 40, K), dt),
                         grad_w=out(kind, (M, W), vdt))
        ptr = lambda name: self.outs[name].ptr + offsets.get(name, 0)             # noqa: E731
        kw = dict(m=M, pi=ptr("pi"), v=ptr("v"), n_pieces=K, n_values=W, x=self.x.ptr, w=self.w.ptr, grad_pi=self.g.ptr, grad_v=self.gv.ptr,
                  grad_x=ptr("grad_x"), grad_w=ptr("grad_w"), f16=np.dtype(dt) == np.float16, value_f16=np.dtype(vdt) == np.float16)
        kw.update(override)
        self.h = b.policy_head(**kw)

    def get(self, *names):
        return {n: self.outs[n].get() for n in (names or self.outs)}


def untouched(buf):
    """whether a guard-filled output still holds nothing but guard bytes"""
    from tests.buffers import GUARD
    return bool((buf.get().view(U8) == GUARD).all())
