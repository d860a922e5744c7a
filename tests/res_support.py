"""One residual layer (include/tetris_hip.h: tetris_res_layer_dev, tetris_res_layer_grad_x_dev, tetris_res_layer_grad_w_dev): a float64
numpy model written from the header's definition — forward and the three gradients, and with the absolute values of its inputs the
sum of the magnitudes of every output's terms, which the tolerances need —, the reference's own lines
(agents/networks/builders/build_blocks.py:43-57, agents/networks/network_utils.py:52-64) with torch ops for autograd in float64, the
input makers, the tolerances with their derivation, and the buffers of one call with the argument struct over them.  The model
owes nothing to drl-tetris_amd/csrc/tetris_res.h."""
import numpy as np

import __graft_entry__ as ge
from tests.buffers import PAD, Buf, out

F16, F32, F64, U8 = np.float16, np.float32, np.float64, np.uint8
U24 = 2.0 ** -24          # the relative error of one float32 rounding
WIDE = 12
EXPM1_ULP = 3             # float32 units in the last place: OpenCL's bound for expm1, which the device library documents that it meets
JOINS, ACTS = ("none", "add", "truncate_add"), ("none", "elu")


def capi():
    return ge.package().capi


def cout(Ci, Co, join):
    return Co if join == "none" else max(Ci, Co) if join == "add" else min(Ci, Co)


# ---------------------------------------------------------------- the model (float64; exact on integers)
def conv_same(x, w):
    """x [M, Hp, 12, Ci], w [3, 3, Ci, Co] -> sum_(a, b) sum_ci x[m][h + a - 1][j + b - 1][ci] w[a][b][ci][o], x = 0 outside"""
    M, Hp, Wd, _ = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    z = np.zeros((M, Hp, Wd, w.shape[3]), F64)
    for a in range(3):
        for b in range(3):
            z += np.einsum("mhjc,co->mhjo", xp[:, a:a + Hp, b:b + Wd, :], w[a, b], optimize=True)
    return z


def pre_activation(x, w, bias, join):
    """p [M, Hp, 12, Cout] = (c < Co ? z[c] : 0) + (join and c < Ci ? x[c] : 0)"""
    x, w = x.astype(F64), w.astype(F64)
    Ci, Co = w.shape[2], w.shape[3]
    Cout = cout(Ci, Co, join)
    z = conv_same(x, w) + bias.astype(F64)
    p = np.zeros(x.shape[:3] + (Cout,), F64)
    p[..., :min(Co, Cout)] += z[..., :min(Co, Cout)]
    if join != "none":
        p[..., :min(Ci, Cout)] += x[..., :min(Ci, Cout)]
    return p


def forward(x, w, bias, join, act):
    p = pre_activation(x, w, bias, join)
    return np.where(p > 0, p, np.expm1(np.minimum(p, 0))) if act == "elu" else p


def e_of(g, y, act, dtype=None):
    """e = g (ELU and y <= 0 ? y + 1 : 1), rounded to dtype where one is given"""
    g = g.astype(F64)
    e = g * np.where(y.astype(F64) <= 0, y.astype(F64) + 1.0, 1.0) if act == "elu" else g
    return e.astype(dtype).astype(F64) if dtype is not None and np.dtype(dtype) == np.float16 else e


def gradients(x, w, e, join):
    """x [M, Hp, 12, Ci] (or None), w [3, 3, Ci, Co], e [M, Hp, 12, Cout] -> grad_x, grad_w, grad_b of sum g out"""
    w = w.astype(F64)
    Ci, Co = w.shape[2], w.shape[3]
    M, Hp, Wd, Cout = e.shape
    Cz = min(Co, Cout)
    gz = e[..., :Cz]
    gp = np.pad(gz, ((0, 0), (1, 1), (1, 1), (0, 0)))
    gx = np.zeros((M, Hp, Wd, Ci), F64)
    for a in range(3):
        for b in range(3):
            gx += np.einsum("mhjo,co->mhjc", gp[:, 2 - a:2 - a + Hp, 2 - b:2 - b + Wd, :], w[a, b][:, :Cz], optimize=True)
    if join != "none":
        gx[..., :min(Ci, Cout)] += e[..., :min(Ci, Cout)]
    res = dict(grad_x=gx)
    if x is not None:
        xp = np.pad(x.astype(F64), ((0, 0), (1, 1), (1, 1), (0, 0)))
        gw = np.zeros((3, 3, Ci, Co), F64)
        for a in range(3):
            for b in range(3):
                gw[a, b, :, :Cz] = np.einsum("mhjc,mhjo->co", xp[:, a:a + Hp, b:b + Wd, :], gz, optimize=True)
        gb = np.zeros(Co, F64)
        gb[:Cz] = gz.sum(axis=(0, 1, 2))
        res.update(grad_w=gw, grad_b=gb)
    return res


def model(inp, round_e=True):
    """every output of the three calls -> dict(out, grad_x, grad_w, grad_b) in float64.  round_e=False leaves e unrounded (the
    tolerances then carry its rounding)."""
    res = dict(out=forward(inp["x"], inp["w"], inp["bias"], inp["join"], inp["act"]))
    res.update(gradients(inp["x"], inp["w"], e_of(inp["g"], inp["y"], inp["act"], inp["x"].dtype if round_e else None), inp["join"]))
    return res


def magnitudes(inp, e=None):
    """sum |terms| (+ |bias|) of every output: the model on the absolute values, e = |e| (or the array given)"""
    ax, aw = np.abs(inp["x"].astype(F64)), np.abs(inp["w"].astype(F64))
    res = dict(out=pre_activation(ax, aw, np.abs(inp["bias"]), inp["join"]))
    res.update(gradients(ax, aw, np.abs(e_of(inp["g"], inp["y"], inp["act"])) if e is None else e, inp["join"]))
    return res


def terms(inp):
    """the number of terms of a sum of each output: 9 Ci + 2 (bias and the join's term), 9 Co + 1, 12 Hp M"""
    M, Hp, _, Ci = inp["x"].shape
    Co = inp["w"].shape[3]
    return dict(out=9 * Ci + 2, grad_x=9 * Co + 1, grad_w=WIDE * Hp * M, grad_b=WIDE * Hp * M)


# ---------------------------------------------------------------- the reference's lines with torch ops (float64, CPU, autograd)
def ref_peephole_join(x, y, mode):
    """network_utils.py:52-64 on NHWC tensors"""
    import torch
    nx, ny = x.shape[3], y.shape[3]
    larger = x if nx > ny else y
    smaller = y if nx > ny else x
    s = larger[:, :, :, :smaller.shape[3]] + smaller
    rest = larger[:, :, :, smaller.shape[3]:]
    return torch.cat([s, rest] if mode == "add" else [s], dim=-1)


def ref_residual_layer(x_nchw, kernel_hwio, bias, join, act):
    """build_blocks.py:43-57 — conv2d 3 x 3 'same', peephole_join(x, y, mode), elu.  x_nchw [M, Ci, Hp, 12] -> NHWC [M, Hp, 12, Cout]"""
    import torch
    z = torch.nn.functional.conv2d(x_nchw, kernel_hwio.permute(3, 2, 0, 1), bias, padding=1).permute(0, 2, 3, 1)
    if join != "none":
        z = ref_peephole_join(z, x_nchw.permute(0, 2, 3, 1), join)
    return torch.nn.functional.elu(z) if act == "elu" else z


# ---------------------------------------------------------------- inputs
ELU_YS = np.array([-0.75, -0.5, -0.25, 0.0, 1.0, 2.0])


def integer_inputs(rng, M, Hp, Ci, Co, join, act, dtype):
    """x, g in [-4, 4], w in [-3, 3], bias in [-8, 8], all integers and every one drawn on its own; y (read with ELU only) from
    {-0.75, -0.5, -0.25, 0, 1, 2}, so that e is a multiple of 0.25, exact in binary16.  Every partial sum of any output in any order
    is a multiple of 0.25 below 2^24 in magnitude: a float32 accumulation of any order is exact."""
    Cout = cout(Ci, Co, join)
    return dict(join=join, act=act, x=rng.integers(-4, 5, (M, Hp, WIDE, Ci)).astype(dtype), w=rng.integers(-3, 4, (3, 3, Ci, Co)).astype(dtype),
                bias=rng.integers(-8, 9, Co).astype(F32), g=rng.integers(-4, 5, (M, Hp, WIDE, Cout)).astype(dtype),
                y=ELU_YS[rng.integers(0, len(ELU_YS), (M, Hp, WIDE, Cout))].astype(dtype))


def grid_inputs(rng, M, Hp, Ci, Co, join, act, dtype, w_div=64.0):
    """every value k / 64 with |k| <= 192 (kbd_support.grid_inputs' grid): exact and normal (or zero) in binary16, products exact in
    float32; y is the model's own output rounded to the element type — an input of the gradient calls like any other"""
    Cout = cout(Ci, Co, join)
    draw = lambda *s: rng.integers(-192, 193, s) / 64.0          # noqa: E731
    inp = dict(join=join, act=act, x=draw(M, Hp, WIDE, Ci).astype(dtype), w=(draw(3, 3, Ci, Co) * (64.0 / w_div)).astype(dtype),
               bias=draw(Co).astype(F32), g=draw(M, Hp, WIDE, Cout).astype(dtype))
    inp["y"] = rounded(forward(inp["x"], inp["w"], inp["bias"], join, act), dtype)
    return inp


def rounded(a, dtype):
    """a float64 result rounded once, to nearest even, to the element type (binary16: overflow to infinity included)"""
    with np.errstate(over="ignore"):
        return a.astype(dtype)


# ---------------------------------------------------------------- tolerances
def bounds(inp, exact, dtype):
    """|got - exact| per element, `exact` being model(inp, round_e=False).
    The sums: kbd_support.bounds' derivation carries over.  A float32 sum of n terms in ANY order errs by at most (n - 1) u
    sum |terms| to first order, u = 2^-24; binary16 inputs on the grid have products that are exact in float32; n + 1 covers the
    second-order part; float32 inputs: n + 2 (the matrix unit's float32 product is rounded once).  n = 9 Ci + 2 for out (bias and
    the join's term), 9 Co + 1 for grad_x, 12 Hp M for grad_w and grad_b.
    out: ELU is 1-Lipschitz, so the bound on p carries to out; where p <= 0, EXPM1_ULP float32 units of |out| are added — OpenCL's
    bound for expm1, which the device library documents that it meets.  "Where p <= 0" is taken at the device's own p, which lies
    within the bound on p of the exact one: the elements with exact p - bound(p) <= 0; and |out| there is |exact| plus that bound.
    The gradients: the device's e differs from the exact g (y + 1).  In float32 by one rounding, u |e|: the product is formed as
    fma(g, y, g), y + 1 itself is not rounded.  In binary16 the same float32 rounding (u |e|) and then the rounding to binary16,
    half a binary16 unit of e — 2^-11 |e|, or 2^-25 among the subnormals.  Each term of a gradient's sum carries that error times
    its other factor: the gradient sums evaluated on the error of e in place of e.
    The output: binary16 half a unit = 2^-11 |exact| (2^-25 among the subnormals); float32 2^-24 |exact|; grad_w and grad_b are
    float32 whatever the element type.
    This bound would hide a single missing term where the integer test does not."""
    half16 = np.dtype(dtype) == np.float16
    mag, n = magnitudes(inp), terms(inp)
    extra = 1 if half16 else 2
    abs_e = np.abs(e_of(inp["g"], inp["y"], inp["act"]))
    e_err = ((2.0 ** -11 + U24) * abs_e + 2.0 ** -25) if half16 else U24 * abs_e
    if inp["act"] != "elu":
        e_err = np.zeros_like(abs_e)          # e is g itself
    mag_e = magnitudes(inp, e=e_err)
    res = {}
    for name in exact:
        half = 2.0 ** -11 * np.abs(exact[name]) + 2.0 ** -25 if half16 and name in ("out", "grad_x") else U24 * np.abs(exact[name])
        res[name] = (n[name] + extra) * U24 * mag[name]
        if name == "out":
            if inp["act"] == "elu":
                p = pre_activation(inp["x"], inp["w"], inp["bias"], inp["join"])
                res[name] += np.where(p - res[name] <= 0, EXPM1_ULP * U24 * (np.abs(exact[name]) + res[name]), 0.0)
            res[name] += half
        else:
            res[name] += mag_e[name] + half
    return res


# ---------------------------------------------------------------- calls
class ResCall:
    """the buffers of the three calls (guard bytes behind every one, the outputs guard-filled) and the argument struct over them"""

    def __init__(self, kind, b, inp, offsets=None, **override):
        x, w = inp["x"], inp["w"]
        M, Hp, _, Ci = x.shape
        Co, dt = w.shape[3], x.dtype
        offsets = offsets or {}
        self.kind, self.M, self.dt = kind, M, dt
        self.ins = {n: Buf(kind, inp[n], offset=offsets.get(n, 0), guard=PAD) for n in ("x", "w", "bias", "g", "y")}
        self.outs = dict(out=out(kind, inp["g"].shape, dt), grad_x=out(kind, x.shape, dt), grad_w=out(kind, w.shape, F32), grad_b=out(kind, (Co,), F32))
        ptr = lambda name: self.outs[name].ptr + offsets.get(name, 0)             # noqa: E731
        kw = dict(m=M, height=Hp, in_channels=Ci, out_channels=Co, join=inp["join"], activation=inp["act"], x=self.ins["x"].ptr,
                  w=self.ins["w"].ptr, bias=self.ins["bias"].ptr, y=self.ins["y"].ptr, grad_out=self.ins["g"].ptr, out=ptr("out"),
                  grad_x=ptr("grad_x"), grad_w=ptr("grad_w"), grad_b=ptr("grad_b"), f16=np.dtype(dt) == np.float16)
        kw.update(override)
        self.k = b.res_layer(**kw)

    def get(self, *names):
        res = {n: self.outs[n].get() for n in (names or self.outs)}
        for buf in self.ins.values():
            buf.get()                   # (asserts the guard bytes behind the inputs)
        return res


def run_all(kind, b, inp, **kw):
    """the three calls -> (call, dict of the four outputs)"""
    from tests.buffers import sync
    call = ResCall(kind, b, inp, **kw)
    b.res_layer_dev(call.k)
    b.res_layer_grad_x_dev(call.k)
    b.res_layer_grad_w_dev(call.k)
    sync(kind, b)
    return call, call.get()


def untouched(buf):
    """whether a guard-filled output still holds nothing but guard bytes"""
    from tests.buffers import GUARD
    return bool((buf.get().view(U8) == GUARD).all())
