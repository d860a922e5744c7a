"""The keyboard convolution (include/tetris_hip.h: tetris_kbd_conv_dev, tetris_kbd_conv_grad_x_dev, tetris_kbd_conv_grad_w_dev): a
float64 numpy model written from the header's definition — forward and the three gradients, and with the absolute values of its
inputs the sum of the magnitudes of every output's terms, which the tolerances need —, the reference's own lines
(agents/networks/builders/build_blocks.py:68-80) with torch ops for autograd in float64, the input makers, the tolerances with
their derivation, and the buffers of one call with the argument struct over them.  The model owes nothing to
drl-tetris_amd/csrc/tetris_kbd.h."""
import numpy as np

import __graft_entry__ as ge
from tests.buffers import PAD, Buf, out

F16, F32, F64, U8 = np.float16, np.float32, np.float64, np.uint8
U24 = 2.0 ** -24          # the relative error of one float32 rounding
T, WIDE, D, ROT = 10, 12, 3, 4


def capi():
    return ge.package().capi


# ---------------------------------------------------------------- the model (float64; exact on integers)
def to_channels(a, K):
    """[M, 4, 10, K] -> [M, 10, O]: o = r K + k"""
    M = a.shape[0]
    return np.ascontiguousarray(a.reshape(M, ROT, T, K).transpose(0, 2, 1, 3)).reshape(M, T, ROT * K)


def from_channels(y, K):
    """[M, 10, O] -> [M, 4, 10, K]: the four slices and the concat along the rotation axis"""
    M = y.shape[0]
    return np.ascontiguousarray(y.reshape(M, T, ROT, K).transpose(0, 2, 1, 3))


def forward(x, w, bias, K):
    """x [M, Hp, 12, C], w [Hp, 3, C, O], bias [O] -> out [M, 4, 10, K] = bias[o] + sum_h sum_d sum_c x[m][h][t + d][c] w[h][d][c][o]"""
    x, w = x.astype(F64), w.astype(F64)
    y = np.zeros((x.shape[0], T, w.shape[3]), F64) + bias.astype(F64)
    for d in range(D):
        y += np.einsum("mhtc,hco->mto", x[:, :, d:d + T, :], w[:, d], optimize=True)
    return from_channels(y, K)


def grad_x(g, w, K):
    """g [M, 4, 10, K], w -> [M, Hp, 12, C]: sum over d with 0 <= j - d <= 9, sum_o g[m][r][j - d][k] w[h][d][c][o]"""
    go, w = to_channels(g.astype(F64), K), w.astype(F64)
    gx = np.zeros((g.shape[0], w.shape[0], WIDE, w.shape[2]), F64)
    for d in range(D):
        gx[:, :, d:d + T, :] += np.einsum("mto,hco->mhtc", go, w[:, d], optimize=True)
    return gx


def grad_w(x, g, K):
    """-> [Hp, 3, C, O]: sum_m sum_t x[m][h][t + d][c] g[m][r][t][k]"""
    x, go = x.astype(F64), to_channels(g.astype(F64), K)
    return np.stack([np.einsum("mhtc,mto->hco", x[:, :, d:d + T, :], go, optimize=True) for d in range(D)], axis=1)


def grad_b(g, K):
    return to_channels(g.astype(F64), K).sum(axis=(0, 1))


def model(inp):
    """every output of the three calls -> dict(out, grad_x, grad_w, grad_b) in float64"""
    K = inp["K"]
    return dict(out=forward(inp["x"], inp["w"], inp["bias"], K), grad_x=grad_x(inp["g"], inp["w"], K), grad_w=grad_w(inp["x"], inp["g"], K),
                grad_b=grad_b(inp["g"], K))


def magnitudes(inp):
    """sum |terms| (+ |bias|) of every output: the model on the absolute values"""
    return model({k: (np.abs(v.astype(F64)) if isinstance(v, np.ndarray) else v) for k, v in inp.items()})


def terms(inp):
    """the number of terms of a sum of each output: 3 Hp C, at most 3 O <= 96, 10 M, 10 M"""
    M, Hp, _, C = inp["x"].shape
    return dict(out=D * Hp * C, grad_x=D * 4 * inp["K"], grad_w=T * M, grad_b=T * M)


# ---------------------------------------------------------------- the reference's lines with torch ops (float64, CPU, autograd)
def ref_keyboard_conv(x_nchw, kernel_hwio, bias, n_rot, n_p):
    """build_blocks.py:69-80 — conv2d 'valid' with a kernel (Hp, 3), the slices x[:, :, :, p * n_p:(p + 1) * n_p] of the NHWC result
    and their concat along axis 1.  x_nchw [M, C, Hp, 12] -> [M, 4, 10, K]"""
    import torch
    y = torch.nn.functional.conv2d(x_nchw, kernel_hwio.permute(3, 2, 0, 1), bias)          # [M, O, 1, 10]
    y = y.permute(0, 2, 3, 1)                                                                  # NHWC [M, 1, 10, O]
    return torch.cat([y[:, :, :, p * n_p:(p + 1) * n_p] for p in range(n_rot)], dim=1)


# ---------------------------------------------------------------- inputs
def integer_inputs(rng, M, Hp, C, K, dtype):
    """x, g in [-4, 4], w in [-3, 3], bias in [-8, 8], all integers and every one drawn on its own: every partial sum of any output in
    any order is an integer below 2^24, so a float32 accumulation of any order is exact"""
    O = ROT * K
    return dict(K=K, x=rng.integers(-4, 5, (M, Hp, WIDE, C)).astype(dtype), w=rng.integers(-3, 4, (Hp, D, C, O)).astype(dtype),
                bias=rng.integers(-8, 9, O).astype(F32), g=rng.integers(-4, 5, (M, ROT, T, K)).astype(dtype))


def grid_inputs(rng, M, Hp, C, K, dtype):
    """every value k / 64 with |k| <= 192: exact and normal (or zero) in binary16, products exact in float32"""
    O = ROT * K
    draw = lambda *s: rng.integers(-192, 193, s) / 64.0          # noqa: E731
    return dict(K=K, x=draw(M, Hp, WIDE, C).astype(dtype), w=draw(Hp, D, C, O).astype(dtype), bias=draw(O).astype(F32), g=draw(M, ROT, T, K).astype(dtype))


def rounded(a, dtype):
    """a float64 result rounded once, to nearest even, to the element type (binary16: overflow to infinity included)"""
    with np.errstate(over="ignore"):
        return a.astype(dtype)


# ---------------------------------------------------------------- tolerances
def bounds(inp, exact, dtype):
    """|got - exact| <= (n + 1) 2^-24 (sum |terms| + |bias|) + half a unit in the last place of the output's type, per element.
    A float32 sum of n terms in ANY order errs by at most (n - 1) u sum |terms| to first order (each of the n - 1 additions rounds a
    partial sum that is at most sum |terms| in magnitude); binary16 inputs on the grid have products that are exact in float32, so
    nothing else rounds; the bias is one more term; n + 1 covers the second-order part ((1 + u)^n - 1 <= (n + 1) u for n u < 0.01).
    float32 inputs: n + 2 (the matrix unit's float32 product is rounded once, u |term| each, which sums to u sum |terms|).  The
    output: binary16 half a unit = 2^-11 |exact| (2^-25 among the subnormals); float32 2^-24 |exact|; grad_w and grad_b are float32
    whatever the element type."""
    mag, n = magnitudes(inp), terms(inp)
    extra = 1 if np.dtype(dtype) == np.float16 else 2
    res = {}
    for name in exact:
        half = 2.0 ** -11 * np.abs(exact[name]) + 2.0 ** -25 if np.dtype(dtype) == np.float16 and name in ("out", "grad_x") else U24 * np.abs(exact[name])
        res[name] = (n[name] + extra) * U24 * mag[name] + half
    return res


# ---------------------------------------------------------------- calls
class KbdCall:
    """the buffers of the three calls (guard bytes behind every one, the outputs guard-filled) and the argument struct over them"""

    def __init__(self, kind, b, inp, offsets=None, **override):
        x, w = inp["x"], inp["w"]
        M, Hp, _, C = x.shape
        K, dt = inp["K"], x.dtype
        offsets = offsets or {}
        self.kind, self.M, self.K, self.dt = kind, M, K, dt
        self.ins = {n: Buf(kind, inp[n], offset=offsets.get(n, 0), guard=PAD) for n in ("x", "w", "bias", "g")}
        self.outs = dict(out=out(kind, (M, ROT, T, K), dt), grad_x=out(kind, x.shape, dt), grad_w=out(kind, w.shape, F32), grad_b=out(kind, (ROT * K,), F32))
        ptr = lambda name: self.outs[name].ptr + offsets.get(name, 0)             # noqa: E731
        kw = dict(m=M, height=Hp, channels=C, n_pieces=K, x=self.ins["x"].ptr, w=self.ins["w"].ptr, bias=self.ins["bias"].ptr,
                  grad_out=self.ins["g"].ptr, out=ptr("out"), grad_x=ptr("grad_x"), grad_w=ptr("grad_w"), grad_b=ptr("grad_b"),
                  f16=np.dtype(dt) == np.float16)
        kw.update(override)
        self.k = b.kbd_conv(**kw)

    def get(self, *names):
        res = {n: self.outs[n].get() for n in (names or self.outs)}
        for buf in self.ins.values():
            buf.get()                   # (asserts the guard bytes behind the inputs)
        return res


def run_all(kind, b, inp, **kw):
    """the three calls -> (call, dict of the four outputs)"""
    from tests.buffers import sync
    call = KbdCall(kind, b, inp, **kw)
    b.kbd_conv_dev(call.k)
    b.kbd_conv_grad_x_dev(call.k)
    b.kbd_conv_grad_w_dev(call.k)
    sync(kind, b)
    return call, call.get()


def untouched(buf):
    """whether a guard-filled output still holds nothing but guard bytes"""
    from tests.buffers import GUARD
    return bool((buf.get().view(U8) == GUARD).all())
