"""The keyboard convolution on the device (include/tetris_hip.h: tetris_kbd_conv_dev, tetris_kbd_conv_grad_x_dev,
tetris_kbd_conv_grad_w_dev) against the model of tests/kbd_support.py, written from the header's definition: 1. the float64 model
against float64 torch autograd of the reference's own lines; 2. integer inputs, whose sums are exact in float32 in any order: bit
equality with the integer model — the structural test; 3. general values within a derived tolerance of the float64 model; 4. a second
call gives the same bytes; 5. the argument rules and untouched buffers; 7. on the GPU TorchEnv.keyboard_conv inside a small training
step.  (6. is the stand-alone sanitizer program tests/sanitizers/kbd_main.cpp.)  Every group but the first and the last runs on the
CPU harness (`-m "not gpu"`) and on the MI355X (`-m gpu`); on the harness the "device" buffers are numpy arrays."""
import importlib
import itertools

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import engines
from tests.buffers import GUARD, sync
from tests.kbd_support import (D, F16, F32, F64, ROT, T, WIDE, KbdCall, bounds, capi, grid_inputs, integer_inputs, model, ref_keyboard_conv,
                               rounded, run_all, untouched)

TYPES = (F32, F16)
HPS, CS, KS = (4, 5, 6, 22, 33), (32, 96, 128, 160, 512), (1, 3, 7)


def block():
    return capi().KBD_BLOCK


def partial():
    return capi().KBD_W_SAMPLES


def _cases():
    """(M, Hp, C, K, dtype): every M around the workgroup's block with both element types; Hp, C and K rotate with indices of their
    own, so that none of them is tied to M, to the type or to another; then every Hp, C and K that the rotation left out of an
    element type, at M = 17 (a partial second block); then M around the samples per partial of grad_w, at C = 32, Hp = 6."""
    B, P = 16, 256
    assert (B, P) == (block(), partial()), "the cases are laid out for these constants of tetris_kbd.h"
    cases = []
    for n, ((mi, M), (ti, dt)) in enumerate(itertools.product(enumerate((1, B - 1, B, B + 1, 2 * B + 1)), enumerate(TYPES))):
        cases.append((M, HPS[(n + mi) % 5], CS[(2 * n + ti + 3) % 5], KS[(n + mi + ti) % 3], dt))
    for ti, dt in enumerate(TYPES):
        for i in range(5):
            cases.append((17 if CS[(i + 2 * ti) % 5] < 512 else 3, HPS[i], CS[(i + 2 * ti) % 5], KS[(i + ti) % 3], dt))
    for i, M in enumerate((P - 1, P, P + 1, 2 * P + 1)):
        cases.append((M, 6, 32, KS[i % 3], TYPES[i % 2]))
        cases.append((M, 6, 32, KS[(i + 1) % 3], TYPES[(i + 1) % 2]))
    return list(dict.fromkeys(cases))


CASES = _cases()


def case_id(c):
    return f"M{c[0]}-Hp{c[1]}-C{c[2]}-K{c[3]}-{np.dtype(c[4]).name}"


@pytest.fixture(scope="module")
def batch_of():
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = engines.make(kind, 4, 1, 8)
        return made[kind]
    yield get
    for b in made.values():
        b.close()


def written(a):
    """every element of an output was written: none still holds the guard pattern"""
    return not (a.view(np.uint8).reshape(-1, a.dtype.itemsize) == GUARD).all(axis=1).any()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- 1. the float64 model against autograd of the reference's lines
# Tolerance.  Both sides form the same n products exactly alike (one rounding each, the same) and add them in different orders: each
# of at most n additions rounds a partial sum of magnitude <= S = sum |terms| + |bias| by at most 2^-53 S.  Two sides, and the
# products' own roundings where the libraries fuse them: 4 (n + 1) 2^-53 S per element, n = 3 Hp C, 3 O or 10 M.
@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("C", [32, 128])
@pytest.mark.parametrize("Hp", [5, 22])
def test_the_float64_model_against_torch_autograd(Hp, C, K):
    import torch
    M, O = 5, ROT * K
    rng = np.random.default_rng(Hp * 1000 + C + K)
    inp = dict(K=K, x=rng.standard_normal((M, Hp, WIDE, C)), w=rng.standard_normal((Hp, D, C, O)), bias=rng.standard_normal(O),
               g=rng.standard_normal((M, ROT, T, K)))
    x = torch.tensor(inp["x"]).permute(0, 3, 1, 2).contiguous().requires_grad_()              # NCHW
    w, bias = torch.tensor(inp["w"]).requires_grad_(), torch.tensor(inp["bias"]).requires_grad_()
    y = ref_keyboard_conv(x, w, bias, ROT, K)
    gx, gw, gb = torch.autograd.grad(y, (x, w, bias), torch.tensor(inp["g"]))
    want = dict(out=y.detach().numpy(), grad_x=gx.permute(0, 2, 3, 1).numpy(), grad_w=gw.numpy(), grad_b=gb.numpy())
    got = model(inp)
    mag = model({k: np.abs(v) if isinstance(v, np.ndarray) else v for k, v in inp.items()})
    n = dict(out=D * Hp * C, grad_x=D * O, grad_w=T * M, grad_b=T * M)
    for name in got:
        err, tol = np.abs(got[name] - want[name]), 4 * (n[name] + 1) * 2.0 ** -53 * mag[name]
        assert got[name].shape == want[name].shape and (err <= tol).all(), f"{name}: {err.max():.3g} against {tol.min():.3g}"


# ---------------------------------------------------------------- 2. exact: integers
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_integer_inputs_give_the_integer_model_bit_for_bit(kind, case, batch_of):
    """x, g in [-4, 4], w in [-3, 3], integer bias, every w[h][d][c][o] drawn on its own: all partial sums are integers below 2^24
    (Hp 3 C 12 <= 608 256, 84 12, 10 M 16), so the float32 sums are exact in any order and every output equals the integer model,
    rounded once to binary16 (overflow to infinity included) where that is the type.  Every element of every output is written."""
    M, Hp, C, K, dt = case
    inp = integer_inputs(np.random.default_rng(hash(case[:4]) % 2 ** 32), M, Hp, C, K, dt)
    _, got = run_all(kind, batch_of(kind), inp)
    want = model(inp)
    assert max(np.abs(v).max() for v in model({k: np.abs(v) if isinstance(v, np.ndarray) else v for k, v in inp.items()}).values()) < 2 ** 24
    for name, a in got.items():
        assert written(a), name
        w = rounded(want[name], dt if name in ("out", "grad_x") else F32)
        bad = np.argwhere(a.view(w.dtype.str.replace("f", "u")) != w.view(w.dtype.str.replace("f", "u")))
        assert a.dtype == w.dtype and len(bad) == 0, f"{name}: {len(bad)} of {a.size} differ, first at {bad[0]}: {a[tuple(bad[0])]} for {w[tuple(bad[0])]}"


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("dt", TYPES, ids=["float32", "float16"])
def test_each_image_column_alone_pins_the_borders(kind, dt, batch_of):
    """x (forward), respectively grad_out's translation (grad_x) nonzero in a single column: of the forward's outputs only t = j - d,
    0 <= t <= 9, see column j, and grad_x's columns 0, 1, 10 and 11 have fewer than three terms — zeros, not wrapped reads."""
    b, M, Hp, C, K = batch_of(kind), 3, 5, 32, 7
    base = integer_inputs(np.random.default_rng(5), M, Hp, C, K, dt)
    for j in range(WIDE):
        inp = dict(base)
        inp["x"] = np.zeros_like(base["x"])
        inp["x"][:, :, j, :] = base["x"][:, :, j, :]
        inp["g"] = np.zeros_like(base["g"])
        if j < T:
            inp["g"][:, :, j, :] = base["g"][:, :, j, :]
        _, got = run_all(kind, b, inp)
        want = model(inp)
        for name in ("out", "grad_x", "grad_w", "grad_b"):
            assert same_bits(got[name], rounded(want[name], dt if name in ("out", "grad_x") else F32)), f"column {j}: {name}"
        touched = [t for t in range(T) if (want["out"][:, :, t, :] != base["bias"].reshape(ROT, K)[None].astype(F64)).any()]
        assert set(touched) <= {t for t in (j - 2, j - 1, j) if 0 <= t < T}


# ---------------------------------------------------------------- 3. general values within the derived bound
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("case", CASES[::2] + [(33, 22, 128, 7, F16), (33, 22, 128, 7, F32)], ids=case_id)
def test_grid_inputs_lie_within_the_bound_of_the_float64_model(kind, case, batch_of):
    """inputs k / 64, |k| <= 192; |got - exact| <= (n + 1) 2^-24 (sum |terms| + |bias|) + half a unit of the output's type (float32
    inputs: n + 2): kbd_support.bounds has the derivation.  The bound hides a single missing term; group 2 does not."""
    M, Hp, C, K, dt = case
    inp = grid_inputs(np.random.default_rng(hash(case[:4]) % 2 ** 32 + 1), M, Hp, C, K, dt)
    _, got = run_all(kind, batch_of(kind), inp)
    exact = model(inp)
    tol = bounds(inp, exact, dt)
    for name, a in got.items():
        with np.errstate(invalid="ignore"):
            err = np.abs(a.astype(F64) - exact[name])
        finite = np.isfinite(a.astype(F64))          # (a binary16 output may overflow: then the exact value rounds to infinity too)
        assert (finite | (np.abs(exact[name]) >= 65520.0)).all(), name
        worst = (err[finite] / np.maximum(tol[name][finite], 2.0 ** -1000)).max() if finite.any() else 0.0
        print(f"{name}: worst error {worst:.3g} of the bound")
        assert (err[finite] <= tol[name][finite]).all(), name         # (group 2 shows that every element is written: here a binary16 result may equal the guard pattern)


# ---------------------------------------------------------------- 4. reproducibility
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("dt", TYPES, ids=["float32", "float16"])
def test_a_second_call_gives_the_same_bytes(kind, dt, batch_of):
    """each entry point twice on the same inputs, grad_w at an M that spans three partials"""
    inp = grid_inputs(np.random.default_rng(9), 2 * partial() + 5, 6, 32, 7, dt)
    b = batch_of(kind)
    _, first = run_all(kind, b, inp)
    _, second = run_all(kind, b, inp)
    for name in first:
        assert same_bits(first[name], second[name]), name


# ---------------------------------------------------------------- 5. the argument rules
RULES = [("M = 0", dict(m=0), "M < 1"), ("M < 0", dict(m=-2), "M < 1"), ("K = 0", dict(n_pieces=0), "n_pieces must be in [1, 7]"),
         ("K = 8", dict(n_pieces=8), "n_pieces must be in [1, 7]"), ("Hp = 3", dict(height=3), "height must be in [4, 33]"),
         ("Hp = 34", dict(height=34), "height must be in [4, 33]"), ("C = 48", dict(channels=48), "channels must be a multiple of 32"),
         ("C = 0", dict(channels=0), "channels must be a multiple of 32"), ("C = 544", dict(channels=544), "channels must be a multiple of 32"),
         ("an unknown flag", dict(flags=2), "unknown flag"),
         ("x is NULL", dict(x=None), "are NULL", "fwd", "grad_w"), ("w is NULL", dict(w=None), "are NULL", "fwd", "grad_x"),
         ("bias is NULL", dict(bias=None), "are NULL", "fwd"), ("out is NULL", dict(out=None), "are NULL", "fwd"),
         ("grad_out is NULL", dict(grad_out=None), "are NULL", "grad_x", "grad_w"), ("grad_x is NULL", dict(grad_x=None), "are NULL", "grad_x"),
         ("grad_w is NULL", dict(grad_w=None), "are NULL", "grad_w"), ("grad_b is NULL", dict(grad_b=None), "are NULL", "grad_w")]


def refused(pkg, fn, k):
    with pytest.raises(pkg.TetrisError) as e:
        fn(k)
    return str(e.value)


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_bad_arguments_are_refused(kind, batch_of):
    """every rule on its own, refused with its own message, and no output byte touched (guard-filled buffers); a NULL struct; each
    array 4 bytes off its alignment; an output that overlaps an input"""
    pkg, b = ge.package(), batch_of(kind)
    fns = dict(fwd=b.kbd_conv_dev, grad_x=b.kbd_conv_grad_x_dev, grad_w=b.kbd_conv_grad_w_dev)
    inp = integer_inputs(np.random.default_rng(1), 5, 5, 32, 7, F32)
    nothing_written = lambda call: all(untouched(buf) for buf in call.outs.values())          # noqa: E731
    for rule in RULES:
        call = KbdCall(kind, b, inp, **rule[1])
        for which, fn in fns.items():
            if len(rule) == 3 or which in rule[3:]:
                assert rule[2] in refused(pkg, fn, call.k), f"{rule[0]} ({which})"
        sync(kind, b)
        assert nothing_written(call), rule[0]
    for fn in fns.values():
        assert "the argument struct is NULL" in refused(pkg, fn, None)
    for name, which in (("x", ("fwd", "grad_w")), ("w", ("fwd", "grad_x")), ("bias", ("fwd",)), ("g", ("grad_x", "grad_w")), ("out", ("fwd",)),
                        ("grad_x", ("grad_x",)), ("grad_w", ("grad_w",)), ("grad_b", ("grad_w",))):
        call = KbdCall(kind, b, inp, offsets={name: 4})
        for f in which:
            assert "16-byte aligned" in refused(pkg, fns[f], call.k), name
        sync(kind, b)
        assert nothing_written(call), name
    call = KbdCall(kind, b, inp)
    before = {n: buf.get() for n, buf in call.ins.items()}
    for field, where, which in (("d_out", call.ins["x"].ptr, "fwd"), ("d_out", call.ins["bias"].ptr, "fwd"), ("d_grad_x", call.ins["w"].ptr, "grad_x"),
                                ("d_grad_w", call.ins["g"].ptr, "grad_w"), ("d_grad_b", call.ins["x"].ptr + 64, "grad_w"),
                                ("d_grad_b", call.outs["grad_w"].ptr + 16, "grad_w")):
        bad = type(call.k).from_buffer_copy(call.k)
        setattr(bad, field, where)
        assert "overlap" in refused(pkg, fns[which], bad), (field, which)
        sync(kind, b)
        assert nothing_written(call) and all(same_bits(before[n], buf.get()) for n, buf in call.ins.items()), (field, which)


# ---------------------------------------------------------------- 7. TorchEnv.keyboard_conv inside a small training step (GPU only)
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_torch_keyboard_conv_inside_a_training_step(dtype):
    """keyboard_conv -> q_head -> dqn_loss -> backward at M = 33 on a float32 and on a binary16 parameter set (a float32 master
    weight either way, cast by the wrapper).  The gradient that reaches keyboard_conv's output is read off (retain_grad) and the
    float64 model is applied to it: grad_x, grad_w and grad_b must lie within group 3's bound for exactly these inputs; the forward
    likewise.  A channels_last input arrives without a copy (the tensor the wrapper hands to the library has the input's
    data_ptr), and a channels-first one, which is copied, gives the same bytes."""
    import torch
    pkg = ge.package()
    M, Hp, C, K = 33, 22, 128, 7
    dt = getattr(torch, dtype)
    ndt = F16 if dtype == "float16" else F32
    b = pkg.TetrisBatch(8, 1, 20, 10, device=0)
    try:
        ti = importlib.import_module("drl-tetris_amd.torch_interop")
        te = ti.TorchEnv(b)
        inp = grid_inputs(np.random.default_rng(11), M, Hp, C, K, ndt)
        inp["w"] = (inp["w"].astype(F64) / 64.0).astype(ndt)                 # small weights keep Q's tanh off saturation
        x_last = torch.tensor(inp["x"]).cuda().permute(0, 3, 1, 2).requires_grad_()          # [M, C, Hp, 12], channels_last memory
        assert x_last.is_contiguous(memory_format=torch.channels_last)
        w = torch.tensor(inp["w"].astype(F32)).cuda().requires_grad_()
        bias = torch.tensor(inp["bias"]).cuda().requires_grad_()
        action = torch.stack([torch.arange(M) % 4, torch.arange(M) % 10, torch.arange(M) % 7], 1).to(torch.uint8).cuda()
        target = torch.linspace(-1, 1, M).cuda()
        assert te._kbd_input(x_last.detach()).data_ptr() == x_last.data_ptr(), "a channels_last input is taken without a copy"
        y = te.keyboard_conv(x_last, w, bias)
        assert y.dtype == dt and tuple(y.shape) == (M, 4, 10, K)
        y.retain_grad()
        first = y.detach().clone()
        loss = te.dqn_loss(te.q_head(y, None, mode="mean")[0], action, target, grad_scale=256.0 if dtype == "float16" else 1.0)[0]
        loss.backward()
        g = y.grad.detach().cpu().numpy()
        assert np.abs(g).max() > 0 and w.grad.dtype == torch.float32 and bias.grad.dtype == torch.float32 and x_last.grad.dtype == dt
        inp["g"] = g
        exact = model(inp)
        tol = bounds(inp, exact, ndt)
        got = dict(out=first.cpu().numpy(), grad_x=x_last.grad.permute(0, 2, 3, 1).contiguous().cpu().numpy(), grad_w=w.grad.cpu().numpy(),
                   grad_b=bias.grad.cpu().numpy())
        for name, a in got.items():
            err = np.abs(a.astype(F64) - exact[name])          # (dqn_loss's gradient is zero but at the action: many sums are exactly 0)
            worst = (err[tol[name] > 0] / tol[name][tol[name] > 0]).max()
            print(f"{dtype} {name}: worst error {worst:.3g} of the bound")
            assert (err <= tol[name]).all(), name
        x_first = x_last.detach().contiguous()                               # channels-first memory: one layout copy inside
        assert not x_first.is_contiguous(memory_format=torch.channels_last) and te._kbd_input(x_first).data_ptr() != x_first.data_ptr()
        again = te.keyboard_conv(x_first, w.detach(), bias.detach())
        assert torch.equal(again, first)
    finally:
        b.close()


def test_weight_layout_helpers_and_the_reference_initialisation():
    """kbd_weight_from_conv2d / _to_conv2d are the permutes between torch's OIHW and the reference's HWIO and undo each other;
    keyboard_conv_init gives a zero kernel and a bias drawn from N(0, 1e-5)"""
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    oihw = torch.arange(28 * 32 * 5 * 3, dtype=torch.float32).reshape(28, 32, 5, 3)
    hwio = ti.kbd_weight_from_conv2d(oihw)
    assert tuple(hwio.shape) == (5, 3, 32, 28) and hwio.is_contiguous() and float(hwio[4, 2, 7, 9]) == float(oihw[9, 7, 4, 2])
    assert torch.equal(ti.kbd_weight_to_conv2d(hwio), oihw)
    w, bias = ti.keyboard_conv_init(22, 128, 7, generator=torch.Generator().manual_seed(1))
    assert tuple(w.shape) == (22, 3, 128, 28) and not w.any() and tuple(bias.shape) == (28,)
    assert 0 < float(bias.abs().max()) < 1e-4 and w.dtype == bias.dtype == torch.float32
