"""One residual layer on the device (include/tetris_hip.h: tetris_res_layer_dev, tetris_res_layer_grad_x_dev,
tetris_res_layer_grad_w_dev) against the model of tests/res_support.py, written from the header's definition: 1. the float64 model
against float64 torch autograd of the reference's own lines; 2. integer inputs, whose sums are exact in float32 in any order: bit
equality with the model — the structural test; 3. general values within a derived tolerance of the float64 model; 4. the border: a
single nonzero position; 5. a second call gives the same bytes; 6. zero-padded channels; 7. the argument rules and untouched
buffers; 8. on the GPU TorchEnv.residual_block inside a small training step.  (9. is the stand-alone sanitizer program
tests/sanitizers/res_main.cpp.)  Every group but 1, 6's model part and 8 runs on the CPU harness (`-m "not gpu"`) and on the MI355X
(`-m gpu`); on the harness the "device" buffers are numpy arrays."""
import importlib
import itertools

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import engines
from tests.buffers import GUARD, sync
from tests.res_support import (ACTS, EXPM1_ULP, F16, F32, F64, JOINS, U24, WIDE, ResCall, bounds, capi, cout, e_of, forward, gradients,
                               grid_inputs, integer_inputs, magnitudes, model, ref_residual_layer, rounded, run_all, untouched)

TYPES = (F32, F16)
CIS, COS = (8, 24, 32, 40, 136, 512), (32, 96, 128, 512)
SETTINGS = list(itertools.product(JOINS, ACTS))


def band():
    return capi().RES_ROWS


def partial():
    return capi().RES_W_SAMPLES


def heights():
    """4, 5, 6, 22, 33 and the heights around the row band R of the kernels: R - 1, R, R + 1, 2 R + 1"""
    R = band()
    return tuple(dict.fromkeys(h for h in (4, 5, 6, 22, 33, R - 1, R, R + 1, 2 * R + 1) if 4 <= h <= 33))


def _cases():
    """(M, Hp, Ci, Co, join, act, dtype), laid out from the blocking constants the library exports.  The forward and grad_x kernels
    block over image rows (RES_ROWS of one sample a workgroup; no sample blocking), so Hp goes around the band besides 4, 5, 6, 22,
    33, and M around the samples per partial of grad_w.  Hp, Ci, Co, the settings and the type rotate with indices of their own,
    so that none is tied to another; the 512-channel cases stay at M <= 3 and Hp = 4; then the default shape; then M around the
    partial at the smallest shape."""
    P, HPS = partial(), heights()
    cases = []
    for n in range(36):
        M, Hp, Ci, Co = (1, 2, 3, 5)[n % 4], HPS[n % len(HPS)], CIS[(n + n // 6) % 6], COS[(n + n // 4 + n // 12) % 4]
        join, act = SETTINGS[(n + n // 9) % 6]
        dt = TYPES[(n + n // 2 + n // 6) % 2]
        if max(Ci, Co) == 512:
            M, Hp = min(M, 3), 4
        elif Hp > 12:
            M = min(M, 2)
        cases.append((M, Hp, Ci, Co, join, act, dt))
    for dt in TYPES:
        cases.append((2, 22, 128, 128, "add", "elu", dt))
        cases.append((2, 9, 136, 128, "add", "elu", dt))
        cases.append((3, 5, 128, 32, "truncate_add", "elu", dt))
        cases.append((3, 5, 32, 32, "truncate_add", "none", dt))
    for i, M in enumerate((P - 1, P, P + 1, 2 * P + 1)):
        join, act = SETTINGS[(i + 3) % 6]
        cases.append((M, 4, 8, 32, join, act, TYPES[i % 2]))
        cases.append((M, 4, 8, 32, "add", "elu", TYPES[(i + 1) % 2]))
    return list(dict.fromkeys(cases))


CASES = _cases()


def case_id(c):
    return f"M{c[0]}-Hp{c[1]}-Ci{c[2]}-Co{c[3]}-{c[4]}-{c[5]}-{np.dtype(c[6]).name}"


def test_the_cases_cover_what_they_should():
    seen = lambda f: {f(c) for c in CASES}          # noqa: E731
    assert seen(lambda c: c[1]) == set(heights()) and seen(lambda c: c[2]) >= set(CIS) and seen(lambda c: c[3]) >= set(COS)
    assert seen(lambda c: (c[4], c[5], c[6])) == set(itertools.product(JOINS, ACTS, TYPES))
    order = lambda c: (c[2] > c[3]) - (c[2] < c[3])          # noqa: E731
    assert seen(lambda c: (c[4], order(c))) >= set(itertools.product(("add", "truncate_add"), (-1, 0, 1)))
    assert all(c[0] <= 3 and c[1] == 4 for c in CASES if max(c[2], c[3]) == 512)
    for dt in TYPES:          # general values meet ELU below zero with every join in both types, and every order of Ci and Co
        assert {(c[4], order(c)) for c in CASES if c[6] == dt and c[5] == "elu"} >= {("none", -1), ("add", -1), ("add", 1), ("truncate_add", 1)}
    P = partial()
    assert seen(lambda c: c[0]) >= {1, P - 1, P, P + 1, 2 * P + 1}


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


def as_uint(a):
    return a.view(a.dtype.str.replace("f", "u"))


# ---------------------------------------------------------------- 1. the float64 model against autograd of the reference's lines
# Tolerance, as derived in test_kbd_conv.py group 1.  Both sides form the same n products exactly alike and add them in different
# orders: each of at most n additions rounds a partial sum of magnitude <= S = sum |terms| by at most 2^-53 S.  Two sides, and the
# products' own roundings where the libraries fuse them: 4 (n + 1) 2^-53 S per element, n = 9 Ci + 2, 9 Co + 1 or 12 Hp M.  ELU's
# exp is one more float64 unit at 1 on the forward (|expm1| <= 1) and, through y + 1 <= 1, one unit of every term of a gradient.
@pytest.mark.parametrize("Ci,Co", [(8, 32), (32, 32), (40, 32)])
@pytest.mark.parametrize("join,act", SETTINGS)
def test_the_float64_model_against_torch_autograd(Ci, Co, join, act):
    import torch
    M, Hp = 3, 5
    rng = np.random.default_rng(Ci * 100 + Co + len(join) + len(act))
    Cout = cout(Ci, Co, join)
    inp = dict(join=join, act=act, x=rng.standard_normal((M, Hp, WIDE, Ci)), w=rng.standard_normal((3, 3, Ci, Co)) / 8.0,
               bias=rng.standard_normal(Co), g=rng.standard_normal((M, Hp, WIDE, Cout)))
    x = torch.tensor(inp["x"]).permute(0, 3, 1, 2).contiguous().requires_grad_()              # NCHW
    w, bias = torch.tensor(inp["w"]).requires_grad_(), torch.tensor(inp["bias"]).requires_grad_()
    y = ref_residual_layer(x, w, bias, join, act)
    assert tuple(y.shape) == (M, Hp, WIDE, Cout)
    gx, gw, gb = torch.autograd.grad(y, (x, w, bias), torch.tensor(inp["g"]))
    want = dict(out=y.detach().numpy(), grad_x=gx.permute(0, 2, 3, 1).numpy(), grad_w=gw.numpy(), grad_b=gb.numpy())
    inp["y"] = forward(inp["x"], inp["w"], inp["bias"], join, act)          # the model's own output, as the definition takes it
    got = model(inp, round_e=False)
    mag = magnitudes(inp)
    n = dict(out=9 * Ci + 2, grad_x=9 * Co + 1, grad_w=WIDE * Hp * M, grad_b=WIDE * Hp * M)
    for name in got:
        err = np.abs(got[name] - want[name])
        tol = 4 * (n[name] + 1) * 2.0 ** -53 * mag[name] + (2.0 ** -53 * (1.0 if name == "out" else 4 * mag[name]) if act == "elu" else 0.0)
        assert got[name].shape == want[name].shape and (err <= tol).all(), f"{name}: {(err - tol).max():.3g} over"


# ---------------------------------------------------------------- 2. exact: integers
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_integer_inputs_give_the_model_bit_for_bit(kind, case, batch_of):
    """x, g in [-4, 4], w in [-3, 3], integer bias, y from {-0.75, -0.5, -0.25, 0, 1, 2}: every partial sum is a multiple of 0.25
    whose magnitudes add up to less than 2^24 quarter units (asserted: 9 512 12 + 8 + 4, 9 512 12 + 4, M Hp 12 16), so the float32
    sums are exact in any order and all four outputs equal the model, rounded once where the type is binary16 — but for the ELU
    forward's elements with p <= 0, which are that or within expm1's bound.  Every element of every output is written."""
    M, Hp, Ci, Co, join, act, dt = case
    inp = integer_inputs(np.random.default_rng(hash(case[:4]) % 2 ** 32), M, Hp, Ci, Co, join, act, dt)
    _, got = run_all(kind, batch_of(kind), inp)
    want = model(inp)
    assert 4 * max(np.abs(v).max() for v in magnitudes(inp).values()) < 2 ** 24
    p = forward(inp["x"], inp["w"], inp["bias"], join, "none")
    for name, a in got.items():
        assert written(a), name
        w = rounded(want[name], dt if name in ("out", "grad_x") else F32)
        differ = as_uint(a) != as_uint(w)
        if name == "out" and act == "elu":
            tol = EXPM1_ULP * U24 * np.abs(want[name]) + (2.0 ** -11 * np.abs(want[name]) + 2.0 ** -25 if dt == F16 else U24 * np.abs(want[name]))
            differ &= ~((p <= 0) & (np.abs(a.astype(F64) - want[name]) <= tol))
        bad = np.argwhere(differ)
        assert a.dtype == w.dtype and len(bad) == 0, f"{name}: {len(bad)} of {a.size} differ, first at {bad[0]}: {a[tuple(bad[0])]} for {w[tuple(bad[0])]}"


# ---------------------------------------------------------------- 3. general values within the derived bound
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("case", CASES + [(33, 22, 128, 128, "add", "elu", F16)], ids=case_id)
def test_grid_inputs_lie_within_the_bound_of_the_float64_model(kind, case, batch_of):
    """inputs k / 64, |k| <= 192, y the model's own rounded output; res_support.bounds has the derivation.  The bound hides a single
    missing term; group 2 does not."""
    M, Hp, Ci, Co, join, act, dt = case
    inp = grid_inputs(np.random.default_rng(hash(case[:4]) % 2 ** 32 + 1), M, Hp, Ci, Co, join, act, dt)
    _, got = run_all(kind, batch_of(kind), inp)
    exact = model(inp, round_e=False)
    tol = bounds(inp, exact, dt)
    for name, a in got.items():
        with np.errstate(invalid="ignore"):
            err = np.abs(a.astype(F64) - exact[name])
        finite = np.isfinite(a.astype(F64))          # (a binary16 output may overflow: then the exact value rounds to infinity too)
        assert (finite | (np.abs(exact[name]) >= 65504.0 - tol[name])).all(), name
        worst = (err[finite] / np.maximum(tol[name][finite], 2.0 ** -1000)).max() if finite.any() else 0.0
        print(f"{name}: worst error {worst:.3g} of the bound")
        assert (err[finite] <= tol[name][finite]).all(), name


# ---------------------------------------------------------------- 4. the border
SPOTS = [(0, 0), (0, 11), (-1, 0), (-1, 11), (0, 5), (-1, 6), (2, 0), (1, 11), (2, 5)]          # corners, edges, interior


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("dt", TYPES, ids=["float32", "float16"])
@pytest.mark.parametrize("Hp", [4, 9])
def test_a_single_position_pins_the_zero_border(kind, dt, Hp, batch_of):
    """x (forward, grad_w), respectively g (grad_x, grad_w) nonzero at a single position of the middle one of three samples: bit
    equality with the model, and only the clipped 3 x 3 neighbourhood of that sample's out differs from the bias-only image —
    zeros, not reads that wrap across rows or samples.  Hp = 9 has a second row band of one row."""
    b, M, Ci, Co = batch_of(kind), 3, 8, 32
    base = integer_inputs(np.random.default_rng(5), M, Hp, Ci, Co, "none", "none", dt)
    for h, j in SPOTS:
        h = h % Hp
        inp = dict(base)
        for name in ("x", "g"):
            inp[name] = np.zeros_like(base[name])
            inp[name][1, h, j, :] = np.where(base[name][1, h, j, :] == 0, 1, base[name][1, h, j, :])
        _, got = run_all(kind, b, inp)
        want = model(inp)
        for name in ("out", "grad_x", "grad_w", "grad_b"):
            assert same_bits(got[name], rounded(want[name], dt if name in ("out", "grad_x") else F32)), f"({h}, {j}): {name}"
        for name, rest in (("out", base["bias"].astype(F64)), ("grad_x", 0.0)):
            moved = np.argwhere((got[name].astype(F64) != rest).any(axis=3))
            assert all(m == 1 and abs(hh - h) <= 1 and abs(jj - j) <= 1 for m, hh, jj in moved), f"({h}, {j}): {name}"


# ---------------------------------------------------------------- 5. reproducibility
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("dt", TYPES, ids=["float32", "float16"])
def test_a_second_call_gives_the_same_bytes(kind, dt, batch_of):
    """each entry point twice on the same inputs, grad_w at an M that spans three partials"""
    inp = grid_inputs(np.random.default_rng(9), 2 * partial() + 5, 5, 24, 32, "add", "elu", dt)
    b = batch_of(kind)
    _, first = run_all(kind, b, inp)
    _, second = run_all(kind, b, inp)
    for name in first:
        assert same_bits(first[name], second[name]), name


# ---------------------------------------------------------------- 6. padding
def _padded_chain(C1, Cp1):
    """two ADD + ELU layers C1 -> 32 -> 32 and the same chain with the input zero-padded to Cp1 channels, arbitrary weights facing
    the pad channels -> (the unpadded inputs per layer, the padded ones)"""
    rng = np.random.default_rng(C1)
    M, Hp, Co = 2, 5, 32
    draw = lambda *s: rng.integers(-64, 65, s) / 64.0          # noqa: E731
    x, w1, w1_pad, b1 = draw(M, Hp, WIDE, C1), draw(3, 3, C1, Co) / 8, draw(3, 3, Cp1 - C1, Co), draw(Co)
    xp = np.concatenate([x, np.zeros((M, Hp, WIDE, Cp1 - C1))], axis=3)
    w1p = np.concatenate([w1, w1_pad], axis=2)
    C2, Cp2 = max(C1, Co), max(Cp1, Co)
    w2, w2_pad, b2 = draw(3, 3, C2, Co) / 8, draw(3, 3, Cp2 - C2, Co), draw(Co)
    w2p = np.concatenate([w2, w2_pad], axis=2)
    return (x, [(w1, b1), (w2, b2)]), (xp, [(w1p, b1), (w2p, b2)])


@pytest.mark.parametrize("C1,Cp1", [(5, 8), (131, 136)])
def test_zero_padded_channels_change_nothing_in_the_model(C1, Cp1):
    """the reference's first layer sees 1..5 channels and its second block 128 + 3: padded to a multiple of 8 with zero channels, a
    two-layer ADD + ELU chain gives the unpadded chain's numbers in the real channels and exact zeros in the pad channels"""
    (x, layers), (xp, layers_p) = _padded_chain(C1, Cp1)
    rng = np.random.default_rng(C1 + 1)
    for (w, b), (wp, bp) in zip(layers, layers_p):
        y, yp = forward(x, w, b, "add", "elu"), forward(xp, wp, bp, "add", "elu")
        C, Cin = y.shape[3], x.shape[3]
        assert np.array_equal(yp[..., :C], y) and not yp[..., C:].any() and yp.shape[3] == max(C, wp.shape[2])
        # the gradients: whatever arrives in the pad channels of out, the real channels' gradients are the unpadded layer's, and the
        # rows of the kernel that face the padding get none
        gp = rng.integers(-64, 65, yp.shape) / 64.0
        got = gradients(xp, wp, e_of(gp, yp, "elu"), "add")
        want = gradients(x, w, e_of(gp[..., :C], y, "elu"), "add")
        close = lambda a, b: np.allclose(a, b, rtol=0, atol=2.0 ** -40 * np.abs(b).max())          # noqa: E731  (float64 sums in two orders)
        assert close(got["grad_w"][:, :, :Cin, :], want["grad_w"]) and not got["grad_w"][:, :, Cin:, :].any()
        assert close(got["grad_b"], want["grad_b"]) and close(got["grad_x"][..., :Cin], want["grad_x"])
        x, xp = y, yp


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_zero_padded_channels_on_the_engine(kind, batch_of):
    """the padded chain 131 -> 136 through the library, float32: every layer's real channels lie within group 3's bound of the
    UNPADDED float64 model of that layer's real input channels, and the pad channels of every layer's out are exactly zero; with
    a gradient that is arbitrary in the pad channels too, grad_w's rows facing the padding are exactly zero and the real
    channels' gradients lie within the bound of the unpadded model's"""
    _, (xp, layers_p) = _padded_chain(131, 136)
    b, xp, real, rng = batch_of(kind), xp.astype(F32), 131, np.random.default_rng(7)
    for wp, bp in layers_p:
        Co = wp.shape[3]
        shape = xp.shape[:3] + (cout(wp.shape[2], Co, "add"),)
        inp = dict(join="add", act="elu", x=xp, w=wp.astype(F32), bias=bp.astype(F32), g=(rng.integers(-64, 65, shape) / 64.0).astype(F32))
        inp["y"] = rounded(forward(inp["x"], inp["w"], inp["bias"], "add", "elu"), F32)
        _, got = run_all(kind, b, inp)
        tol = bounds(inp, model(inp, round_e=False), F32)          # (the pad channels add zeros to the magnitudes)
        out_real = max(real, Co)
        plain = dict(inp, x=xp[..., :real], w=inp["w"][:, :, :real, :], g=inp["g"][..., :out_real], y=inp["y"][..., :out_real])
        want = model(plain, round_e=False)
        assert want["out"].shape[3] == out_real and (np.abs(got["out"][..., :out_real].astype(F64) - want["out"]) <= tol["out"][..., :out_real]).all()
        assert not got["out"][..., out_real:].any() and got["out"].shape[3] == max(xp.shape[3], Co)
        assert not got["grad_w"][:, :, real:, :].any()
        assert (np.abs(got["grad_w"][:, :, :real, :].astype(F64) - want["grad_w"]) <= tol["grad_w"][:, :, :real, :]).all()
        assert (np.abs(got["grad_b"].astype(F64) - want["grad_b"]) <= tol["grad_b"]).all()
        assert (np.abs(got["grad_x"][..., :real].astype(F64) - want["grad_x"]) <= tol["grad_x"][..., :real]).all()
        xp, real = got["out"], out_real


# ---------------------------------------------------------------- 7. the argument rules
RULES = [("M = 0", dict(m=0), "M < 1"), ("M < 0", dict(m=-2), "M < 1"), ("Hp = 3", dict(height=3), "height must be in [4, 33]"),
         ("Hp = 34", dict(height=34), "height must be in [4, 33]"), ("Ci = 12", dict(in_channels=12), "in_channels must be a multiple of 8"),
         ("Ci = 0", dict(in_channels=0), "in_channels must be a multiple of 8"), ("Ci = 520", dict(in_channels=520), "in_channels must be a multiple of 8"),
         ("Co = 48", dict(out_channels=48), "out_channels must be a multiple of 32"), ("Co = 0", dict(out_channels=0), "out_channels must be a multiple of 32"),
         ("Co = 544", dict(out_channels=544), "out_channels must be a multiple of 32"), ("join = 3", dict(join=3), "unknown join"),
         ("join = -1", dict(join=-1), "unknown join"), ("activation = 2", dict(activation=2), "unknown activation"),
         ("an unknown flag", dict(flags=2), "unknown flag"),
         ("x is NULL", dict(x=None), "are NULL", "fwd", "grad_w"), ("w is NULL", dict(w=None), "are NULL", "fwd", "grad_x"),
         ("bias is NULL", dict(bias=None), "are NULL", "fwd"), ("out is NULL", dict(out=None), "are NULL", "fwd"),
         ("y is NULL", dict(y=None), "are NULL", "grad_x", "grad_w"),
         ("grad_out is NULL", dict(grad_out=None), "are NULL", "grad_x", "grad_w"), ("grad_x is NULL", dict(grad_x=None), "are NULL", "grad_x"),
         ("grad_w is NULL", dict(grad_w=None), "are NULL", "grad_w"), ("grad_b is NULL", dict(grad_b=None), "are NULL", "grad_w")]


def refused(pkg, fn, k):
    with pytest.raises(pkg.TetrisError) as e:
        fn(k)
    return str(e.value)


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_bad_arguments_are_refused(kind, batch_of):
    """every rule on its own, refused with its own message, and no output byte touched (guard-filled buffers); a NULL struct; each
    array 4 bytes off its alignment; an output that overlaps an input.  Without ELU y may be NULL."""
    pkg, b = ge.package(), batch_of(kind)
    fns = dict(fwd=b.res_layer_dev, grad_x=b.res_layer_grad_x_dev, grad_w=b.res_layer_grad_w_dev)
    inp = integer_inputs(np.random.default_rng(1), 5, 5, 8, 32, "add", "elu", F32)
    nothing_written = lambda call: all(untouched(buf) for buf in call.outs.values())          # noqa: E731
    for rule in RULES:
        call = ResCall(kind, b, inp, **rule[1])
        for which, fn in fns.items():
            if len(rule) == 3 or which in rule[3:]:
                assert rule[2] in refused(pkg, fn, call.k), f"{rule[0]} ({which})"
        sync(kind, b)
        assert nothing_written(call), rule[0]
    for fn in fns.values():
        assert "the argument struct is NULL" in refused(pkg, fn, None)
    for name, which in (("x", ("fwd", "grad_w")), ("w", ("fwd", "grad_x")), ("bias", ("fwd",)), ("g", ("grad_x", "grad_w")), ("y", ("grad_x", "grad_w")),
                        ("out", ("fwd",)), ("grad_x", ("grad_x",)), ("grad_w", ("grad_w",)), ("grad_b", ("grad_w",))):
        call = ResCall(kind, b, inp, offsets={name: 4})
        for f in which:
            assert "16-byte aligned" in refused(pkg, fns[f], call.k), name
        sync(kind, b)
        assert nothing_written(call), name
    call = ResCall(kind, b, inp)
    before = {n: buf.get() for n, buf in call.ins.items()}
    for field, where, which in (("d_out", call.ins["x"].ptr, "fwd"), ("d_out", call.ins["bias"].ptr, "fwd"), ("d_grad_x", call.ins["w"].ptr, "grad_x"),
                                ("d_grad_x", call.ins["y"].ptr + 32, "grad_x"), ("d_grad_w", call.ins["g"].ptr, "grad_w"),
                                ("d_grad_b", call.ins["x"].ptr + 64, "grad_w"), ("d_grad_b", call.outs["grad_w"].ptr + 16, "grad_w")):
        bad = type(call.k).from_buffer_copy(call.k)
        setattr(bad, field, where)
        assert "overlap" in refused(pkg, fns[which], bad), (field, which)
        sync(kind, b)
        assert nothing_written(call) and all(same_bits(before[n], buf.get()) for n, buf in call.ins.items()), (field, which)
    plain = dict(inp, act="none")
    call = ResCall(kind, b, plain, y=None)
    b.res_layer_grad_x_dev(call.k)
    b.res_layer_grad_w_dev(call.k)
    sync(kind, b)
    want = model(plain)
    assert all(same_bits(call.get(n)[n], rounded(want[n], F32)) for n in ("grad_x", "grad_w", "grad_b"))


# ---------------------------------------------------------------- 8. TorchEnv.residual_block inside a small training step (GPU only)
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_torch_residual_block_inside_a_training_step(dtype):
    """residual_block (three layers, Ci 8 -> 128, Hp = 22) -> keyboard_conv -> q_head -> dqn_loss -> backward at M = 33, float32
    master weights.  Each layer's input, output and incoming gradient are read off (retain_grad) and the float64 model is applied to
    exactly those tensors, layer by layer: out, grad_x, grad_w and grad_b must lie within group 3's bound for those inputs.  The
    chain hands channels_last tensors on without a copy (the tensor the wrapper hands to the library has the input's data_ptr),
    and a channels-first input gives the same bytes."""
    import torch
    pkg = ge.package()
    M, Hp, K = 33, 22, 7
    dt = getattr(torch, dtype)
    ndt = F16 if dtype == "float16" else F32
    b = pkg.TetrisBatch(8, 1, 20, 10, device=0)
    try:
        ti = importlib.import_module("drl-tetris_amd.torch_interop")
        te = ti.TorchEnv(b)
        rng = np.random.default_rng(12)
        gen = torch.Generator().manual_seed(3)
        x0 = torch.tensor((rng.integers(-64, 65, (M, Hp, WIDE, 5)) / 64.0).astype(ndt)).cuda().permute(0, 3, 1, 2)
        x_in = ti.pad_channels(x0).requires_grad_()
        assert tuple(x_in.shape) == (M, 8, Hp, WIDE) and x_in.is_contiguous(memory_format=torch.channels_last) and not x_in[:, 5:].any()
        params = [tuple(t.cuda().requires_grad_() for t in ti.residual_layer_init(ci, 128, generator=gen)) for ci in (8, 128, 128)]
        with torch.no_grad():
            for _, bias in params:
                bias.add_(torch.tensor(rng.integers(-8, 9, 128) / 64.0, dtype=torch.float32).cuda())
        kw = (torch.tensor(rng.integers(-64, 65, (Hp, 3, 128, 4 * K)) / 4096.0, dtype=torch.float32).cuda().requires_grad_())
        kb = torch.zeros(4 * K, dtype=torch.float32).cuda().requires_grad_()
        action = torch.stack([torch.arange(M) % 4, torch.arange(M) % 10, torch.arange(M) % 7], 1).to(torch.uint8).cuda()
        target = torch.linspace(-1, 1, M).cuda()
        seen, xs = [], [x_in]
        for i, (w, bias) in enumerate(params):
            y = te.residual_layer(xs[-1], w, bias, slot=i)
            assert y.grad_fn.x.data_ptr() == xs[-1].data_ptr(), "the tensor handed to the library is the channels_last input itself"
            assert y.dtype == dt and tuple(y.shape) == (M, 128, Hp, WIDE) and y.is_contiguous(memory_format=torch.channels_last)
            y.retain_grad()
            xs.append(y)
        first = [t.detach().clone() for t in xs[1:]]
        q = te.keyboard_conv(xs[-1], kw, kb)
        assert q.grad_fn.x.data_ptr() == xs[-1].data_ptr(), "the last layer feeds keyboard_conv without a copy"
        loss = te.dqn_loss(te.q_head(q, None, mode="mean")[0], action, target, grad_scale=256.0 if dtype == "float16" else 1.0)[0]
        loss.backward()
        nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous().cpu().numpy()          # noqa: E731
        for i, (w, bias) in enumerate(params):
            assert w.grad.dtype == torch.float32 and bias.grad.dtype == torch.float32 and xs[i].grad.dtype == dt
            inp = dict(join="add", act="elu", x=nhwc(xs[i]), w=w.detach().to(dt).cpu().numpy(), bias=bias.detach().cpu().numpy(),
                       g=nhwc(xs[i + 1].grad), y=nhwc(first[i]))
            assert np.abs(inp["g"]).max() > 0
            exact = model(inp, round_e=False)
            tol = bounds(inp, exact, ndt)
            got = dict(out=nhwc(first[i]), grad_x=nhwc(xs[i].grad), grad_w=w.grad.cpu().numpy(), grad_b=bias.grad.cpu().numpy())
            for name, a in got.items():
                err = np.abs(a.astype(F64) - exact[name])
                worst = (err[tol[name] > 0] / tol[name][tol[name] > 0]).max()
                print(f"{dtype} layer {i} {name}: worst error {worst:.3g} of the bound")
                assert (err <= tol[name]).all(), (i, name)
        # the block is the same three calls; a channels-first input is copied once and gives the same bytes
        x_first = x_in.detach().contiguous()
        assert not x_first.is_contiguous(memory_format=torch.channels_last) and te._kbd_input(x_first).data_ptr() != x_first.data_ptr()
        again = te.residual_block(x_first, [(w.detach(), bias.detach()) for w, bias in params])
        assert torch.equal(again, first[-1])
        short = te.residual_block(x_in.detach(), [(w.detach(), bias.detach()) for w, bias in params[:1]] +
                                  [tuple(t.cuda() for t in ti.residual_layer_init(128, 32, generator=gen))], output_activation=None, output_n_filters=32, slot=8)
        assert tuple(short.shape) == (M, 32, Hp, WIDE)
        # without slots every pending forward of equal shape finds a buffer set of its own: the same step gives the same bytes,
        # twice over (the sets come round), and so does a chain without a gradient
        want = [t.grad.clone() for pair in params for t in pair] + [x_in.grad.clone()]
        for _ in range(2):
            for t in [x_in] + [t for pair in params for t in pair] + [kw, kb]:
                t.grad = None
            out = te.residual_block(x_in, params)
            assert torch.equal(out, first[-1])
            q = te.keyboard_conv(out, kw, kb)
            te.dqn_loss(te.q_head(q, None, mode="mean")[0], action, target, grad_scale=256.0 if dtype == "float16" else 1.0)[0].backward()
            assert all(torch.equal(a, b) for a, b in zip([t.grad for pair in params for t in pair] + [x_in.grad], want))
            assert not any(te._res_pending.values())
        with torch.no_grad():
            assert torch.equal(te.residual_block(x_in, params), first[-1])
    finally:
        b.close()


def test_the_reference_initialisation_and_the_padding_helper():
    """residual_layer_init gives a glorot-uniform HWIO kernel (|w| <= sqrt(6 / (9 Ci + 9 Co)), spread over the range) and a zero
    bias; pad_channels zero-fills up to a multiple of 8 in channels_last memory; the layout helpers serve 3 x 3 kernels"""
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    w, bias = ti.residual_layer_init(40, 128, generator=torch.Generator().manual_seed(1))
    limit = (6.0 / (9 * 40 + 9 * 128)) ** 0.5
    assert tuple(w.shape) == (3, 3, 40, 128) and tuple(bias.shape) == (128,) and not bias.any() and w.dtype == bias.dtype == torch.float32
    assert 0.99 * limit < float(w.abs().max()) <= limit and abs(float(w.mean())) < 0.01 * limit and abs(float(w.var()) - limit ** 2 / 3) < 0.05 * limit ** 2
    x = torch.arange(2 * 5 * 4 * 12, dtype=torch.float32).reshape(2, 5, 4, 12)
    xp = ti.pad_channels(x)
    assert tuple(xp.shape) == (2, 8, 4, 12) and xp.is_contiguous(memory_format=torch.channels_last) and torch.equal(xp[:, :5], x) and not xp[:, 5:].any()
    assert ti.pad_channels(xp) is xp
    oihw = torch.arange(32 * 8 * 9, dtype=torch.float32).reshape(32, 8, 3, 3)
    hwio = ti.kbd_weight_from_conv2d(oihw)
    assert tuple(hwio.shape) == (3, 3, 8, 32) and float(hwio[2, 1, 5, 7]) == float(oihw[7, 5, 2, 1]) and torch.equal(ti.kbd_weight_to_conv2d(hwio), oihw)
