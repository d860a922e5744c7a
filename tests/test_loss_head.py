"""The trainer's loss heads on the device (include/tetris_hip.h: tetris_ppo_loss_dev, tetris_dqn_loss_dev) against the model of
tests/loss_support.py, written from the header's definitions: bit equality in float32 for everything that does not pass through
the logarithm, the same formulas in float64 with a derived tolerance for what does, the float64 model's gradients against torch
autograd of the reference's expressions, the statistics against float64 sums with the standard summation bound and bit for bit
against the sum in the order the header states, all of this again at batch sizes where the single-workgroup loops behind the
heads (the count of D, the reduction of the blocks' rows) go round more than once, the scratch buffer across sizes, the argument
rules, and on the GPU the TorchEnv wrappers inside a small training step.  Every test but the last group runs on the CPU harness
(`-m "not gpu"`) and on the MI355X (`-m gpu`); on the harness the "device" buffers are numpy arrays."""
import importlib
import itertools

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import engines
from tests.loss_support import (BLOCK, CARRY_SIZES, DQN_STATS, F32, F64, PARAM_SETS, PPO_STATS, U24, DqnCall, Params, PpoCall, assert_carry_mask,
                                carry_mask, dqn_inputs, dqn_model, dqn_stated_stats, entropy_constants, expand, expand_v, loop_sum, ppo_inputs,
                                ppo_model, ppo_stated_stats, same_bits, stated_bound, stated_sum, sum_bound, torch_dqn_loss, torch_ppo_loss,
                                weigh_the_full_slots, written)

SIZES = (1, 33, 64, 65, 257)          # one sample, a partial wave, a block, a block and one, several blocks with a partial last
KV = ((7, 1), (7, 7), (1, 1))
TYPES = (np.float32, np.float16)
# |H - formula| on normalised maps, as tests/test_act_eval.py::test_entropy_of_pi derives it — 40 terms |q log q| <= 0.368 with an
# input rounding, a logf of 1 ulp on the host and at most 3 ulp on the device (the bound OpenCL sets and the device library
# documents) and a product rounding, and 40 partial-sum roundings below 3.7: about 1.2e-5 — times four
TOL_H = 5e-5
# |e_j - formula|, e_j = -(l_j + [q_j > e]): l_j = logf(q_j) lies in [-13.9, 0.01]: 3 ulp of a float32 below 16 are 2.9e-6, the
# rounding of q_j moves the logarithm by 6e-8, the addition rounds by at most 4.8e-7: about 3.4e-6 — times four
TOL_E = 1.4e-5


def shapes(types=2):
    """(M, K, V, input type, gradient type, masked): every size with every (K, V); `types` 2: with every pair of element types, 1:
    the pairs go round.  The (7, 7) and (1, 1) calls carry a valid mask — and count D on the device —, the (7, 1) calls none."""
    res = []
    for n, (M, (K, V)) in enumerate(itertools.product(SIZES, KV)):
        pairs = list(itertools.product(TYPES, TYPES))
        for dt, gt in pairs if types == 2 else [pairs[n % 4]]:
            res.append((M, K, V, dt, gt, V == K))
    return res


def shape_id(s):
    return f"M{s[0]}-K{s[1]}-V{s[2]}-{np.dtype(s[3]).name}-grad_{np.dtype(s[4]).name}" + ("-masked" if s[5] else "")


@pytest.fixture(scope="module")
def batch_of():
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = engines.make(kind, 4, 1)
        return made[kind]
    yield get
    for b in made.values():
        b.close()


def grad_scale_for(gt):
    return 1.0 if np.dtype(gt) == np.float32 else 1024.0          # (float16 gradients: the range an AMP loss scale is for)


# ---------------------------------------------------------------- 1. bit equality
def ppo_bits(kind, b, inp, gt):
    """A PPO call with entropy_loss = 0 against the float32 model: the per-sample outputs bit for bit, every entry written, zeros
    outside the piece's plane, nothing past M (Buf.get checks the guard bytes), D exact -> (outputs, model)"""
    M, K, V = inp["pi"].shape[0], inp["pi"].shape[3], inp["v"].shape[1]
    prm = Params(0.15, 0.3, 1.0, 0.0, 0.05, 1.0, 2.0)
    gs = grad_scale_for(gt)
    call = PpoCall(kind, b, inp, prm, grad_dtype=gt, grad_scale=gs)
    b.ppo_loss_dev(call.l)
    got = call.get()
    m = ppo_model(F32, inp["pi"], inp["v"], inp["action"], inp["old"], inp["adv"], inp["target"], inp["valid"], prm, gs)
    for row, name in ((0, "p"), (1, "ratio"), (2, "pl"), (5, "val")):
        assert same_bits(got["terms"][row], m[name]), f"'{name}' differs in samples {np.nonzero(got['terms'][row] != m[name])[0][:8]}"
    want, want_v = expand(m["g"], m["k"], K, gt), expand_v(m["gv"], m["k"], V, gt)
    assert written(got["grad_pi"], want) and written(got["grad_v"], want_v) and written(got["terms"]) and written(got["stats"])
    assert same_bits(got["grad_v"], want_v), "grad_v"
    assert same_bits(got["grad_pi"], want), f"grad_pi differs in samples {np.unique(np.nonzero(got['grad_pi'] != want)[0])[:8]}"
    other = np.ones((M, 40, K), bool)
    other[np.arange(M), :, m["k"]] = False
    assert not got["grad_pi"].reshape(M, 40, K)[other].any(), "a non-zero outside the piece's plane"
    assert got["stats"][0] == m["D"] and got["stats"][4] == 0.0
    return got, m


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("shape", shapes(), ids=shape_id)
def test_ppo_equals_the_model_bit_for_bit(kind, shape, batch_of):
    """entropy_loss = 0 leaves the policy part of grad_pi alone: probability, ratio, pl, val, grad_v and all of grad_pi carry the
    model's bits.  Every entry of both gradient arrays is written, zeros outside the piece's plane, nothing past M."""
    M, K, V, dt, gt, masked = shape
    rng = np.random.default_rng(100 * M + 10 * K + V)
    inp = ppo_inputs(rng, M, K, V, dt, masked)
    got, m = ppo_bits(kind, batch_of(kind), inp, gt)
    if M == 257:                                                  # every branch occurred
        ok, ratio, cl, A = m["ok"], m["ratio"], m["cl"], m["A"]
        for sign in (A > 0, A < 0):
            assert (ok & sign & (ratio < cl)).any() and (ok & sign & (ratio == cl)).any() and (ok & sign & (ratio > cl)).any()
        p = inp["pi"].reshape(M, 40, K)[np.arange(M), m["c"], m["k"]]
        assert (ok & (p < 1e-6)).any() and (ok & (inp["old"] == 0)).any() and (ok & (inp["old"] > 0) & (inp["old"] < 1e-6)).any()
        plane = inp["pi"].reshape(M, 40, K)[np.arange(M), :, m["k"]]
        assert (ok & ((plane == 0).sum(axis=1) == 39)).any(), "no one-hot map"
        a = inp["action"]
        assert (a[:, 0] > 3).any() and (a[:, 1] > 9).any() and (a[:, 2] > K - 1).any()
        if masked:
            assert not ok[0] and not ok[M - 1] and not ok[64:192].all() and ok.sum() > 200


def dqn_bits(kind, b, inp, gt, optimistic, gs):
    """A DQN call against the float32 model: q, new_prio and all of grad_Q bit for bit, every entry written, nothing past M, D and
    Dnz exact -> (the call, outputs, model)"""
    K = inp["Q"].shape[3]
    call = DqnCall(kind, b, inp, grad_dtype=gt, optimistic=optimistic, grad_scale=gs)
    b.dqn_loss_dev(call.l)
    got = call.get()
    m = dqn_model(F32, inp["Q"], inp["action"], inp["target"], inp["weight"], inp["valid"], optimistic, gs)
    want = expand(m["g"], m["k"], K, gt)
    assert written(got["grad_Q"], want) and all(written(a) for name, a in got.items() if name != "grad_Q")
    assert same_bits(got["q"], m["q"]) and same_bits(got["new_prio"], m["prio"])
    assert same_bits(got["grad_Q"], want), f"grad_Q differs in samples {np.unique(np.nonzero(got['grad_Q'] != want)[0])[:8]}"
    assert got["stats"][0] == m["D"] and got["stats"][1] == m["Dnz"]
    return call, got, m


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("shape", [s[:2] + s[3:] for s in shapes() if s[2] == 1], ids=lambda s: f"M{s[0]}-K{s[1]}-{np.dtype(s[2]).name}-grad_{np.dtype(s[3]).name}")
def test_dqn_equals_the_model_bit_for_bit(kind, shape, batch_of):
    """q, new_prio and all of grad_Q, with weights (some of them 0) and a valid mask on the K = 1 calls and the plain mean on the
    others; optimistic priorities on every second size."""
    M, K, dt, gt, masked = shape
    rng = np.random.default_rng(7 * M + K)
    inp = dqn_inputs(rng, M, K, dt, masked, weighted=masked or M == 65)
    _, got, m = dqn_bits(kind, batch_of(kind), inp, gt, 0.25 if M % 2 else 0.0, grad_scale_for(gt))
    if M == 257 and masked:
        assert (m["ok"] & (inp["weight"] == 0)).any() and not m["ok"][0] and not m["ok"][M - 1] and not m["ok"][64:192].all()
        a = inp["action"]
        assert (a[:, 0] > 3).any() and (a[:, 1] > 9).any() and (a[:, 2] > K - 1).any()


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("dt", TYPES, ids=["float32", "float16"])
def test_a_call_without_a_valid_sample_gives_zeros(kind, dt, batch_of):
    """D == 0 (the reference would give NaN): every output of both heads is written, and is zero"""
    M, K = 65, 7
    rng = np.random.default_rng(3)
    inp = ppo_inputs(rng, M, K, K, dt, True)
    inp["valid"][:] = 0
    call = PpoCall(kind, batch_of(kind), inp, PARAM_SETS[0], grad_dtype=dt)
    batch_of(kind).ppo_loss_dev(call.l)
    for name, a in call.get().items():
        assert written(a) and not a.any(), name
    dq = dqn_inputs(rng, M, K, dt, True, True)
    dq["valid"][:] = 0
    call = DqnCall(kind, batch_of(kind), dq, grad_dtype=dt, optimistic=0.5)
    batch_of(kind).dqn_loss_dev(call.l)
    for name, a in call.get().items():
        assert written(a) and not a.any(), name
    dq["valid"][:] = 1
    dq["weight"][:] = 0                                           # Dnz == 0 with D > 0: no loss, no gradient, the other statistics stay
    call = DqnCall(kind, batch_of(kind), dq, grad_dtype=dt)
    batch_of(kind).dqn_loss_dev(call.l)
    got = call.get()
    assert not got["grad_Q"].any() and got["stats"][0] == M and got["stats"][1] == 0 and got["stats"][2] == 0 and got["new_prio"].any()


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_no_samples_zeroes_the_statistics(kind, batch_of):
    inp = ppo_inputs(np.random.default_rng(4), 1, 7, 1, np.float32, False)
    call = PpoCall(kind, batch_of(kind), inp, PARAM_SETS[0], m=0)
    batch_of(kind).ppo_loss_dev(call.l)
    got = call.get()
    assert written(got["stats"]) and not got["stats"].any() and not written(got["grad_pi"]) and not written(got["grad_v"])


# ---------------------------------------------------------------- 2. what passes through the logarithm
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("eps", [0.05, 0.9])
@pytest.mark.parametrize("shape", shapes(types=1), ids=shape_id)
def test_entropy_outputs_against_float64(kind, eps, shape, batch_of):
    """H, bonus and the entropy part of grad_pi against the same formulas in float64.
    H: TOL_H = 5e-5 (above).  bonus = bonus0 + cr (Hmax - bonus0) with bonus0 = H - cf relu(floor - H): the error of H enters
    with |1 - cr| (1 + cf), and the six roundings of these two lines are each below 2^-24 of the largest magnitude they handle,
    |H| + cf |floor - H| + cr (Hmax + |bonus0|) + |bonus|; four times their sum.  grad_pi's entropy part is (ce e_j) grad_scale: TOL_E
    (above) on e_j times |ce grad_scale|, plus the seven roundings of ce, of the product and of the scale, 7 x 2^-24 |g|, times
    four; a float16 gradient adds its own rounding, 2^-11 |g| and 2^-25 below the normal range.  The branch [H < floor] cannot
    flip: every H of the float64 model is at least 1e-3 from the floor, which the test asserts; with the one-hot and the nearly
    uniform maps of the inputs the samples of a batch of 33 or more lie on both sides of either floor."""
    M, K, V, dt, gt, masked = shape
    rng = np.random.default_rng(1000 * M + 10 * K + V)
    inp = ppo_inputs(rng, M, K, V, dt, masked)
    prm = Params(0.15, 0.3, 0.0, 0.01, eps, 1.0, 0.5)             # policy_loss = 0: grad_pi is its entropy part (the policy part: section 1)
    gs = grad_scale_for(gt) * 64.0
    call = PpoCall(kind, batch_of(kind), inp, prm, grad_dtype=gt, grad_scale=gs)
    batch_of(kind).ppo_loss_dev(call.l)
    got = call.get()
    m = ppo_model(F64, inp["pi"], inp["v"], inp["action"], inp["old"], inp["adv"], inp["target"], inp["valid"], prm, gs)
    ok = m["ok"]
    assert (np.abs(m["H"] - m["floor"])[ok] >= 1e-3).all(), "an entropy of the inputs lies within 1e-3 of the floor"
    if M >= 33:
        assert (ok & (m["H"] < m["floor"])).any() and (ok & (m["H"] > m["floor"])).any()
    err_h = np.abs(got["terms"][3] - m["H"])
    scale = np.abs(m["H"]) + prm.cf * np.abs(m["floor"] - m["H"]) + prm.cr * (3.7 + np.abs(m["bonus0"])) + np.abs(m["bonus"])
    tol_b = abs(1 - prm.cr) * (1 + prm.cf) * TOL_H + 4 * 6 * U24 * scale
    err_b = np.abs(got["terms"][4] - m["bonus"])
    want = expand(m["g"], m["k"], K, F64)
    assert not m["g_policy"].any()
    tol_g = 4 * (np.abs(m["ce"])[:, None] * (TOL_E / 4) + 7 * U24 * np.abs(m["g"]))
    if np.dtype(gt) == np.float16:
        assert np.abs(m["g"]).max() < 6e4, "the scaled gradients leave the range of a float16"
        tol_g = tol_g + 2.0 ** -11 * np.abs(m["g"]) + 2.0 ** -25
    err_g = np.abs(got["grad_pi"].astype(F64) - want)
    print(f"H: largest error {err_h.max():.3g} (allowed {TOL_H:.3g}); bonus: {err_b.max():.3g} ({tol_b.min():.3g}); "
          f"grad_pi: {err_g.max():.3g}, largest share of its tolerance {(err_g / expand(tol_g, m['k'], K, F64).clip(1e-300)).max():.3g}")
    assert (err_h < TOL_H).all() and (err_b <= tol_b).all()
    assert (err_g <= expand(tol_g, m["k"], K, F64)).all()


def test_the_entropy_constants():
    capi = ge.package().capi
    for eps in (0.05, 0.3, 0.9):
        assert capi.ppo_entropy_constants(eps) == pytest.approx(entropy_constants(eps), rel=1e-15)
    assert entropy_constants(0.05)[1] == pytest.approx(np.log(40.0), abs=1e-6)
    for eps in (0.0, 1.0, -0.5, 2.0):                              # the reference's expression is NaN there: the floor term is switched off
        assert capi.ppo_entropy_constants(eps)[0] == 0.0


# ---------------------------------------------------------------- 3. the model against autograd of the reference's expression
@pytest.mark.parametrize("prm", PARAM_SETS, ids=["set0", "set1", "set2"])
@pytest.mark.parametrize("K,V,masked", [(7, 7, False), (7, 1, True), (1, 1, False)])
def test_the_float64_model_against_torch_autograd_ppo(prm, K, V, masked):
    """d loss / d pi and d loss / d v of the float64 model against torch autograd (float64, CPU) of create_training_ops written
    with torch ops, 1e-10 of the largest gradient; inputs without exact ties (no zero in a map, no ratio on a clip bound).  With
    the bit equality and the float64 comparison above this pins the kernels to the reference's loss."""
    import torch
    M = 257
    rng = np.random.default_rng(11 + K + V)
    inp = ppo_inputs(rng, M, K, V, np.float32, masked, ties=False)
    m = ppo_model(F64, inp["pi"], inp["v"], inp["action"], inp["old"], inp["adv"], inp["target"], inp["valid"], prm)
    assert (m["ratio"] != 1 - F64(F32(prm.clip))).all() and (m["ratio"] != 1 + F64(F32(prm.clip))).all() and (inp["pi"] > 0).all()
    assert (m["ok"] & (m["H"] < m["floor"])).any() or prm.eps < 0.5
    pi = torch.from_numpy(inp["pi"].astype(F64)).requires_grad_()
    v = torch.from_numpy(inp["v"].astype(F64)).requires_grad_()
    loss = torch_ppo_loss(torch, pi, v, inp["action"], inp["old"], inp["adv"], inp["target"], m["ok"], prm)
    g_pi, g_v = torch.autograd.grad(loss, (pi, v))
    want_pi, want_v = g_pi.numpy(), g_v.numpy()
    err_pi = np.abs(expand(m["g"], m["k"], K, F64) - want_pi).max()
    err_v = np.abs(expand_v(m["gv"], m["k"], V, F64) - want_v).max()
    print(f"largest gradients {np.abs(want_pi).max():.3g} / {np.abs(want_v).max():.3g}, largest differences {err_pi:.3g} / {err_v:.3g}")
    assert err_pi <= 1e-10 * np.abs(want_pi).max() and err_v <= 1e-10 * np.abs(want_v).max()
    total = m["terms"][m["ok"]].sum(axis=0) / m["D"]
    mine = F64(F32(prm.c1)) * total[0] - F64(F32(prm.c2)) * total[1] - F64(F32(prm.c3)) * total[2]
    assert mine == pytest.approx(float(loss.detach()), rel=1e-12, abs=1e-12)


@pytest.mark.parametrize("weighted", [False, True], ids=["mean", "weighted"])
@pytest.mark.parametrize("K", [7, 1])
def test_the_float64_model_against_torch_autograd_dqn(weighted, K):
    import torch
    M = 257
    inp = dqn_inputs(np.random.default_rng(13 + K), M, K, np.float32, weighted, weighted)
    inp["action"] = np.stack(np.unravel_index(np.arange(M) % (40 * K), (4, 10, K)), axis=1).astype(np.uint8)      # (no out-of-range entry: one_hot)
    m = dqn_model(F64, inp["Q"], inp["action"], inp["target"], inp["weight"], inp["valid"])
    Q = torch.from_numpy(inp["Q"].astype(F64)).requires_grad_()
    loss = torch_dqn_loss(torch, Q, inp["action"], inp["target"], inp["weight"], m["ok"])
    want = torch.autograd.grad(loss, Q)[0].numpy()
    err = np.abs(expand(m["g"], m["k"], K, F64) - want).max()
    print(f"largest gradient {np.abs(want).max():.3g}, largest difference {err:.3g}")
    assert err <= 1e-10 * np.abs(want).max()
    assert m["terms"][m["ok"], 0].sum() / m["Dnz"] == pytest.approx(float(loss.detach()), rel=1e-12)


# ---------------------------------------------------------------- 4. statistics
def stat_check(name, got, terms, coef, D, term_err=0.0, bound=None):
    """got against coef * sum(terms) / D in float64: the summation bound of the float32 sum — in any order, or `bound`, that of
    the stated order (loss_support.stated_bound) — plus the terms' own error, through the division and the product (two roundings,
    and one more for a sum of such statistics)"""
    terms = np.asarray(terms, F64)
    want = coef * terms.sum() / D
    tol = abs(coef) * ((sum_bound(terms) if bound is None else bound) + len(terms) * term_err) / D + 3 * U24 * abs(want) + 1e-45
    print(f"{name}: got {got:.9g}, want {want:.9g}, difference {abs(got - want):.3g}, allowed {tol:.3g}")
    assert abs(got - want) <= tol, name
    return want, tol


def ppo_stats_in_the_stated_order(got, m32, prm):
    """Every PPO statistic bit for bit: the sum of its per-sample float32 terms in the stated order, then loss_finish's division and
    products in float32.  The terms that carry the float32 model's bits come from the model (dv^2, pl, val, val^2, T, T^2,
    [ratio != cl], ratio); H and bonus, which pass through the logarithm, are the rows the call itself wrote to `terms` — the header
    sums the very values it writes, and section 2 holds those rows against float64 —, and H^2 is the float32 square of that H."""
    t = m32["terms"].copy()
    H, bonus = got["terms"][3], got["terms"][4]
    t[:, 2], t[:, 3], t[:, 4] = bonus, H, H * H
    want = ppo_stated_stats(t, m32["D"], prm)
    for slot, name in enumerate(PPO_STATS):
        assert same_bits(got["stats"][slot], want[slot]), f"'{name}' is {got['stats'][slot]!r}, the sum in the stated order gives {want[slot]!r}"
    assert not got["stats"][len(PPO_STATS):].any()


def dqn_stats_in_the_stated_order(got, m32):
    """Every DQN statistic bit for bit: the float32 model's per-sample terms summed in the stated order, divided in float32"""
    want = dqn_stated_stats(m32["terms"], m32["D"], m32["Dnz"])
    for slot, name in enumerate(DQN_STATS):
        assert same_bits(got["stats"][slot], want[slot]), f"'{name}' is {got['stats'][slot]!r}, the sum in the stated order gives {want[slot]!r}"
    assert not got["stats"][len(DQN_STATS):].any()


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("shape", shapes(types=1), ids=shape_id)
def test_ppo_statistics(kind, shape, batch_of):
    """Every statistic against the float64 sum of the model's per-sample terms: the float32 model's for the terms that carry its
    bits (section 1), the float64 model's with the per-term tolerance of section 2 for H, H^2 and bonus; (n - 1) 2^-24 sum |x_i|
    holds for any order of the sum.  Then every statistic bit for bit against the sum in the stated order
    (ppo_stats_in_the_stated_order).  D and clip_saturation D are integers.  A second call gives the same bits everywhere."""
    M, K, V, dt, gt, masked = shape
    rng = np.random.default_rng(50 * M + K + V)
    inp = ppo_inputs(rng, M, K, V, dt, masked)
    prm = PARAM_SETS[2]
    call = PpoCall(kind, batch_of(kind), inp, prm, grad_dtype=gt, grad_scale=128.0)
    batch_of(kind).ppo_loss_dev(call.l)
    got = call.get()
    stats = dict(zip(PPO_STATS, got["stats"].astype(F64)))
    args = (inp["pi"], inp["v"], inp["action"], inp["old"], inp["adv"], inp["target"], inp["valid"], prm, 128.0)
    m32, m64 = ppo_model(F32, *args), ppo_model(F64, *args)
    ok, D = m32["ok"], m32["D"]
    assert stats["n"] == D and not got["stats"][len(PPO_STATS):].any()
    if D == 0:                                                    # (M = 1 with its sample masked)
        assert not got["stats"].any()
        return
    saturated = int((m32["ratio"] != m32["cl"])[ok].sum())          # (the mean is a rounded quotient: it gives the integer back to 2^-23)
    assert round(stats["clip_saturation"] * D) == saturated and abs(stats["clip_saturation"] * D - saturated) <= 2 * U24 * saturated
    t32, t64 = m32["terms"][ok].astype(F64), m64["terms"][ok]
    scale = np.abs(m64["H"]) + prm.cf * np.abs(m64["floor"] - m64["H"]) + prm.cr * (3.7 + np.abs(m64["bonus0"])) + np.abs(m64["bonus"])
    tol_b = float((abs(1 - prm.cr) * (1 + prm.cf) * TOL_H + 4 * 6 * U24 * scale).max())
    c1, c2, c3 = (float(F32(z)) for z in (prm.c1, prm.c2, prm.c3))
    vl = stat_check("value_loss", stats["value_loss"], t32[:, 0], c1, D)
    pol = stat_check("policy_loss", stats["policy_loss"], t32[:, 1], -c2, D)
    ent = stat_check("entropy_loss", stats["entropy_loss"], t64[:, 2], -c3, D, tol_b)
    want = vl[0] + pol[0] + ent[0]
    tol = vl[1] + pol[1] + ent[1] + 2 * U24 * (abs(vl[0]) + abs(pol[0]) + abs(ent[0]))
    print(f"loss: got {stats['loss']:.9g}, want {want:.9g}, allowed {tol:.3g}")
    assert abs(stats["loss"] - want) <= tol
    stat_check("entropy", stats["entropy"], t64[:, 3], 1.0, D, TOL_H)
    stat_check("entropy_sq", stats["entropy_sq"], t64[:, 4], 1.0, D, 2 * 3.7 * TOL_H + TOL_H ** 2 + U24 * 13.7)
    stat_check("entropy_bonus", stats["entropy_bonus"], t64[:, 2], 1.0, D, tol_b)
    for name, col in (("values", 5), ("values_sq", 6), ("target_values", 7), ("target_values_sq", 8), ("clip_saturation", 9), ("ratio", 10)):
        stat_check(name, stats[name], t32[:, col], 1.0, D)
    ppo_stats_in_the_stated_order(got, m32, prm)
    batch_of(kind).ppo_loss_dev(call.l)
    again = call.get()
    for name in got:
        assert got[name].tobytes() == again[name].tobytes(), f"'{name}' of a second call differs"


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("shape", [s[:2] + s[3:] for s in shapes(types=1) if s[2] == 1], ids=lambda s: f"M{s[0]}-K{s[1]}-{np.dtype(s[2]).name}-grad_{np.dtype(s[3]).name}")
def test_dqn_statistics(kind, shape, batch_of):
    """Every statistic against the float64 sum of the float32 model's per-sample terms within the bound of any order, then bit for
    bit against the sum in the stated order (dqn_stats_in_the_stated_order); a second call gives the same bits everywhere."""
    M, K, dt, gt, masked = shape
    inp = dqn_inputs(np.random.default_rng(9 * M + K), M, K, dt, masked, weighted=True)
    call = DqnCall(kind, batch_of(kind), inp, grad_dtype=gt, optimistic=0.5, grad_scale=128.0)
    batch_of(kind).dqn_loss_dev(call.l)
    got = call.get()
    stats = dict(zip(DQN_STATS, got["stats"].astype(F64)))
    m = dqn_model(F32, inp["Q"], inp["action"], inp["target"], inp["weight"], inp["valid"], 0.5, 128.0)
    ok, D, Dnz = m["ok"], m["D"], m["Dnz"]
    assert stats["n"] == D and stats["n_weighted"] == Dnz == (ok & (inp["weight"] != 0)).sum() and not got["stats"][len(DQN_STATS):].any()
    t = m["terms"][ok].astype(F64)
    if Dnz:
        stat_check("loss", stats["loss"], t[:, 0], 1.0, Dnz)
    else:
        assert stats["loss"] == 0
    for name, col in (("q_val", 1), ("q_val_sq", 2), ("q_target", 3), ("q_target_sq", 4), ("new_prio", 5)):
        if D:
            stat_check(name, stats[name], t[:, col], 1.0, D)
    dqn_stats_in_the_stated_order(got, m)
    batch_of(kind).dqn_loss_dev(call.l)
    again = call.get()
    for name in got:
        assert got[name].tobytes() == again[name].tobytes(), f"'{name}' of a second call differs"


# ---------------------------------------------------------------- 4a. the model of the stated order
@pytest.mark.parametrize("block", [BLOCK, 16], ids=["block64", "block16"])
def test_the_model_of_the_stated_order(block):
    """loss_support.stated_sum against the sentence of tetris_loss.h (STATISTICS) written as plain scalar loops, on 515 blocks
    with a short last one (slots 0, 1 and 2 take three rows): the same bits in every column.  And the sentence is not idle at
    that size: adding the same rows without slots, or into their slots in descending b, gives other bits in some column."""
    rng = np.random.default_rng(block)
    M = 515 * block - block // 2 - 1
    terms = rng.standard_normal((M, 6)) * 10.0 ** rng.uniform(-1, 1, (M, 1))
    # (only slots 0, 1 and 2 hold three rows, and only there can the order of a slot's rows show; their nine blocks weigh 1024
    # times the others, so that a last bit of theirs is not rounded away on the way through the slots' tree)
    heavy = np.isin(np.arange(M) // block, [0, 1, 2, 256, 257, 258, 512, 513, 514])
    terms = np.where(heavy[:, None], 1024.0 * terms, terms).astype(F32)
    stated = stated_sum(terms, block)
    assert stated.dtype == F32 and stated.shape == (6,)
    for col in range(6):
        assert same_bits(stated[col], loop_sum(terms[:, col], block)), f"column {col}"
        assert same_bits(stated[col], stated_sum(terms[:, col], block)), "a single column"
    assert (stated != stated_sum(terms, block, "slotless")).any(), "the slots change nothing"
    assert (stated != stated_sum(terms, block, "descending")).any(), "the order of a slot's rows changes nothing"
    few = terms[:3 * block + 1]                                   # fewer blocks than slots: every slot holds one row or none
    assert same_bits(stated_sum(few, block), stated_sum(few, block, "descending"))


# ---------------------------------------------------------------- 4b. batches whose loops take a second trip
def carry_shapes():
    """(M, K, V, input type, gradient type, last_valid, span) at the sizes of loss_support.CARRY_SIZES — the count of D and Dnz is
    one workgroup of 1024 lanes that strides over M, the reduction of the blocks' partial rows one of 256 lanes that strides over
    the blocks of 64:
      M = 1025 = 16 x 64 + 1    one lane of the count has a second trip; 17 blocks
      M = 5123 = 5 x 1024 + 3   lanes 0-2 count six samples, the others five; 81 blocks
      M = 16385 = 256 x 64 + 1  17 trips of the count; 257 blocks: slot 0 takes a second row, and the last block holds one sample
      M = 32833 = 513 x 64 + 1  33 trips; 514 blocks: slots 0 and 1 take a third row
    Every size with every (K, V), the element type pairs going round.  Every call carries a valid mask (loss_support.carry_mask):
    the second (K, V) of a size has its last sample — at every size the only one of its block — valid, the others invalid; from
    M = 5123 on every mask has 1024 consecutive invalid samples, so D lies more than 1024 below M.  At M = 1025 such a run leaves
    one sample at most, so no D there can lie more than 1024 from M without being 0: the third (K, V) takes the run, with the
    last sample valid (D = 1), and the other two do without."""
    res = []
    pairs = list(itertools.product(TYPES, TYPES))
    for n, (M, (i, (K, V))) in enumerate(itertools.product(CARRY_SIZES, enumerate(KV))):
        dt, gt = pairs[n % 4]
        res.append((M, K, V, dt, gt, i == 1 or (M == 1025 and i == 2), M > 1025 or i == 2))
    return res


def carry_id(s):
    return f"M{s[0]}-K{s[1]}-V{s[2]}-{np.dtype(s[3]).name}-grad_{np.dtype(s[4]).name}-last_{'valid' if s[5] else 'invalid'}" + ("-run1024" if s[6] else "")


def check_carry_counts(M, ok, D, last_valid, span):
    """the mask is what the case needs, and a count that drops or doubles a trip of 1024 lanes cannot land on this D"""
    assert_carry_mask(ok, BLOCK, last_valid, span)
    assert D == ok.sum() and D % 1024 != 0
    if M > 1025:
        assert M - D > 1024


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("shape", carry_shapes(), ids=carry_id)
def test_ppo_equals_the_model_bit_for_bit_across_the_carries(kind, shape, batch_of):
    """Section 1's comparison (ppo_bits) at the sizes of carry_shapes: every per-sample output and both gradient arrays bit for
    bit, D exact; and with entropy_loss = 0 every statistic in the stated order."""
    M, K, V, dt, gt, last_valid, span = shape
    rng = np.random.default_rng(100 * M + 10 * K + V)
    inp = ppo_inputs(rng, M, K, V, dt, True)
    inp["valid"] = carry_mask(rng, M, BLOCK, last_valid, span)
    weigh_the_full_slots(inp["target"], BLOCK)
    got, m = ppo_bits(kind, batch_of(kind), inp, gt)
    check_carry_counts(M, m["ok"], got["stats"][0], last_valid, span)
    ppo_stats_in_the_stated_order(got, m, Params(0.15, 0.3, 1.0, 0.0, 0.05, 1.0, 2.0))


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("shape", carry_shapes(), ids=carry_id)
def test_ppo_statistics_across_the_carries(kind, shape, batch_of):
    """With every loss coefficient non-zero: D exact; H and bonus of every sample against float64 within section 2's tolerances
    (so that summing the written rows is not circular); every statistic bit for bit in the stated order; entropy_sq also against
    the float64 sum with the bound of the stated order (loss_support.stated_bound) and section 4's per-term error of H^2 — at
    M = 32833 that bound is a thirtieth of one sample's share, where the any-order bound exceeds a whole block's —; a second call
    gives the same bytes in every output."""
    M, K, V, dt, gt, last_valid, span = shape
    rng = np.random.default_rng(50 * M + K + V)
    inp = ppo_inputs(rng, M, K, V, dt, True)
    inp["valid"] = carry_mask(rng, M, BLOCK, last_valid, span)
    weigh_the_full_slots(inp["target"], BLOCK)
    prm = PARAM_SETS[2]
    b = batch_of(kind)
    call = PpoCall(kind, b, inp, prm, grad_dtype=gt, grad_scale=128.0)
    b.ppo_loss_dev(call.l)
    got = call.get()
    args = (inp["pi"], inp["v"], inp["action"], inp["old"], inp["adv"], inp["target"], inp["valid"], prm, 128.0)
    m32, m64 = ppo_model(F32, *args), ppo_model(F64, *args)
    ok, D = m32["ok"], m32["D"]
    assert written(got["terms"]) and written(got["stats"])        # (the gradient arrays: the test above)
    check_carry_counts(M, ok, got["stats"][0], last_valid, span)
    assert got["stats"][0] == D
    scale = np.abs(m64["H"]) + prm.cf * np.abs(m64["floor"] - m64["H"]) + prm.cr * (3.7 + np.abs(m64["bonus0"])) + np.abs(m64["bonus"])
    tol_b = abs(1 - prm.cr) * (1 + prm.cf) * TOL_H + 4 * 6 * U24 * scale
    assert (np.abs(m64["H"] - m64["floor"])[ok] >= 1e-3).all(), "an entropy of the inputs lies within 1e-3 of the floor"
    assert (np.abs(got["terms"][3] - m64["H"]) < TOL_H).all() and (np.abs(got["terms"][4] - m64["bonus"]) <= tol_b).all()
    ppo_stats_in_the_stated_order(got, m32, prm)
    t64 = m64["terms"][ok]
    stat_check("entropy_sq", float(got["stats"][6]), t64[:, 4], 1.0, D, 2 * 3.7 * TOL_H + TOL_H ** 2 + U24 * 13.7, bound=stated_bound(t64[:, 4], BLOCK))
    b.ppo_loss_dev(call.l)
    again = call.get()
    for name in got:
        assert got[name].tobytes() == again[name].tobytes(), f"'{name}' of a second call differs"


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("shape", carry_shapes(), ids=carry_id)
def test_dqn_across_the_carries(kind, shape, batch_of):
    """The DQN head at the sizes of carry_shapes, with the mask of each case and weights, every sixth of them 0 (the three cases of
    a size differ in K, in the element types and in the mask; V is no argument of this head): q, new_prio and all of grad_Q bit for
    bit, D and Dnz exact, every statistic bit for bit in the stated order, and a second call with the same bytes."""
    M, K, _, dt, gt, last_valid, span = shape
    rng = np.random.default_rng(9 * M + K)
    inp = dqn_inputs(rng, M, K, dt, True, True)
    inp["valid"] = carry_mask(rng, M, BLOCK, last_valid, span)
    weigh_the_full_slots(inp["target"], BLOCK)
    call, got, m = dqn_bits(kind, batch_of(kind), inp, gt, 0.5, 128.0)
    check_carry_counts(M, m["ok"], got["stats"][0], last_valid, span)
    zero_weight = m["ok"] & (inp["weight"] == 0)
    assert got["stats"][1] == m["Dnz"] == m["D"] - zero_weight.sum() and (zero_weight.any() or m["D"] == 1)
    dqn_stats_in_the_stated_order(got, m)
    batch_of(kind).dqn_loss_dev(call.l)
    again = call.get()
    for name in got:
        assert got[name].tobytes() == again[name].tobytes(), f"'{name}' of a second call differs"


# ---------------------------------------------------------------- 4c. the scratch buffer across sizes
def same_outputs(a, b, what):
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), f"{what}: '{name}' differs"


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("head", ["ppo", "dqn"])
def test_the_scratch_buffer_grows_between_calls(kind, head):
    """On a batch of its own, so that the first call finds no scratch: a call at M = 33 (one partial row), one at M = 32833 (514
    rows: the scratch is replaced while the first call may still run) and the first again, enqueued one after the other — the
    outputs are read only after the third.  The third call's outputs are the first's byte for byte, the large call's are those
    of the same call on a fresh batch, and no error is pending."""
    rng = np.random.default_rng(33)
    if head == "ppo":
        small, large = (ppo_inputs(rng, M, 7, 7, np.float32, True) for M in (33, CARRY_SIZES[-1]))
        make = lambda b, inp: PpoCall(kind, b, inp, PARAM_SETS[2], grad_scale=128.0)                     # noqa: E731
    else:
        small, large = (dqn_inputs(rng, M, 7, np.float32, True, True) for M in (33, CARRY_SIZES[-1]))
        make = lambda b, inp: DqnCall(kind, b, inp, optimistic=0.5, grad_scale=128.0)                    # noqa: E731
    b, fresh = engines.make(kind, 4, 1), engines.make(kind, 4, 1)
    try:
        calls = [make(b, small), make(b, large), make(b, small)]
        for call in calls:
            (b.ppo_loss_dev if head == "ppo" else b.dqn_loss_dev)(call.l)
        first, big, third = (call.get() for call in calls)
        assert all(written(a) for got in (first, big, third) for a in got.values())
        assert first["stats"][0] == (small["valid"] != 0).sum() and big["stats"][0] == (large["valid"] != 0).sum() > 30000
        same_outputs(third, first, "the small call after the large one")
        alone = make(fresh, large)
        (fresh.ppo_loss_dev if head == "ppo" else fresh.dqn_loss_dev)(alone.l)
        same_outputs(big, alone.get(), "the large call after a small one")
        assert b.take_errors() == 0 and fresh.take_errors() == 0
    finally:
        b.close()
        fresh.close()


# ---------------------------------------------------------------- 5. argument rules
RULES = [("K = 3", "ppo", dict(n_pieces=3)), ("V = 2", "ppo", dict(n_values=2)), ("pi is NULL", "ppo", dict(pi=None)),
         ("grad_v is NULL", "ppo", dict(grad_v=None)), ("stats is NULL", "ppo", dict(stats=None)), ("negative M", "ppo", dict(m=-1)),
         ("negative clip", "ppo", dict(clipping_parameter=-0.1)), ("an unknown flag", "ppo", dict(flags=8)),
         ("K = 3", "dqn", dict(n_pieces=3)), ("Q is NULL", "dqn", dict(Q=None)), ("new_prio is NULL", "dqn", dict(new_prio=None)),
         ("negative M", "dqn", dict(m=-1)), ("an unknown flag", "dqn", dict(flags=2))]


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("rule", RULES, ids=[f"{r[1]}-{r[0].replace(' ', '_')}" for r in RULES])
def test_bad_arguments_are_refused(kind, rule, batch_of):
    pkg, b = ge.package(), batch_of(kind)
    rng = np.random.default_rng(1)
    if rule[1] == "ppo":
        call = PpoCall(kind, b, ppo_inputs(rng, 5, 7, 7, np.float32, True), PARAM_SETS[0], **rule[2])
        with pytest.raises(pkg.TetrisError):
            b.ppo_loss_dev(call.l)
    else:
        call = DqnCall(kind, b, dqn_inputs(rng, 5, 7, np.float32, True, True), **rule[2])
        with pytest.raises(pkg.TetrisError):
            b.dqn_loss_dev(call.l)
    assert not any(written(a) for a in call.get().values()), "a refused call wrote an output"
    with pytest.raises(pkg.TetrisError):
        (b.ppo_loss_dev if rule[1] == "ppo" else b.dqn_loss_dev)(None)


# ---------------------------------------------------------------- 6. TorchEnv: the heads inside a training step (GPU only)
def action_softmax(torch, x):
    """network_utils.action_softmax: over the 40 actions of every piece"""
    mx = x.amax(dim=(1, 2), keepdim=True)
    un = torch.exp(x - mx)
    return un / un.sum(dim=(1, 2), keepdim=True)


def composed_ppo(torch, pi, v, action, old, adv, target, valid, prm):
    """the same loss composed from torch ops on the device, float32"""
    M, K = pi.shape[0], pi.shape[3]
    a = action.long()
    rows = torch.arange(M, device=pi.device)
    plane = pi.reshape(M, 40, K)[rows, :, a[:, 2]]
    p = plane[rows, 10 * a[:, 0] + a[:, 1]]
    val = v[rows, a[:, 2]] if v.shape[1] == K else v[:, 0]
    e = 1e-6
    r = torch.clamp(p, min=e) / torch.clamp(old, min=e)
    pl = torch.minimum(r * adv, torch.clamp(r, 1 - prm.clip, 1 + prm.clip) * adv)
    q = plane + e
    H = -(q * torch.log(torch.clamp(q, min=e))).sum(dim=1)
    floor, hmax = entropy_constants(prm.eps)
    bonus = H - prm.cf * torch.relu(floor - H)
    bonus = bonus + prm.cr * (hmax - bonus)
    sel = valid != 0
    return prm.c1 * ((val - target) ** 2)[sel].mean() - prm.c2 * pl[sel].mean() - prm.c3 * bonus[sel].mean()


@pytest.mark.gpu
@pytest.mark.parametrize("M", [257, 64])
def test_ppo_loss_backward_matches_the_composed_loss(M):
    """te.ppo_loss(...).backward() on a small module — a linear layer to [M, 280] followed by the reference's action_softmax, and a
    linear value head — leaves the parameter gradients of the same loss composed from torch ops.  grad_scale = 128 is undone.
    Tolerance: the head's gradient with respect to pi differs from autograd's float32 one by the error of section 2 in the
    entropy part — TOL_E |ce| per element — and by float32 roundings elsewhere, a few 2^-24 of each element; both pass through the
    same backward of the module, a sum over M x 280 such elements per parameter: 1e-4 of the largest gradient of a parameter
    tensor leaves more than an order of magnitude (measured: printed)."""
    import torch
    pkg = ge.package()
    torch.manual_seed(M)
    dev = torch.device("cuda")
    b = pkg.TetrisBatch(8, 1, device=0)
    te = importlib.import_module("drl-tetris_amd.torch_interop").TorchEnv(b)
    K, F = 7, 24
    body, head = torch.nn.Linear(F, 280).to(dev), torch.nn.Linear(F, K).to(dev)
    feat = torch.randn(M, F, device=dev)
    rng = np.random.default_rng(M)
    inp = ppo_inputs(rng, M, K, K, np.float32, True, ties=False)
    action, adv, target, valid = (torch.from_numpy(inp[n]).to(dev) for n in ("action", "adv", "target", "valid"))
    prm = PARAM_SETS[2]

    def net():
        return action_softmax(torch, body(feat).reshape(M, 4, 10, K)), head(feat)
    with torch.no_grad():
        pi0, _ = net()
        a = action.long()
        p0 = pi0.reshape(M, 40, K)[torch.arange(M, device=dev), 10 * a[:, 0] + a[:, 1], a[:, 2]]
        old = (p0 / torch.from_numpy(np.choose(np.arange(M) % 3, [0.6, 1.01, 1.9]).astype(F32)).to(dev)).contiguous()
    params = list(body.parameters()) + list(head.parameters())
    pi, v = net()
    want_loss = composed_ppo(torch, pi, v, action, old, adv, target, valid, prm)
    want = torch.autograd.grad(want_loss, params, retain_graph=True)
    loss, stats = te.ppo_loss(pi, v, action, old, adv, target, valid, clipping_parameter=prm.clip, value_loss=prm.c1, policy_loss=prm.c2,
                              entropy_loss=prm.c3, ppo_epsilon=prm.eps, entropy_floor_loss=prm.cf, rescaled_entropy=prm.cr, grad_scale=128.0)
    loss.backward()
    torch.cuda.synchronize()
    assert float(loss.detach()) == pytest.approx(float(want_loss.detach()), rel=1e-5, abs=1e-6) and float(stats[0]) == float((valid != 0).sum())
    for prm_t, w in zip(params, want):
        got = prm_t.grad / 128.0
        err, top = float((got - w).abs().max()), float(w.abs().max())
        print(f"parameter {tuple(prm_t.shape)}: largest gradient {top:.3g}, largest difference {err:.3g}")
        assert err <= 1e-4 * top
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("M", [257, 64])
def test_dqn_loss_backward_and_new_prios_reach_the_replay(M):
    """te.dqn_loss(...).backward() against the weighted mean squared error composed from torch ops (float32 roundings only: 1e-5 of
    the largest gradient), and its new_prio through Replay.update_prios: the ring's prio changes at the sampled indices, there
    only."""
    import torch
    pkg = ge.package()
    torch.manual_seed(M)
    dev = torch.device("cuda")
    b = pkg.TetrisBatch(8, 1, device=0)
    te = importlib.import_module("drl-tetris_amd.torch_interop").TorchEnv(b)
    K, F = 7, 24
    body = torch.nn.Linear(F, 280).to(dev)
    feat = torch.randn(M, F, device=dev)
    inp = dqn_inputs(np.random.default_rng(M), M, K, np.float32, False, True)
    inp["action"][:, 0] %= 4
    inp["action"][:, 1] %= 10
    inp["action"][:, 2] %= K
    action, target = (torch.from_numpy(inp[n]).to(dev) for n in ("action", "target"))
    rp = te.replay(4 * M, k_step=1)
    rp.prio.copy_(torch.rand(rp.max_size, device=dev))
    rp.cursor[1] = rp.max_size                                    # a full ring: the sample's indices and importance weights
    index, weight, count = rp.sample(M, 0.7, 0.5, draw=3)
    assert int(count) == M and len(torch.unique(index)) == M
    a = action.long()
    rows = torch.arange(M, device=dev)
    Q = body(feat).reshape(M, 4, 10, K)
    q = Q.reshape(M, 40, K)[rows, 10 * a[:, 0] + a[:, 1], a[:, 2]]
    want_loss = (weight * (q - target) ** 2).sum() / (weight != 0).sum()
    want = torch.autograd.grad(want_loss, list(body.parameters()), retain_graph=True)
    loss, stats, new_prio = te.dqn_loss(Q, action, target, weight, grad_scale=128.0)
    loss.backward()
    torch.cuda.synchronize()
    assert float(loss.detach()) == pytest.approx(float(want_loss.detach()), rel=1e-5)
    for prm_t, w in zip(body.parameters(), want):
        err, top = float((prm_t.grad / 128.0 - w).abs().max()), float(w.abs().max())
        print(f"parameter {tuple(prm_t.shape)}: largest gradient {top:.3g}, largest difference {err:.3g}")
        assert err <= 1e-5 * top
    assert torch.equal(new_prio, (q - target).abs().detach())
    before = rp.prio.clone()
    rp.update_prios(index, new_prio)
    torch.cuda.synchronize()
    assert torch.equal(rp.prio[index.long()], new_prio)
    rest = torch.ones(rp.max_size, dtype=torch.bool, device=dev)
    rest[index.long()] = False
    assert torch.equal(rp.prio[rest], before[rest]) and not torch.equal(rp.prio, before)
    b.close()
