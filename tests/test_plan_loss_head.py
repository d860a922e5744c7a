"""The planning loss head on the device (include/tetris_hip.h: tetris_plan_loss_dev) against the model of
tests/plan_loss_support.py, written from the definition: bit equality in float32 for everything that does not pass through the
logarithm, the same formulas in float64 with a derived tolerance for what does, the float64 model's gradients against torch
autograd of the reference's expressions, the statistics against float64 sums with the standard summation bound and bit for bit
against the sum in the stated order, determinism, all of this again at batch sizes where the count of D and the reduction of the
blocks' rows go round more than once, the scratch buffer across sizes, the reference's own recorded planes, the argument rules, and on the GPU the TorchEnv wrappers inside a small training step.  The
records are made by the library's own calls (record_plan over crafted lists) and the model is fed what batch_plan expands from
them.  Every test but the torch ones runs on the CPU harness (`-m "not gpu"`) and on the MI355X (`-m gpu`); on the harness the
"device" buffers are numpy arrays."""
import importlib
import itertools

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import engines
from tests.buffers import MIRROR
from tests.plan_loss_support import (BLOCK, E32, F32, F64, PARAM_SETS, STATS, U24, PlanLossCall, PlanParams, assert_carry_mask, carry_mask,
                                     crafted_window, entropy_tolerances, expand, expand_v, golden_window, named, ok_of, plan_inputs, plan_model,
                                     plan_stated_stats, same_bits, sample_index, stated_bound, sum_bound, torch_plan_loss, weigh_the_full_slots, with_old, written)

SIZES = (1, 3, 16, 17, 33)            # one sample, a few, a block of 16, a block and one, two blocks and one
HEIGHTS = (20, 7)                     # 200 cells: four cells in some lanes, three in others; 70 cells: lanes with one and with none
KV = ((7, 1), (7, 7), (1, 1))
TYPES = (np.float32, np.float16)
FILLS = (0.0, 1e-3)


def shapes(types=2):
    """(M, H, K, V, input type, gradient type, masked, small_fill): every size with every height and (K, V); `types` 2: with every
    pair of element types, 1: the pairs go round.  The (7, 7) and (1, 1) calls carry a valid mask.  small_fill goes round."""
    res = []
    for n, (M, H, (K, V)) in enumerate(itertools.product(SIZES, HEIGHTS, KV)):
        pairs = list(itertools.product(TYPES, TYPES))
        for q, (dt, gt) in enumerate(pairs if types == 2 else [pairs[n % 4]]):
            res.append((M, H, K, V, dt, gt, V == K and M > 1, FILLS[(n + q + n // 6) % 2]))
    return res


def shape_id(s):
    return f"M{s[0]}-H{s[1]}-K{s[2]}-V{s[3]}-{np.dtype(s[4]).name}-grad_{np.dtype(s[5]).name}-fill{s[7]:g}" + ("-masked" if s[6] else "")


@pytest.fixture(scope="module")
def window_of():
    """one recorded window per engine and height, shared and left unchanged"""
    made = {}

    def get(kind, H):
        if (kind, H) not in made:
            made[(kind, H)] = crafted_window(kind, H)
        return made[(kind, H)]
    yield get
    for w in made.values():
        w.b.close()


def grad_scale_for(gt):
    return 1.0 if np.dtype(gt) == np.float32 else 1024.0          # (float16 gradients: the range an AMP loss scale is for)


def prepare(kind, window_of, shape, seed, prm, ties=True, carry=None):
    """inputs, index list, the planes batch_plan gives, ok, with prob_old placed around the model's probabilities.  carry =
    (last_valid, span): the mask of plan_loss_support.carry_mask over blocks of 16, and the indices of block 5 name no entry."""
    M, H, K, V, dt, gt, masked, fill = shape
    w = window_of(kind, H)
    rng = np.random.default_rng(seed)
    index = sample_index(rng, M, w.total)
    inp = plan_inputs(rng, M, H, K, V, dt, masked, ties=ties)
    if carry:
        inp["valid"] = carry_mask(rng, M, BLOCK, *carry)
        weigh_the_full_slots(inp["target"], BLOCK)
        index[5 * BLOCK:6 * BLOCK] = np.resize([-1, w.total, (w.total + 5) | MIRROR, 0x7FFFFFFF], BLOCK)
    delta, sums = w.planes(index, fill)
    ok = ok_of(inp, index, w.total)
    m = plan_model(F32, inp["phi"], inp["v"], delta, sums, inp["piece"], inp["old"], inp["adv"], inp["target"], ok, prm)
    with_old(inp, m["probability"], rng)
    return w, inp, index, delta, sums, ok


def model(ft, inp, delta, sums, ok, prm, gs=1.0):
    return plan_model(ft, inp["phi"], inp["v"], delta, sums, inp["piece"], inp["old"], inp["adv"], inp["target"], ok, prm, gs)


# ---------------------------------------------------------------- 1. bit equality
BITS_PRM = PlanParams(0.15, 0.3, 1.0, 0.0, 0.25)                 # entropy_loss = 0: grad_phi carries the float32 model's bits


def plan_bits(kind, window_of, shape, carry=None):
    """A call with entropy_loss = 0 against the float32 model: the per-sample outputs and both gradient arrays bit for bit, every
    entry written, zeros outside the piece's plane and for samples that are not valid, nothing past M (Buf.get checks the guard
    bytes), D exact -> (outputs, model, window, inputs, index, ok)"""
    M, H, K, V, dt, gt, masked, fill = shape
    prm = BITS_PRM
    w, inp, index, delta, sums, ok = prepare(kind, window_of, shape, 100 * M + 10 * K + V + H, prm, carry=carry)
    gs = grad_scale_for(gt)
    got = PlanLossCall(kind, w.b, w.plan, inp, index, prm, fill, grad_dtype=gt, grad_scale=gs, stride3=M % 2 == 1).run(w.b)
    m = model(F32, inp, delta, sums, ok, prm, gs)
    for row, name in ((0, "probability"), (1, "ratio"), (2, "pl"), (4, "I"), (5, "val")):
        assert same_bits(got["terms"][row], m[name]), f"'{name}' differs in samples {np.nonzero(got['terms'][row] != m[name])[0][:8]}"
    want, want_v = expand(m["g"], m["k"], K, gt), expand_v(m["gv"], m["k"], V, gt)
    assert written(got["grad_phi"], want) and written(got["grad_v"], want_v) and written(got["terms"]) and written(got["stats"])
    assert same_bits(got["grad_v"], want_v), "grad_v"
    assert same_bits(got["grad_phi"], want), f"grad_phi differs in samples {np.unique(np.nonzero(got['grad_phi'] != want)[0])[:8]}"
    other = np.ones((M, 10 * H, K), bool)
    other[np.arange(M), :, m["k"]] = False
    assert not got["grad_phi"].reshape(M, 10 * H, K)[other].any(), "a non-zero outside the piece's plane"
    assert not got["grad_phi"][~ok].any() and not got["terms"][:, ~ok].any(), "a sample that is not valid"
    assert got["stats"][0] == m["D"] == ok.sum() and got["stats"][4] == 0.0
    return got, m, w, inp, index, ok


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("shape", shapes(), ids=shape_id)
def test_equals_the_model_bit_for_bit(kind, shape, window_of):
    """entropy_loss = 0: probability, ratio, pl, the impossibility sum, val, grad_v and all of grad_phi carry the model's bits.
    Every entry of both gradient arrays is written, zeros outside the piece's plane, nothing past M (guard bytes)."""
    M, K = shape[0], shape[2]
    got, m, w, inp, index, ok = plan_bits(kind, window_of, shape)
    if M == 33:                                                   # every branch occurred
        ratio, cl, A, s, raw = m["ratio"], m["cl"], m["A"], m["s"][ok], m["raw"][ok]
        for sign in (A > 0, A < 0):
            assert (ok & sign & (ratio < cl)).any() and (ok & sign & (ratio > cl)).any()
        assert (ok & (ratio == cl)).any()
        assert (s == 0).any() and (s > 1).any() and (s < 0).any(), "no cell without a list, with several, or that lists clear"
        assert (raw < 1e-6).any() and (raw > 1).any() and ((raw > 1e-6) & (raw < 1)).any()
        assert (index[ok] & MIRROR).any() and (~named(index, w.total)).sum() >= 3 and (inp["piece"] > K - 1).any()
        kinds = w.kinds()[(index & 0x7FFFFFFF)[named(index, w.total)]]
        assert set(np.unique(w.kinds())) == {0, 1, 2} and len(np.unique(kinds)) >= 2, "chosen lists of kind NORMAL, SMALL and PAST"


# ---------------------------------------------------------------- 2. what passes through the logarithm
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("shape", shapes(types=1), ids=shape_id)
def test_entropy_outputs_against_float64(kind, shape, window_of):
    """Hent and, with entropy_loss != 0 and policy_loss = 0 (the policy part: section 1), grad_phi against the same formulas in
    float64, within plan_loss_support.entropy_tolerances.  The indicator [y_t > e] cannot flip between the two: no x_t s_t / S of the
    inputs lies in (0, 1e-12), which the test asserts (below 5.7e-14 the float32 sum with e rounds to e).  Measured on the MI355X
    over these cases: Hent within 4.95e-7, 0.5 % of its allowance; grad_phi within 94 % of its allowance, reached where the output
    is float16, whose own rounding nearly fills it."""
    M, H, K, V, dt, gt, masked, fill = shape
    prm = PlanParams(0.15, 0.3, 0.0, 0.5, 0.25)
    w, inp, index, delta, sums, ok = prepare(kind, window_of, shape, 1000 * M + 10 * K + V + H, prm)
    gs = grad_scale_for(gt) * 16.0
    got = PlanLossCall(kind, w.b, w.plan, inp, index, prm, fill, grad_dtype=gt, grad_scale=gs).run(w.b)
    m = model(F64, inp, delta, sums, ok, prm, gs)
    q = (m["b"] / m["S"][:, None])[ok]
    assert not ((q > 0) & (q < 1e-12)).any(), "a cell's share of the entropy lies where float32 cannot tell it from zero"
    assert not m["g_policy"][ok].any()
    tol_H, tol_g = entropy_tolerances(m, gt)
    err_H = np.abs(got["terms"][3] - m["Hent"])
    if np.dtype(gt) == np.float16:
        assert np.abs(m["g"]).max() < 6e4, "the scaled gradients leave the range of a float16"
    err_g = np.abs(got["grad_phi"].astype(F64) - expand(m["g"], m["k"], K, F64))
    full_tol = expand(tol_g, m["k"], K, F64)
    print(f"Hent: largest error {err_H.max():.3g}, largest share of its tolerance {(err_H / np.maximum(tol_H, 1e-300)).max():.3g}; "
          f"grad_phi: {err_g.max():.3g}, largest share {(err_g / np.maximum(full_tol, 1e-300)).max():.3g}")
    assert (err_H <= tol_H).all()
    assert (err_g <= full_tol).all()
    if M == 33:
        assert (np.abs(m["g_entropy"])[ok] > 0).any() and (m["Hent"][ok] != 0).all()


# ---------------------------------------------------------------- 3. the model against autograd of the reference's expressions
def autograd_case(w, prm, K, V, masked, M=33, seed=0, adjust=None):
    """the float64 model and torch autograd of the reference's expressions on the same inputs: M samples of the window w, every index
    naming an entry, raw strictly inside (e, 1), small_fill = 0; adjust(inp, ok, m) may then move inputs onto a tie (prob_old
    may become a float64 array: both sides take it as it is)"""
    import torch
    rng = np.random.default_rng(seed)
    index = sample_index(rng, M, w.total)
    index = np.where(named(index, w.total), index, 3)                        # (the mask alone selects)
    inp = plan_inputs(rng, M, w.b.height, K, V, np.float32, masked, ties=False)
    delta, sums = w.planes(index, 0.0)
    ok = ok_of(inp, index, w.total)
    m = model(F64, inp, delta, sums, ok, prm)
    with_old(inp, m["probability"], rng)
    inp["old"] = np.maximum(inp["old"], F32(1e-3))
    if adjust:
        adjust(inp, ok, m)
    m = model(F64, inp, delta, sums, ok, prm)
    phi = torch.from_numpy(inp["phi"].astype(F64)).requires_grad_()
    v = torch.from_numpy(inp["v"].astype(F64)).requires_grad_()
    loss, probability, r, entropy = torch_plan_loss(torch, phi, v, delta, sums, inp["piece"], inp["old"], inp["adv"], inp["target"], ok, prm)
    g_phi, g_v = torch.autograd.grad(loss, (phi, v))
    return inp, m, ok, float(loss.detach()), g_phi.numpy(), g_v.numpy(), probability.detach().numpy(), entropy.detach().numpy()


@pytest.mark.parametrize("prm", PARAM_SETS, ids=["set0", "set1", "set2"])
@pytest.mark.parametrize("K,V,masked", [(7, 7, False), (7, 1, True), (1, 1, False)])
def test_the_float64_model_against_torch_autograd(prm, K, V, masked, window_of):
    """d loss / d phi and d loss / d v of the float64 model against torch autograd (float64, CPU) of delta_ppo_nets.py:30 and
    150-182 written line by line with torch ops, inputs without ties.  Allowance: both sides round in float64; a gradient element
    is a sum of three parts, the policy part itself the quotient by den2 of a difference d_t - p s_t that may cancel, behind
    which stand three sums of HW terms in different orders: 1e-10 of the largest gradient, 4.5e5 float64 epsilons, as
    tests/test_loss_head.py allows the PPO model."""
    inp, m, ok, loss, want_phi, want_v, probability, entropy = autograd_case(window_of("harness", 20), prm, K, V, masked, seed=11 + K + V)
    assert (m["ratio"] != 1 - F64(F32(prm.clip))).all() and (m["ratio"] != 1 + F64(F32(prm.clip))).all()
    assert ((m["raw"] > 1e-6) & (m["raw"] < 1)).all() and (np.abs(m["g_policy"]) > 0).any() and (np.abs(m["g_entropy"]) > 0).any()
    err_phi = np.abs(expand(m["g"], m["k"], K, F64) - want_phi).max()
    err_v = np.abs(expand_v(m["gv"], m["k"], V, F64) - want_v).max()
    print(f"largest gradients {np.abs(want_phi).max():.3g} / {np.abs(want_v).max():.3g}, largest differences {err_phi:.3g} / {err_v:.3g}")
    assert err_phi <= 1e-10 * np.abs(want_phi).max() and err_v <= 1e-10 * np.abs(want_v).max()
    assert np.allclose(m["probability"][ok], probability, rtol=1e-11, atol=0) and np.allclose(m["Hent"][ok], entropy, rtol=1e-11, atol=1e-15)
    t = m["terms"][ok].sum(axis=0) / m["D"]
    c1, c2, c3, c4 = (F64(F32(z)) for z in prm[1:])
    mine = ((c1 * t[0] - c2 * t[1]) + c4 * t[11] / (10 * inp["phi"].shape[1])) - c3 * t[2]
    assert mine == pytest.approx(loss, rel=1e-11, abs=1e-12)


@pytest.mark.parametrize("tie", ["raw_at_e", "raw_at_1", "y_at_e", "ratio_at_lower_bound", "ratio_at_upper_bound"])
def test_the_tie_rules_against_torch_autograd(tie, window_of):
    """raw exactly at e and at 1 (clip_by_value sends the gradient to its input: it passes), y_t exactly at e (a cell with s_t = 0;
    tf.maximum(1e-6, y) sends the gradient to the constant: the model's entropy part is zero there, and so is autograd's, whose
    dy/dx = s_t / S vanishes), and a ratio exactly on a clip bound (the clipped ratio passes): the model's rule is the one
    autograd applies; torch.clamp's gradient, like tf.clip_by_value's, passes on both bounds."""
    prm, K, V = PARAM_SETS[1], 7, 7
    lo, hi = 1 - F64(F32(prm.clip)), 1 + F64(F32(prm.clip))
    bound = lo if tie.endswith("lower_bound") else hi

    def adjust(inp, ok, m):
        rows = np.arange(len(ok))
        plane = inp["phi"].reshape(len(ok), -1, K)
        if tie == "raw_at_e":
            plane[rows, ::3, m["k"]] = E32
        elif tie == "raw_at_1":
            plane[rows, ::3, m["k"]] = 1.0
        elif tie.startswith("ratio"):
            inp["old"] = np.maximum(m["probability"], F64(E32)) / bound           # float64: the quotient by it is the bound for most samples
    inp, m, ok, loss, want_phi, want_v, probability, entropy = autograd_case(window_of("harness", 20), prm, K, V, False, seed=5, adjust=adjust)
    got = expand(m["g"], m["k"], K, F64)
    close = np.abs(got - want_phi).max(axis=(1, 2, 3)) <= 1e-10 * np.abs(want_phi).max()
    assert close.all(), f"samples {np.nonzero(~close)[0][:8]} differ from autograd"
    if tie.startswith("raw"):
        at = m["raw"] == (F64(E32) if tie == "raw_at_e" else 1.0)
        assert at.sum() >= 60 * len(ok) and m["passes"][at].all() and (np.abs(m["g"][at]) > 0).any(), "the gradient passes at the tie"
    elif tie == "y_at_e":
        at = (m["s"] == 0) & ok[:, None]
        assert at.any() and (m["y"][at] == F64(E32)).all() and not m["g_entropy"][at].any(), "the constant takes the gradient: no entropy part"
    else:
        hit = ok & (m["ratio"] == bound) & (np.abs(m["g_policy"]).max(axis=1) > 0)
        assert hit.sum() >= 3 and (m["cl"][hit] == m["ratio"][hit]).all(), "no sample with its ratio exactly on the bound and a policy gradient"


# ---------------------------------------------------------------- 4. statistics
def stat_check(name, got, terms, coef, D, term_err=0.0, bound=None):
    """got against coef * sum(terms) / D in float64: the summation bound of the float32 sum — in any order, or `bound`, that of
    the stated order (loss_support.stated_bound) — plus the terms' own error, through the divisions and the product (three
    roundings, and one more for a sum of such statistics)"""
    terms = np.asarray(terms, F64)
    want = coef * terms.sum() / D
    tol = abs(coef) * ((sum_bound(terms) if bound is None else bound) + np.sum(term_err)) / D + 4 * U24 * abs(want) + 1e-45
    print(f"{name}: got {got:.9g}, want {want:.9g}, difference {abs(got - want):.3g}, allowed {tol:.3g}")
    assert abs(got - want) <= tol, name
    return want, tol


def stats_in_the_stated_order(got, m32, prm, H):
    """Every statistic bit for bit: the sum of its per-sample float32 terms in the stated order (loss_support.stated_sum with
    blocks of 16), then the definition's divisions and products in float32.  The terms that carry the float32 model's bits come
    from the model; Hent, which passes through the logarithm, is the row the call itself wrote to `terms` — the head sums the
    very value it writes, and section 2 holds that row against float64 —, and Hent^2 is the float32 square of that Hent."""
    t = m32["terms"].copy()
    Hent = got["terms"][3]
    t[:, 2], t[:, 3] = Hent, Hent * Hent
    want = plan_stated_stats(t, m32["D"], prm, H)
    for slot, name in enumerate(STATS):
        assert same_bits(got["stats"][slot], want[slot]), f"'{name}' is {got['stats'][slot]!r}, the sum in the stated order gives {want[slot]!r}"
    assert not got["stats"][len(STATS):].any()


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("shape", shapes(types=1), ids=shape_id)
def test_statistics_and_determinism(kind, shape, window_of):
    """Every statistic against the float64 sum of the model's per-sample terms — the float32 model's for the terms that carry its
    bits (section 1), the float64 model's with the per-sample tolerance of section 2 for Hent and Hent^2 —; then every statistic
    bit for bit against the sum in the stated order (stats_in_the_stated_order).  D counts the mask and the indices that name
    no entry.  A second call gives the same bytes in every output."""
    M, H, K, V, dt, gt, masked, fill = shape
    prm = PARAM_SETS[1]
    w, inp, index, delta, sums, ok = prepare(kind, window_of, shape, 50 * M + K + V + H, prm)
    call = PlanLossCall(kind, w.b, w.plan, inp, index, prm, fill, grad_dtype=gt, grad_scale=128.0)
    got = call.run(w.b)
    stats = dict(zip(STATS, got["stats"].astype(F64)))
    m32, m64 = model(F32, inp, delta, sums, ok, prm, 128.0), model(F64, inp, delta, sums, ok, prm, 128.0)
    D = m32["D"]
    assert stats["n"] == D == ok.sum() and not got["stats"][len(STATS):].any()
    if D == 0:
        assert not got["stats"].any()
        return
    t32, t64 = m32["terms"][ok].astype(F64), m64["terms"][ok]
    tol_H = entropy_tolerances(m64, gt)[0][ok]
    c1, c2, c3, c4 = (float(F32(z)) for z in prm[1:])
    vl = stat_check("value_loss", stats["value_loss"], t32[:, 0], c1, D)
    pol = stat_check("policy_loss", stats["policy_loss"], t32[:, 1], -c2, D)
    imp = stat_check("impossibility_loss", stats["impossibility_loss"], t32[:, 11], c4 / (10 * H), D)
    ent = stat_check("entropy_loss", stats["entropy_loss"], t64[:, 2], -c3, D, tol_H)
    want = vl[0] + pol[0] + imp[0] + ent[0]
    tol = vl[1] + pol[1] + imp[1] + ent[1] + 3 * U24 * (abs(vl[0]) + abs(pol[0]) + abs(imp[0]) + abs(ent[0]))
    print(f"loss: got {stats['loss']:.9g}, want {want:.9g}, allowed {tol:.3g}")
    assert abs(stats["loss"] - want) <= tol
    stat_check("entropy", stats["entropy"], t64[:, 2], 1.0, D, tol_H)
    stat_check("entropy_sq", stats["entropy_sq"], t64[:, 3], 1.0, D, 2 * np.abs(t64[:, 2]) * tol_H + tol_H ** 2 + U24 * t64[:, 3])
    for name, col in (("values", 4), ("values_sq", 5), ("target_values", 6), ("target_values_sq", 7), ("clip_saturation", 8), ("ratio", 9),
                      ("probability", 10)):
        stat_check(name, stats[name], t32[:, col], 1.0, D)
    stats_in_the_stated_order(got, m32, prm, H)
    again = call.run(w.b)
    for name in got:
        assert got[name].tobytes() == again[name].tobytes(), f"'{name}' of a second call differs"


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("dt", TYPES, ids=["float32", "float16"])
def test_a_call_without_a_valid_sample_gives_zeros(kind, dt, window_of):
    """D == 0 (the reference would give NaN), once by the mask and once by indices that name no entry: every output is written,
    and is zero"""
    M, H, K = 17, 20, 7
    w = window_of(kind, H)
    rng = np.random.default_rng(3)
    inp = plan_inputs(rng, M, H, K, K, dt, True)
    index = sample_index(rng, M, w.total)
    inp["valid"][:] = 0
    for name, a in PlanLossCall(kind, w.b, w.plan, inp, index, PARAM_SETS[0], 1e-3, grad_dtype=dt).run(w.b).items():
        assert written(a) and not a.any(), name
    inp["valid"][:] = 1
    for name, a in PlanLossCall(kind, w.b, w.plan, inp, np.full(M, -1), PARAM_SETS[0], 1e-3, grad_dtype=dt).run(w.b).items():
        assert written(a) and not a.any(), name


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_no_samples_zeroes_the_statistics(kind, window_of):
    w = window_of(kind, 20)
    inp = plan_inputs(np.random.default_rng(4), 1, 20, 7, 1, np.float32, False)
    got = PlanLossCall(kind, w.b, w.plan, inp, [0], PARAM_SETS[0], 0.0, m=0).run(w.b)
    assert written(got["stats"]) and not got["stats"].any() and not written(got["grad_phi"]) and not written(got["grad_v"])


# ---------------------------------------------------------------- 5. batches whose loops take a second trip
CARRY_SIZES = (1025, 4097, 5123, 8209)


def carry_shapes():
    """(shape as in shapes(), (last_valid, span)) at the sizes where the single-workgroup loops behind the head go round again — the
    count of D is one workgroup of 1024 lanes that strides over M, the reduction of the blocks' partial rows one of 256 lanes that
    strides over the blocks of 16:
      M = 1025 = 64 x 16 + 1    one lane of the count has a second trip; 65 blocks
      M = 4097 = 256 x 16 + 1   5 trips of the count; 257 blocks: slot 0 takes a second row, and the last block holds one sample
      M = 5123 = 5 x 1024 + 3   lanes 0-2 count six samples, the others five; 321 blocks: slots 0-64 take a second row
      M = 8209 = 513 x 16 + 1   9 trips; 514 blocks: slots 0 and 1 take a third row
    Every size with every (K, V); the heights, the element type pairs and small_fill go round.  Every call carries a valid mask
    (plan_loss_support.carry_mask over blocks of 16) and an index list with repeats and with entries that name nothing, a whole
    block of them: the second (K, V) of a size has its last sample valid, the others invalid; from M = 4097 on every mask has 1024
    consecutive invalid samples, so D lies more than 1024 below M.  At M = 1025 such a run leaves one sample at most, so no D
    there can lie more than 1024 from M without being 0: the third (K, V) takes the run, with the last sample valid (D = 1)."""
    res = []
    pairs = list(itertools.product(TYPES, TYPES))
    for n, (M, (i, (K, V))) in enumerate(itertools.product(CARRY_SIZES, enumerate(KV))):
        dt, gt = pairs[n % 4]
        res.append(((M, HEIGHTS[(n + 1) % 2], K, V, dt, gt, True, FILLS[(n // 2) % 2]), (i == 1 or (M == 1025 and i == 2), M > 1025 or i == 2)))
    assert {s[0][7] for s in res} == set(FILLS) and all({s[0][1] for s in res if s[0][0] == M} == set(HEIGHTS) for M in CARRY_SIZES)
    return res


def carry_id(case):
    return shape_id(case[0]).replace("-masked", "") + f"-last_{'valid' if case[1][0] else 'invalid'}" + ("-run1024" if case[1][1] else "")


def check_carry_inputs(w, inp, index, ok, D, carry):
    """the mask and the index list are what the case needs, and a count that drops or doubles a trip of 1024 lanes cannot land on
    this D"""
    M = len(ok)
    assert_carry_mask(ok, BLOCK, *carry)
    is_named = named(index, w.total)
    assert not is_named[5 * BLOCK:6 * BLOCK].any() and (inp["valid"][5 * BLOCK:6 * BLOCK] != 0).any() == (M > 1025 or not carry[1])
    assert len(np.unique(index[is_named])) < is_named.sum(), "no entry is named twice"
    assert D == 1 or ((index[ok] & MIRROR).any() and not (index[ok] & MIRROR).all())
    assert D == ok.sum() and D % 1024 != 0
    if M > 1025:
        assert M - D > 1024


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("case", carry_shapes(), ids=carry_id)
def test_equals_the_model_bit_for_bit_across_the_carries(kind, case, window_of):
    """Section 1's comparison (plan_bits) at the sizes of carry_shapes: every per-sample output and both gradient arrays bit for
    bit, D exact; and every statistic in the stated order."""
    shape, carry = case
    got, m, w, inp, index, ok = plan_bits(kind, window_of, shape, carry)
    check_carry_inputs(w, inp, index, ok, got["stats"][0], carry)
    stats_in_the_stated_order(got, m, BITS_PRM, shape[1])


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("case", carry_shapes(), ids=carry_id)
def test_statistics_and_determinism_across_the_carries(kind, case, window_of):
    """With every loss coefficient non-zero: D exact; Hent of every sample against float64 within section 2's tolerance (so that
    summing the written row is not circular); every statistic bit for bit in the stated order — at these sizes the slots of the
    order take more than one row —; entropy_sq also against the float64 sum with the bound of the stated order
    (loss_support.stated_bound) and section 4's per-sample error of Hent^2; a second call gives the same bytes in every output."""
    shape, carry = case
    M, H, K, V, dt, gt, masked, fill = shape
    prm = PARAM_SETS[1]
    w, inp, index, delta, sums, ok = prepare(kind, window_of, shape, 50 * M + K + V + H, prm, carry=carry)
    call = PlanLossCall(kind, w.b, w.plan, inp, index, prm, fill, grad_dtype=gt, grad_scale=128.0)
    got = call.run(w.b)
    m32, m64 = model(F32, inp, delta, sums, ok, prm, 128.0), model(F64, inp, delta, sums, ok, prm, 128.0)
    D = m32["D"]
    assert written(got["terms"]) and written(got["stats"])        # (the gradient arrays: the test above)
    check_carry_inputs(w, inp, index, ok, got["stats"][0], carry)
    assert got["stats"][0] == D
    tol_H = entropy_tolerances(m64, gt)[0]
    assert (np.abs(got["terms"][3] - m64["Hent"]) <= tol_H).all()
    stats_in_the_stated_order(got, m32, prm, H)
    t64, tol_H = m64["terms"][ok], tol_H[ok]
    stat_check("entropy_sq", float(got["stats"][7]), t64[:, 3], 1.0, D, 2 * np.abs(t64[:, 2]) * tol_H + tol_H ** 2 + U24 * t64[:, 3],
               bound=stated_bound(t64[:, 3], BLOCK))
    again = call.run(w.b)
    for name in got:
        assert got[name].tobytes() == again[name].tobytes(), f"'{name}' of a second call differs"


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_the_scratch_buffer_grows_between_calls(kind):
    """On a window of its own, so that the first call finds no scratch: a call at M = 33 (three partial rows), one at M = 8209 (514
    rows: the scratch is replaced while the first call may still run) and the first again, enqueued one after the other — the
    outputs are read only after the third.  The third call's outputs are the first's byte for byte, the large call's are those
    of the same call on a fresh window with the same records, and no error is pending."""
    H, K, prm = 7, 7, PARAM_SETS[1]
    made = {}

    def own_window(kind_, H_):
        return made.setdefault("w", crafted_window(kind_, H_))
    fresh = None
    try:
        prepared = [prepare(kind, own_window, (M, H, K, K, np.float32, np.float32, True, 1e-3), 7 * M, prm) for M in (33, CARRY_SIZES[-1])]
        w = made["w"]
        (_, small, small_index, *_), (_, large, large_index, *_) = prepared
        calls = [PlanLossCall(kind, w.b, w.plan, inp, index, prm, 1e-3, grad_scale=128.0)
                 for inp, index in ((small, small_index), (large, large_index), (small, small_index))]
        for call in calls:
            w.b.plan_loss_dev(w.plan, call.l)
        first, big, third = (call.get() for call in calls)
        assert all(written(a) for got in (first, big, third) for a in got.values())
        assert first["stats"][0] == prepared[0][5].sum() and big["stats"][0] == prepared[1][5].sum() > 8000
        for name in first:
            assert third[name].tobytes() == first[name].tobytes(), f"the small call after the large one: '{name}' differs"
        fresh = crafted_window(kind, H)
        assert fresh.bufs["rec"].get().tobytes() == w.bufs["rec"].get().tobytes()
        alone = PlanLossCall(kind, fresh.b, fresh.plan, large, large_index, prm, 1e-3, grad_scale=128.0).run(fresh.b)
        for name in big:
            assert big[name].tobytes() == alone[name].tobytes(), f"the large call after a small one: '{name}' differs"
        assert w.b.take_errors() == 0 and fresh.b.take_errors() == 0
    finally:
        for win in (made.get("w"), fresh):
            if win is not None:
                win.b.close()


# ---------------------------------------------------------------- 6. the reference's own planes
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_the_fixtures_planes(kind):
    """The episodes of tests/golden/traj_plan.npz through a window (plan_loss_support.golden_window): the head on those records
    with small_fill = 0 against the float64 model fed the delta / delta_sum the reference's trajectory recorded, within the
    tolerances of section 2; what does not pass through the logarithm carries the bits of the float32 model fed the same planes."""
    w, index, steps, z = golden_window(kind)
    try:
        M, K, V = len(index), 7, 7
        assert M == len(z["a_idx"])
        delta, sums = z["out5"][steps][..., 0].astype(F32), z["out6"][steps][..., 0].astype(F32)
        mine = w.planes(index, 0.0)
        assert np.array_equal(mine[0], delta) and np.array_equal(mine[1], sums), "batch_plan does not give the fixture's planes"
        rng = np.random.default_rng(8)
        inp = plan_inputs(rng, M, 20, K, V, np.float32, False)
        inp["piece"] = z["piece"][steps].astype(np.uint8)
        ok = np.ones(M, bool)
        prm = PlanParams(0.15, 0.3, 0.0, 0.5, 0.25)
        with_old(inp, model(F32, inp, delta, sums, ok, prm)["probability"], rng)
        got = PlanLossCall(kind, w.b, w.plan, inp, index, prm, 0.0, grad_scale=16.0).run(w.b)
        m = model(F64, inp, delta, sums, ok, prm, 16.0)
        tol_H, tol_g = entropy_tolerances(m, F32)
        err_H = np.abs(got["terms"][3] - m["Hent"])
        err_g = np.abs(got["grad_phi"].astype(F64) - expand(m["g"], m["k"], K, F64))
        full_tol = expand(tol_g, m["k"], K, F64)
        print(f"{M} samples; Hent: largest error {err_H.max():.3g}, largest share of its tolerance {(err_H / np.maximum(tol_H, 1e-300)).max():.3g}; "
              f"grad_phi: {err_g.max():.3g}, largest share {(err_g / np.maximum(full_tol, 1e-300)).max():.3g}")
        assert (err_H <= tol_H).all() and (err_g <= full_tol).all()
        m32 = model(F32, inp, delta, sums, ok, prm, 16.0)
        for row, name in ((0, "probability"), (1, "ratio"), (2, "pl"), (4, "I"), (5, "val")):
            assert same_bits(got["terms"][row], m32[name]), name
        assert (np.abs(m["g_entropy"]) > 0).any() and (delta < 0).any() and (sums > 1).any()
    finally:
        w.b.close()


# ---------------------------------------------------------------- 7. argument rules
RULES = [("the struct is NULL", None), ("phi is NULL", dict(phi=None)), ("v is NULL", dict(v=None)), ("index is NULL", dict(index=None)),
         ("piece is NULL", dict(piece=None)), ("prob_old is NULL", dict(prob_old=None)), ("adv is NULL", dict(adv=None)),
         ("target is NULL", dict(target=None)), ("grad_phi is NULL", dict(grad_phi=None)), ("grad_v is NULL", dict(grad_v=None)),
         ("stats is NULL", dict(stats=None)), ("negative M", dict(m=-1)), ("K = 3", dict(n_pieces=3)), ("V = 2", dict(n_values=2)),
         ("negative clip", dict(clipping_parameter=-0.1)), ("NaN clip", dict(clipping_parameter=float("nan"))), ("an unknown flag", dict(flags=8)),
         ("piece_stride 0", dict(piece_stride=0)), ("misaligned phi", "phi"), ("misaligned grad_phi", "grad_phi"),
         ("a window without records", "no_rec"), ("a NULL window", "no_plan"), ("three players", 3), ("four players", 4), ("a split batch", "split")]


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("rule", RULES, ids=[r[0].replace(" ", "_") for r in RULES])
def test_bad_arguments_are_refused(kind, rule, window_of):
    pkg, w = ge.package(), window_of(kind, 20)
    rng = np.random.default_rng(1)
    inp = plan_inputs(rng, 5, 20, 7, 7, np.float32, True)
    index = sample_index(rng, 5, w.total)
    b, plan, what, kw = w.b, w.plan, rule[1], {}
    other = None
    try:
        if isinstance(what, dict):
            kw = what
        elif what in (3, 4):
            b = other = engines.make(kind, 4, what)
        elif what == "split":
            b = other = pkg.TetrisBatch(4, 2, 20, 10, split_side=0, **(dict(lib_path=ge.build_harness()) if kind == "harness" else dict(device=0)))
        elif what == "no_rec":
            plan = b.traj_plan(w.T, None)
        elif what == "no_plan":
            plan = None
        call = PlanLossCall(kind, b, plan, inp, index, PARAM_SETS[0], 0.0, **kw)
        if what in ("phi", "grad_phi"):
            ptr = (call.inp if what == "phi" else call.out)[what].ptr + 8
            call = PlanLossCall(kind, b, plan, inp, index, PARAM_SETS[0], 0.0, **{what: ptr})
        with pytest.raises(pkg.TetrisError):
            b.plan_loss_dev(plan, None if what is None else call.l)
        assert not any(written(a) for a in call.get().values()), "a refused call wrote an output"
    finally:
        if other is not None:
            other.close()


# ---------------------------------------------------------------- 8. TorchEnv (GPU only)
def composed_plan_loss(torch, phi, v, delta, sums, piece, old, adv, target, valid, prm):
    """the same loss composed from batch_plan's planes and torch ops on the device, float32: what a user runs without the head"""
    M, K = phi.shape[0], phi.shape[3]
    e = 1e-6
    rows = torch.arange(M, device=phi.device)
    k = piece.long()
    x = torch.clamp(phi, e, 1.0)[rows, :, :, k][..., None]
    val = v[rows, k] if v.shape[1] == K else v[:, 0]
    probability = ((x * delta).sum(dim=(1, 2, 3)) + e) / ((x * sums).sum(dim=(1, 2, 3)) + e)
    r = torch.clamp(probability, min=e) / torch.clamp(old, min=e)
    pl = torch.minimum(r * adv, torch.clamp(r, 1 - prm.clip, 1 + prm.clip) * adv)
    imp = x * (1 - torch.clamp(sums, max=1.0))
    y = x * sums / (sums + e).sum(dim=(1, 2, 3), keepdim=True) + e
    Hent = -(y * torch.log(torch.clamp(y, min=e))).sum(dim=(1, 2, 3))
    sel = valid != 0
    return prm.c1 * ((val - target) ** 2)[sel].mean() - prm.c2 * pl[sel].mean() + prm.c4 * imp[sel].mean() - prm.c3 * Hent[sel].mean()


def torch_window(torch, ti, n=64, T=2, L=32):
    """a TorchEnv with a recorded planning window of T rows: action_lists, observe, step_lists_eval, record_plan"""
    from oracle import oracle as orc
    b = engines.make("hip", n, 2, seeds=orc.episode_seed(np.arange(n), 2))
    b.rollout_random(1, 18)
    te = ti.TorchEnv(b)
    tr = te.trajectory(T, states=True, plan=True)
    gen = torch.Generator(device="cuda").manual_seed(5)
    for t in range(T):
        pt = ((torch.arange(n, device="cuda") + t) % 2).to(torch.uint8)
        te.action_lists(player=pt, max_lists=L)
        tr.observe(t, pt)
        te.step_lists_eval(torch.rand(n, 20, 10, 7, generator=gen, device="cuda") + 0.1, mode="pi", player=pt, seed=3, draw=t, planes=False)
        tr.record_plan(t)
    return b, te, tr


@pytest.mark.gpu
@pytest.mark.parametrize("M", [257, 64])
def test_plan_loss_backward_matches_the_composed_loss(M):
    """te.plan_loss(...).backward() on a small module — a linear layer to [M, 20, 10, 7] through a sigmoid scaled to reach below e
    and above 1, and a linear value head — leaves the parameter gradients of the same loss composed from batch_plan and torch
    ops.  grad_scale = 128 is undone.  Tolerance, as for the PPO wrapper (tests/test_loss_head.py): the head's gradient differs
    from autograd's float32 one by the error of section 2 in the entropy part and by float32 roundings elsewhere; both pass
    through the same backward of the module: 1e-4 of the largest gradient of a parameter tensor (measured: printed)."""
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    torch.manual_seed(M)
    dev = torch.device("cuda")
    b, te, tr = torch_window(torch, ti)
    try:
        n, T, K, F = 64, 2, 7, 24
        body, head = torch.nn.Linear(F, 20 * 10 * K).to(dev), torch.nn.Linear(F, K).to(dev)
        feat = torch.randn(M, F, device=dev)
        rng = np.random.default_rng(M)
        index = rng.integers(0, T * n, M).astype(np.int64)
        index[::2] |= MIRROR
        index[5] = -1
        idx = torch.from_numpy(index.astype(np.uint32).view(np.int32)).to(dev)
        action = torch.from_numpy(np.stack([rng.integers(0, 32, M), np.zeros(M, np.int64), rng.integers(0, K, M)], axis=1).astype(np.uint8)).to(dev)
        adv, target = (torch.from_numpy(rng.standard_normal(M).astype(F32)).to(dev) for _ in range(2))
        valid_np = np.ones(M, np.uint8)
        valid_np[[0, M - 1, 5]] = 0
        valid = torch.from_numpy(valid_np).to(dev)
        prm = PARAM_SETS[1]

        def net():
            return 1.2 * torch.sigmoid(body(feat)).reshape(M, 20, 10, K) - 0.05, head(feat)
        planes = tr.batch_plan(idx, small_fill=0.0)
        with torch.no_grad():
            phi0, v0 = net()
            stats0, _, _, terms0 = te.plan_head(phi0.contiguous(), v0, tr, idx, action[:, 2], torch.ones(M, device=dev), adv, target, valid, small_fill=0.0,
                                                clipping_parameter=prm.clip, value_loss=prm.c1, policy_loss=prm.c2, entropy_loss=prm.c3,
                                                impossibility_loss=prm.c4, terms=True)
            old = (terms0[0].clamp(min=1e-3) / torch.from_numpy(np.choose(np.arange(M) % 3, [0.6, 1.01, 1.9]).astype(F32)).to(dev)).contiguous()
        params = list(body.parameters()) + list(head.parameters())
        phi, v = net()
        want_loss = composed_plan_loss(torch, phi, v, planes.delta, planes.sums, action[:, 2], old, adv, target, valid, prm)
        want = torch.autograd.grad(want_loss, params, retain_graph=True)
        loss, stats = te.plan_loss(phi, v, tr, idx, action[:, 2], old, adv, target, valid, small_fill=0.0, clipping_parameter=prm.clip,
                                   value_loss=prm.c1, policy_loss=prm.c2, entropy_loss=prm.c3, impossibility_loss=prm.c4, grad_scale=128.0)
        loss.backward()
        torch.cuda.synchronize()
        assert float(loss.detach()) == pytest.approx(float(want_loss.detach()), rel=1e-5, abs=1e-6) and float(stats[0]) == float((valid != 0).sum())
        for prm_t, w_ in zip(params, want):
            got = prm_t.grad / 128.0
            err, top = float((got - w_).abs().max()), float(w_.abs().max())
            print(f"parameter {tuple(prm_t.shape)}: largest gradient {top:.3g}, largest difference {err:.3g}")
            assert err <= 1e-4 * top
        b.set_stream(None, external=False)
    finally:
        b.close()


@pytest.mark.gpu
def test_plan_head_equals_the_c_level_call():
    """TorchEnv.plan_head (the pieces as the strided view action[:, 2]) against tetris_plan_loss_dev on buffers of the test's own,
    bit for bit, in both element types, with and without terms"""
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    dev = torch.device("cuda")
    b, te, tr = torch_window(torch, ti)
    try:
        n, T, K, M = 64, 2, 7, 77
        rng = np.random.default_rng(77)
        for dt, V in ((np.float32, 7), (np.float16, 1)):
            inp = plan_inputs(rng, M, 20, K, V, dt, True)
            index = sample_index(rng, M, T * n)
            with_old(inp, 0.3 * rng.random(M), rng)
            prm = PARAM_SETS[0]
            want = PlanLossCall("hip", b, tr._plan, inp, index, prm, 1e-3, grad_dtype=dt, grad_scale=64.0).run(b)
            action = np.zeros((M, 3), np.uint8)
            action[:, 2] = inp["piece"]
            tt = {name: torch.from_numpy(a).to(dev) for name, a in inp.items() if a is not None}
            got = te.plan_head(tt["phi"], tt["v"], tr, torch.from_numpy(index.astype(np.uint32).view(np.int32)).to(dev), torch.from_numpy(action).to(dev)[:, 2],
                               tt["old"], tt["adv"], tt["target"], tt["valid"], small_fill=1e-3, clipping_parameter=prm.clip, value_loss=prm.c1,
                               policy_loss=prm.c2, entropy_loss=prm.c3, impossibility_loss=prm.c4, grad_scale=64.0, terms=True)
            torch.cuda.synchronize()
            for name, t in zip(("stats", "grad_phi", "grad_v", "terms"), got):
                assert t.cpu().numpy().tobytes() == want[name].tobytes(), f"plan_head: '{name}' differs from the C-level call"
        b.set_stream(None, external=False)
    finally:
        b.close()
